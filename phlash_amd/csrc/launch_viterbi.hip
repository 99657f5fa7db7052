// Viterbi decoding (max-product): the single most probable hidden path of every sequence and its log probability.
// One translation unit per (real, K), compiled with -DPHK_REAL=float|double -DPHK_K=<K> -DPHK_SUFFIX=<tag> (see the
// Makefile: launch_viterbi_<real>_<K>.o).
//
// The O(K) form of the transition matrix survives the change of semiring.  With A[i][j] = b[j] (i > j), d[j] (i == j),
// u[i] v[j] (i < j), one step is
//     delta'_j = e_j * max( v_j * max_{i<j} u_i delta_i,  d_j delta_j,  b_j * max_{i>j} delta_i ):
// an exclusive prefix maximum of u .* delta and an exclusive suffix maximum of delta, serial inside a lane and by DPP row
// shifts across the R lanes of a sequence; which index a maximum came from is worked out for the states on the path only
// (vit_back_kernel).  All operands are >= 0, so 0 is the identity and DPP's zero fill is right.  The model is the folded
// one of the sum-product kernels (Lane::try_fold: the factor emis0_j multiplies column j of A whatever the reduction over
// i is), the rescale schedule is theirs (a power of two every NRM sites, here the exponent of the MAXIMUM), and so is the
// underflow rule.
// Ties: the lowest predecessor index wins, and the lowest final state.
//
// vit_fwd_kernel: the recursion alone, delta stored every T sites (16; float64: 8) into the handle's checkpoint slab (layout
// of Lane::ck_lane), logp = E ln 2 + log(max delta_n).
// vit_back_kernel: one group per sequence walks the blocks right to left; per block it re-runs the T steps from the
// checkpoint keeping the T delta vectors in registers, then walks back from the block's right-edge state: at every site
// the predecessor of the ONE state on the path is the arg-max of its K candidates, formed from the stored delta and that
// state's factors (three LDS reads, one arg-max butterfly), and writes the block's T path bytes.  (Carrying the indices
// of all K states through the scans of the re-run instead -- back-pointer vectors -- was the first version and costs
// more instructions per site: profiles/viterbi_timing.txt.)
//
// Rows of their own length (VArgs::lens): every sequence of a launch walks the same blocks; past its own length a
// sequence's delta is frozen (selects, no branch) and its path stays where it is, so its end state and logp are
// those of its last own site and the control flow stays wave-uniform.
//
// Lanes per sequence: R = K / 4 (4 states per lane) for every (real, K), as the posterior-decoding sweep.
#include "psmc_kernels.hip"
#include "sweep_common.h"

namespace phk {

// sites per block: a divisor of the 16 sites of an observation word.  The traceback keeps a block's delta vectors in registers:
// 16 x 4 float32 states are 64 VGPRs, and 8 float64 sites the same (with 16 the float64 kernels took 256 VGPRs and 70 AGPR copies)
template <typename real>
constexpr int vit_block() { return sizeof(real) == 8 ? 8 : 16; }
constexpr int VIT_T = vit_block<PHK_REAL>();
// kernel ids in the overrun record (KArgs::risk[1]; phk_underflow_risk names them)
constexpr int OVERRUN_VIT_FWD = 7;
constexpr int OVERRUN_VIT_BACK = 8;

template <int CTRL>
__device__ __forceinline__ int dppi_(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, false);
}

template <typename real, int K, int R>
struct VitLane {
    using L = Lane<real, K, R>;
    static constexpr int SPL = L::SPL;
    static_assert(SPL == SWEEP_SPL, "four states per lane");
    real b[SPL], d[SPL], u[SPL], v[SPL];
    const real* etab;
    int rank, k0;

    __device__ __forceinline__ void init(const L& lane, int rank_) {
        rank = rank_;
        k0 = rank_ * SPL;
        etab = lane.etab;
#pragma unroll
        for (int i = 0; i < SPL; ++i) {
            b[i] = L::get(lane.b, i);
            d[i] = L::get(lane.d, i);
            u[i] = L::get(lane.u, i);
            v[i] = L::get(lane.v, i);
        }
    }
    // maximum over the R lanes of the group (every lane gets it)
    __device__ __forceinline__ real gmax(real x) const {
        if constexpr (R >= 2) x = fmax_(x, dpp_<QP(1, 0, 3, 2)>(x));
        if constexpr (R >= 4) x = fmax_(x, dpp_<QP(2, 3, 0, 1)>(x));
        if constexpr (R >= 8) x = fmax_(x, dpp_<ROW_HALF_MIRROR>(x));
        if constexpr (R >= 16) x = fmax_(x, dpp_<ROW_MIRROR>(x));
        return x;
    }
    static __device__ __forceinline__ float fmax_(float a, float c) { return __builtin_fmaxf(a, c); }
    static __device__ __forceinline__ double fmax_(double a, double c) { return __builtin_fmax(a, c); }

    // ... with the lowest state index that reaches it
    template <int CTRL>
    __device__ __forceinline__ void argmax_step(real& x, int& a) const {
        const real xo = dpp_<CTRL>(x);
        const int ao = dppi_<CTRL>(a);
        const bool take = xo > x || (xo == x && ao < a);
        x = take ? xo : x;
        a = take ? ao : a;
    }
    __device__ __forceinline__ int argmax(const real (&x)[SPL]) const {
        real m = x[0];
        int a = k0;
#pragma unroll
        for (int i = 1; i < SPL; ++i) {
            const bool take = x[i] > m;
            m = take ? x[i] : m;
            a = take ? k0 + i : a;
        }
        if constexpr (R >= 2) argmax_step<QP(1, 0, 3, 2)>(m, a);
        if constexpr (R >= 4) argmax_step<QP(2, 3, 0, 1)>(m, a);
        if constexpr (R >= 8) argmax_step<ROW_HALF_MIRROR>(m, a);
        if constexpr (R >= 16) argmax_step<ROW_MIRROR>(m, a);
        return a;
    }

    // One Hillis-Steele step of a maximum scan over the lanes of the group
    template <bool PREFIX, int N>
    __device__ __forceinline__ real scan_step(real cv) const {
        const real vn = PREFIX ? dpp_<ROW_SHR(N)>(cv) : dpp_<ROW_SHL(N)>(cv);
        const bool ok = PREFIX ? rank >= N : rank + N < R;
        return fmax_(cv, ok ? vn : real(0));
    }
    // in: the lane's own maximum; out: the maximum over the lanes before (PREFIX) / after this one (0 where there is none)
    template <bool PREFIX>
    __device__ __forceinline__ real excl_scan_max(real val) const {
        const real v1 = PREFIX ? dpp_<ROW_SHR(1)>(val) : dpp_<ROW_SHL(1)>(val);
        const bool ok = PREFIX ? rank >= 1 : rank + 1 < R;
        real cv = ok ? v1 : real(0);
        if constexpr (R > 2) cv = scan_step<PREFIX, 1>(cv);
        if constexpr (R > 2) cv = scan_step<PREFIX, 2>(cv);
        if constexpr (R > 4) cv = scan_step<PREFIX, 4>(cv);
        if constexpr (R > 8) cv = scan_step<PREFIX, 8>(cv);
        return cv;
    }

    // One max-product site: y = e_code .* max(v .* pre(u .* x), d .* x, b .* suf(x)), values only
    __device__ __forceinline__ void site(const real (&x)[SPL], const int code, real (&y)[SPL]) const {
        real pre[SPL], suf[SPL];
        real tp = real(0), ts = real(0);
#pragma unroll
        for (int i = 0; i < SPL; ++i) {
            pre[i] = tp;
            tp = fmax_(tp, u[i] * x[i]);
        }
#pragma unroll
        for (int i = SPL - 1; i >= 0; --i) {
            suf[i] = ts;
            ts = fmax_(ts, x[i]);
        }
        if constexpr (R > 1) {
            tp = excl_scan_max<true>(tp);
            ts = excl_scan_max<false>(ts);
        }
        const real* row = etab + code * L::EROW;
#pragma unroll
        for (int i = 0; i < SPL; ++i) {
            const real cp = v[i] * (R > 1 ? fmax_(pre[i], tp) : pre[i]);
            const real cb = b[i] * (R > 1 ? fmax_(suf[i], ts) : suf[i]);
            y[i] = fmax_(fmax_(cp, d[i] * x[i]), cb) * row[L::SLOT(i)];
        }
    }

    // The predecessor of state `cur` (the same in every lane of the group) given x = delta before the site: the lowest
    // index among the largest of  (u_i x_i) v_cur (i < cur),  d_cur x_cur,  b_cur x_i (i > cur)  -- the products the step
    // itself compares (the site's emission multiplies them all alike).  fac: the group's factors in LDS, [b | d | v][K].
    __device__ __forceinline__ int predecessor(const real (&x)[SPL], const int cur, const real* fac) const {
        const real bj = fac[cur], dj = fac[K + cur], vj = fac[2 * K + cur];
        real best = real(-1);
        int arg = k0;
#pragma unroll
        for (int i = 0; i < SPL; ++i) {
            const int k = k0 + i;
            const real lo = (u[i] * x[i]) * vj;
            const real hi = (k == cur ? dj : bj) * x[i];
            const real c = k < cur ? lo : hi;
            const bool take = c > best;
            best = take ? c : best;
            arg = take ? k : arg;
        }
        if constexpr (R >= 2) argmax_step<QP(1, 0, 3, 2)>(best, arg);
        if constexpr (R >= 4) argmax_step<QP(2, 3, 0, 1)>(best, arg);
        if constexpr (R >= 8) argmax_step<ROW_HALF_MIRROR>(best, arg);
        if constexpr (R >= 16) argmax_step<ROW_MIRROR>(best, arg);
        return arg;
    }

    // y *= 2^-ex with ex the exponent of the group's maximum; returns ex, m = that maximum
    __device__ __forceinline__ int rescale(real (&y)[SPL], real& m) const {
        m = gmax(fmax_(fmax_(y[0], y[1]), fmax_(y[2], y[3])));
        const int ex = frexp_exp_(m);
        const real s = ldexp_(real(1), -ex);
#pragma unroll
        for (int i = 0; i < SPL; ++i) y[i] = y[i] * s;
        return ex;
    }
};

template <typename real, int K, int R, int T, int NRM>
__global__ __launch_bounds__(NT_MAX) void vit_fwd_kernel(KArgs A, VArgs D) {
    using L = Lane<real, K, R>;
    using V = typename L::V;
    constexpr int SPL = L::SPL, NP = L::NP;
    static_assert((T == 8 || T == 16) && T % NRM == 0, "a block never straddles an observation word");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x;
    const int64_t nseq = A.B * A.S;
    const int64_t gid = (int64_t)blockIdx.x * (blockDim.x / R) + tid / R;
    const bool active = gid < nseq;
    const int64_t seq = active ? gid : nseq - 1;  // (idle groups repeat the last sequence: same bits, no stores)
    const int rank = tid & (R - 1);
    const int64_t ss = seq / A.B, bb = seq - ss * A.B;  // chunk-major order (see SeqMap)
    const int64_t oseq = bb * A.S + ss;                   // ... the caller's, for the outputs

    L lane;
    V pi[NP];
    lane.load((const real*)A.params + bb * A.pstride_b + ss * A.pstride_s, rank, (real*)smem_raw + (size_t)tid * L::ETAB_STRIDE, pi);
    const real* pfb = prefold_block<real>(A, bb, ss);
    (void)lane.try_fold(pfb != nullptr ? pfb + rank * SPL : nullptr);
    VitLane<real, K, R> vl;
    vl.init(lane, rank);

    const int64_t row = checked_row(A, ss);
    const int64_t n = sweep_len(A, D, row);
    const uint32_t* words = A.packed + row * A.Lw;
    const int nblk = (int)((A.Ltot + T - 1) / T);
    const int64_t ck_step = nseq * K;
    real* ck = (real*)A.ckpt + L::ck_lane(nseq, seq, rank);
    constexpr int RISK_EXP = sizeof(real) == 4 ? RISK_EXP_F32 : RISK_EXP_F64;

    real x[SPL];
#pragma unroll
    for (int i = 0; i < SPL; ++i) x[i] = L::get(pi, i);
    int E = 0;
    bool risky = false;
    int budget = A.loop_budget[0];
    uint32_t wnext = words[0];
    for (int blk = 0; blk < nblk; ++blk) {
        if (__builtin_expect(--budget < 0, 0)) {
            report_overrun(A, OVERRUN_VIT_FWD, seq, blk);
            return;
        }
        const int64_t t0 = (int64_t)blk * T;
        const uint32_t codes = wnext >> (2 * (int)(t0 & 15));
        if (blk + 1 < nblk) wnext = words[(t0 + T) >> 4];  // (requested a block ahead)
        if (active) {
#pragma unroll
            for (int i = 0; i < SPL; ++i) ck_store(&ck[(int64_t)blk * ck_step + L::ck_elem(i, nseq)], x[i]);
        }
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const bool on = t0 + i < n;
            real y[SPL];
            vl.site(x, (codes >> (2 * i)) & 3, y);
            int ex = 0;
            bool r = false;
            if (rescale_after<NRM>(i)) {
                real m;
                ex = vl.rescale(y, m);
                r = !(m > real(0)) || (NRM > 1 && ex < RISK_EXP);
            }
#pragma unroll
            for (int k = 0; k < SPL; ++k) x[k] = on ? y[k] : x[k];
            E += on ? ex : 0;
            risky = risky || (on && r);
        }
    }
    const real m = vl.gmax(vl.fmax_(vl.fmax_(x[0], x[1]), vl.fmax_(x[2], x[3])));
    risky = risky || !(m > real(0));
    if (active && rank == 0) A.ll[oseq] = (double)E * LN2 + log((double)m);
    if (risky && active && A.risk != nullptr) atomicOr(A.risk, FLAG_UNDERFLOW);
}

template <typename real, int K, int R, int T, int NRM>
__global__ __launch_bounds__(NT_MAX) void vit_back_kernel(KArgs A, VArgs D) {
    using L = Lane<real, K, R>;
    using V = typename L::V;
    constexpr int SPL = L::SPL, NP = L::NP;
    static_assert((T == 8 || T == 16) && T % NRM == 0, "a block never straddles an observation word");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x;
    const int64_t nseq = A.B * A.S;
    const int64_t gid = (int64_t)blockIdx.x * (blockDim.x / R) + tid / R;
    const bool active = gid < nseq;
    const int64_t seq = active ? gid : nseq - 1;
    const int rank = tid & (R - 1);
    const int64_t ss = seq / A.B, bb = seq - ss * A.B;
    const int64_t oseq = bb * A.S + ss;

    L lane;
    V pi[NP];
    lane.load((const real*)A.params + bb * A.pstride_b + ss * A.pstride_s, rank, (real*)smem_raw + (size_t)tid * L::ETAB_STRIDE, pi);
    const real* pfb = prefold_block<real>(A, bb, ss);
    (void)lane.try_fold(pfb != nullptr ? pfb + rank * SPL : nullptr);  // the forward kernel's factors, to the bit
    VitLane<real, K, R> vl;
    vl.init(lane, rank);

    const int64_t row = checked_row(A, ss);
    const int64_t n = sweep_len(A, D, row);
    const int64_t Lt = A.Ltot, W = A.W;
    const uint32_t* words = A.packed + row * A.Lw;
    const int nblk = (int)((Lt + T - 1) / T);
    const int64_t ck_step = nseq * K;
    const real* ck = (const real*)A.ckpt + L::ck_lane(nseq, seq, rank);
    uint8_t* prow = D.path + oseq * D.path_stride - W;  // indexed by site
    const bool aligned = (((uintptr_t)prow) & 3) == 0;   // (block starts are multiples of 16)
    // the group's factors b, d, v by state, behind the workgroup's emission tables: the trace reads those of ONE state per site
    real* fac = (real*)smem_raw + (size_t)blockDim.x * L::ETAB_STRIDE + (size_t)(tid - rank) * 3 * SPL;
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        fac[rank * SPL + i] = vl.b[i];
        fac[K + rank * SPL + i] = vl.d[i];
        fac[2 * K + rank * SPL + i] = vl.v[i];
    }
    __syncthreads();

    int cur = 0;  // state of the path at the site being written (the same in every lane of the group)
    int budget = A.loop_budget[1];
    uint32_t wnext = words[((int64_t)(nblk - 1) * T) >> 4];
    real xnext[SPL];
#pragma unroll
    for (int i = 0; i < SPL; ++i) xnext[i] = ck_load(&ck[(int64_t)(nblk - 1) * ck_step + L::ck_elem(i, nseq)]);
    for (int blk = nblk - 1; blk >= 0; --blk) {
        if (__builtin_expect(--budget < 0, 0)) {
            report_overrun(A, OVERRUN_VIT_BACK, seq, blk);
            return;
        }
        const int64_t t0 = (int64_t)blk * T;
        const uint32_t codes = wnext >> (2 * (int)(t0 & 15));
        real x[SPL];
#pragma unroll
        for (int i = 0; i < SPL; ++i) x[i] = xnext[i];
        if (blk > 0) {  // the next block's checkpoint and word, requested a block ahead
            wnext = words[(t0 - T) >> 4];
#pragma unroll
            for (int i = 0; i < SPL; ++i) xnext[i] = ck_load(&ck[(int64_t)(blk - 1) * ck_step + L::ck_elem(i, nseq)]);
        }
        // re-run, keeping xs[i] = delta before site t0 + i in registers
        real xs[T][SPL];
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const bool on = t0 + i < n;
            real y[SPL];
#pragma unroll
            for (int k = 0; k < SPL; ++k) xs[i][k] = x[k];
            vl.site(x, (codes >> (2 * i)) & 3, y);
            if (rescale_after<NRM>(i)) {
                real m;
                (void)vl.rescale(y, m);
            }
#pragma unroll
            for (int k = 0; k < SPL; ++k) x[k] = on ? y[k] : x[k];
        }
        if (blk == nblk - 1) cur = vl.argmax(x);  // the lowest of the best final states
        // trace: the state at site t0 + i, then its predecessor, decided for that one state from xs[i]
        uint32_t out[T / 4];
#pragma unroll
        for (int q = 0; q < T / 4; ++q) out[q] = 0u;
#pragma unroll
        for (int i = T - 1; i >= 0; --i) {
            const bool on = t0 + i < n;
            const uint32_t byte = on ? (uint32_t)cur : 255u;
            out[i >> 2] |= byte << (8 * (i & 3));
            const int pred = vl.predecessor(xs[i], cur, fac);
            cur = on ? pred : cur;
        }
        if (active) {
            if (aligned && t0 >= W && t0 + T <= Lt) {  // four dwords, one per lane (R < 4: several)
#pragma unroll
                for (int q = 0; q < T / 4; ++q)
                    if ((R <= 4 ? (q & (R - 1)) : q) == rank) *(uint32_t*)(prow + t0 + 4 * q) = out[q];
            } else {
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    const int64_t t = t0 + i;
                    if (t >= W && t < Lt && (i & (R - 1)) == rank) prow[t] = (uint8_t)(out[i >> 2] >> (8 * (i & 3)));
                }
            }
        }
    }
}

template <int NRM>
static hipError_t viterbi_n(const KArgs& a, const VArgs& d, int nt, hipStream_t st) {
    using L = Lane<PHK_REAL, PHK_K, SWEEP_R>;
    const int64_t nseq = a.B * a.S;
    const int spb = nt / SWEEP_R;
    const size_t lds = (size_t)L::ETAB_STRIDE * nt * sizeof(PHK_REAL);
    const dim3 grid((unsigned)((nseq + spb - 1) / spb)), block(nt);
    hipLaunchKernelGGL((vit_fwd_kernel<PHK_REAL, PHK_K, SWEEP_R, VIT_T, NRM>), grid, block, lds, st, a, d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t lds_back = lds + (size_t)3 * SWEEP_SPL * nt * sizeof(PHK_REAL);  // + the factors by state (vit_back_kernel: fac)
    hipLaunchKernelGGL((vit_back_kernel<PHK_REAL, PHK_K, SWEEP_R, VIT_T, NRM>), grid, block, lds_back, st, a, d);
    return hipGetLastError();
}

// forward recursion, then the traceback, on one stream; nrm: the handle's rescale interval
hipError_t PHK_CAT(launch_viterbi_, PHK_SUFFIX)(int nrm, const KArgs& a, const VArgs& d, int nt, hipStream_t st) {
    if (nrm == 1) return viterbi_n<1>(a, d, nt, st);
    if (nrm == 2) return viterbi_n<2>(a, d, nt, st);
    if (nrm == 4) return viterbi_n<4>(a, d, nt, st);
    return hipErrorInvalidValue;
}

}  // namespace phk
