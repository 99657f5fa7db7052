// Pair-count sweep: C(i, j) = sum over a row's own scored sites of the pair posterior xi_t(i, j) = P(z_{t-1} = i, z_t = j | o),
// the expected number of moves from TMRCA state i to state j (the Baum-Welch transition statistic), K x K per sequence.  One
// translation unit per (real, K), compiled with -DPHK_REAL=float|double -DPHK_K=<K> -DPHK_SUFFIX=<tag> (see the Makefile:
// launch_pairs_<real>_<K>.o).
//
// This is trans_kernel (launch_trans.hip) with another accumulator: the same units, forward re-run from the checkpoint, rescale
// schedule, folded factors, lens by select, loop budget and underflow flag.  With A[i,j] = b_j (i > j), d_j (i = j), u_i v_j
// (i < j) and w = e_{o_t} .* beta_t,
//     xi_t(i, j) = alpha_{t-1}(i) A[i, j] w_t(j) / Z_t,
// and A belongs to the model, not to the site: the sweep sums the raw outer products
//     G(i, j) = sum_t alpha_{t-1}(i) w_t(j) / Z_t
// and pairs_finalize_kernel multiplies by A[i, j] once.  Z_t is the sum of xi_t over all (i, j), from the transition sweep's three
// structured products in O(K).  In the folded model column j of A carries the hom emission and w is divided by it, so the
// finalize kernel takes the factors as the sweep held them (see launch_trans.hip: both forms give the same numbers).
//
// K = 16, float32 (pairs_mfma): the outer product of a site is 16 v_mfma_f32_4x4x1_16b_f32, the 16-block form with one block
// per sequence.  The sweep's layout is 4 lanes per sequence and 4 states per lane: lane 4q + r holds states 4r + m (slot m) of
// sequence q of the wave, which is element r of block q of the instruction's A and B operands as it stands.  Instruction
// (m, n) takes slot m of alpha_{t-1} / Z_t and slot n of w; register rho of lane 4q + c of its result is row rho, column c of
// block q, so tile (m, n) holds G(4 rho + m, 4 c + n) of sequence q.  16 independent accumulator tiles, 64 registers.
// Every other (real, K): a lane accumulates, for its own 4 columns, a tile of RT origin rows whose alpha_{t-1} / Z_t is read
// from the lane that holds it; one launch per row tile (ceil(K / RT) launches re-run the sweep: this path is only correct).
//
// float32 accumulators are added into the unit's float64 partial and zeroed every PAIRS_FLUSH_SITES sites; float64 kernels
// accumulate in float64 throughout.  A unit writes only its own partial [unit, sequence, K, K] (zeroed by the launcher: a unit
// without a scored site leaves zeros); the finalize kernel sums the units in index order: one writer, no atomics, the same bits
// for any slab.
#include "psmc_kernels.hip"
#include "sweep_common.h"

#ifndef PHK_PAIRS_MFMA
#define PHK_PAIRS_MFMA 1  // A/B (scripts/pair_counts_timing.py): 0 = K = 16 float32 runs the plain template like every other (real, K)
#endif

namespace phk {

// kernel ids of the pair-count sweep in the overrun record (KArgs::risk[1]; phk_underflow_risk names them)
constexpr int OVERRUN_PAIRS_SERIAL = 18;
constexpr int OVERRUN_PAIRS_SEG = 19;
// float32 accumulators go into the float64 partial this often: 64 * 2^-24 = 3.8e-6 is the worst rounding a float32 sum of 64
// terms adds to an entry, relative to the entry ("Pair counts")
#ifndef PHK_PAIRS_FLUSH_SITES
#define PHK_PAIRS_FLUSH_SITES 64  // (diagnostic builds: a multiple of 16 beyond the row length carries the float32 sums over the whole unit)
#endif
constexpr int PAIRS_FLUSH_SITES = PHK_PAIRS_FLUSH_SITES;

typedef float pairs_f4 __attribute__((ext_vector_type(4)));

// sites whose alphas are held at once (the mechanism of trans_hold): float32 a 16-site block in two pieces of 8, float64 every
// block in pieces of 4 -- the accumulator tile takes the registers the held alphas give up
template <typename real, int T>
constexpr int pairs_hold() { return sizeof(real) == 8 ? 4 : (T == 16 ? 8 : T); }
template <typename real, int K>
constexpr bool pairs_mfma() { return PHK_PAIRS_MFMA != 0 && sizeof(real) == 4 && K == 16; }
// origin rows per launch of the plain template: what leaves the object without scratch at two waves per SIMD
template <typename real, int K>
constexpr int pairs_rt() { return sizeof(real) == 8 ? 4 : (K <= 16 ? K : 8); }

// lane `src` of this lane's group of R
template <int R>
__device__ __forceinline__ float pairs_bcast(float x, int src) { return R > 1 ? __shfl(x, src, R) : x; }
template <int R>
__device__ __forceinline__ double pairs_bcast(double x, int src) { return R > 1 ? __shfl(x, src, R) : x; }

// SEG = false: one unit per sequence walks every block.  SEG = true: blockIdx.y picks a unit of the segment layout, seeded from
// the beta scan's value at its right edge (see decode_kernel: the units and their seeds are the same; a unit owns the scored
// sites of its own blocks).
template <typename real, int K, int R, int T, int NRM, bool SEG>
__global__ __launch_bounds__(NT_MAX, 2) void pairs_kernel(KArgs A, PArgs D) {
    using L = Lane<real, K, R>;
    using V = typename L::V;
    constexpr int SPL = L::SPL, NP = L::NP;
    static_assert(SPL == 4 && T <= 16 && 16 % T == 0 && T % NRM == 0, "layout / block / rescale schedule");
    constexpr int H = pairs_hold<real, T>();
    static_assert(T % H == 0 && H % NRM == 0, "pieces / rescale schedule");
    constexpr bool MFMA = pairs_mfma<real, K>();
    constexpr int RT = MFMA ? 4 : pairs_rt<real, K>();  // (matrix path: RT sizes nothing but the unused plain tile)
    static_assert(RT % 4 == 0 && K % RT == 0, "row tiles of whole lanes");
    constexpr bool F32ACC = sizeof(real) == 4;
    static_assert(PAIRS_FLUSH_SITES % T == 0, "the partial is updated between blocks");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x;
    const int64_t nseq = A.B * A.S;
    const int64_t seq_hi = A.seq_end > 0 ? A.seq_end : nseq;
    const int64_t gid = A.seq_begin + (int64_t)blockIdx.x * (blockDim.x / R) + tid / R;
    const bool active = gid < seq_hi;
    const int64_t seq = active ? gid : seq_hi - 1;  // (idle groups repeat the last sequence: same bits, no stores)
    const int rank = tid & (R - 1);
    const int64_t ss = seq / A.B, bb = seq - ss * A.B;  // chunk-major order (see SeqMap)

    // Sites of this unit: the same for every sequence of the launch, so the control flow is wave-uniform, the DPP reductions
    // and the matrix instruction see every lane (the row's own length enters through selects only).
    const int64_t Lt = A.Ltot, W = A.W;
    const int nblk = (int)((Lt + T - 1) / T);
    int blk_lo = 0, blk_hi = nblk;
    if constexpr (SEG) {
        const int G = A.seg_blocks;
        const int segW = A.W > 0 ? (int)((A.W - 1) / T) / G : 0;  // segment holding the warm-up boundary
        const int seg = segW + (int)blockIdx.y;
        blk_lo = blockIdx.y == 0 ? 0 : seg * G;
        blk_hi = (seg + 1) * G < nblk ? (seg + 1) * G : nblk;
    }
    const int64_t s_lo = (int64_t)blk_lo * T, s_hi = (int64_t)blk_hi * T < Lt ? (int64_t)blk_hi * T : Lt;
    const int64_t t_top = s_hi - 1;             // last owned site
    const int64_t t_bot = s_lo > W ? s_lo : W;  // first owned site
    if (t_top < t_bot || blk_hi <= blk_lo) return;
    const int b_bot = (int)(t_bot / T);

    L lane;
    V pi[NP];
    lane.load((const real*)A.params + bb * A.pstride_b + ss * A.pstride_s, rank, (real*)smem_raw + (size_t)tid * L::ETAB_STRIDE, pi);
    const real* pfb = prefold_block<real>(A, bb, ss);
    (void)lane.try_fold(pfb != nullptr ? pfb + rank * SPL : nullptr);  // the forward kernel's factors, to the bit

    // beta at the unit's right edge: 1 at the row's end, else the beta scan's seed (its exponent does not matter here)
    V beta[NP];
#pragma unroll
    for (int h = 0; h < NP; ++h) beta[h] = splat<real>(real(0));
    if (SEG && blk_hi < nblk) {
        const int64_t sb = blk_hi / A.seg_blocks;
        const real* src = (const real*)A.bseg + (sb * nseq + seq) * K + rank * SPL;
#pragma unroll
        for (int i = 0; i < SPL; ++i) L::set(beta, i, src[i]);
    } else {
#pragma unroll
        for (int i = 0; i < SPL; ++i) L::set(beta, i, real(1));
    }

    const int64_t row = checked_row(A, ss);
    const uint32_t* words = A.packed + row * A.Lw;
    const int64_t len = sweep_len(A, D, row);
    const int64_t ck_step = nseq * K;
    const real* ck = (const real*)A.ckpt + L::ck_lane(nseq, seq, rank);
    constexpr int RISK_EXP = sizeof(real) == 4 ? RISK_EXP_F32 : RISK_EXP_F64;
    bool risky = false;

    // this unit's partial of this sequence: [K, K] float64, origin state first
    const int64_t nloc = seq_hi - A.seq_begin;
    double* const part = D.part + (((int64_t)(SEG ? blockIdx.y : 0) * nloc + (seq - A.seq_begin)) * K + 0) * K + rank * SPL;
    pairs_f4 tile[MFMA ? 4 : 1][MFMA ? 4 : 1];  // matrix path: tile[m][n][rho] = G(4 rho + m, 4 rank + n)
    real acc[MFMA ? 1 : RT][SPL];               // plain path: acc[r][n] = G(row0 + r, 4 rank + n)
#pragma unroll
    for (int m = 0; m < (MFMA ? 4 : 1); ++m)
#pragma unroll
        for (int n = 0; n < (MFMA ? 4 : 1); ++n) tile[m][n] = pairs_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < (MFMA ? 1 : RT); ++r)
#pragma unroll
        for (int n = 0; n < SPL; ++n) acc[r][n] = real(0);
    auto flush = [&]() {
        if constexpr (MFMA) {
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int rho = 0; rho < 4; ++rho) {
                    double* dst = part + (4 * rho + m) * K;
                    if (active) {
#pragma unroll
                        for (int n = 0; n < 4; ++n) dst[n] += (double)tile[m][n][rho];
                    }
                }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) tile[m][n] = pairs_f4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                double* dst = part + (D.row0 + r) * K;
                if (active) {
#pragma unroll
                    for (int n = 0; n < SPL; ++n) dst[n] += (double)acc[r][n];
                }
#pragma unroll
                for (int n = 0; n < SPL; ++n) acc[r][n] = real(0);
            }
        }
    };
    const int src0 = D.row0 / SPL;  // plain path: the lane of the group that holds origin state row0

    int since = 0;  // sites walked since the float32 accumulators last went into the partial
    int budget = SEG ? A.loop_budget[3] : A.loop_budget[1];  // (see KArgs::loop_budget)
    for (int blk = blk_hi - 1; blk >= b_bot; --blk) {
        if (__builtin_expect(--budget < 0, 0)) {
            report_overrun(A, SEG ? OVERRUN_PAIRS_SEG : OVERRUN_PAIRS_SERIAL, seq, blk);
            return;
        }
        const int64_t t0 = (int64_t)blk * T;
        const int ns = Lt - t0 < T ? (int)(Lt - t0) : T;
        const uint32_t codes = words[t0 >> 4] >> (2 * (int)(t0 & 15));  // (T divides 16: a block never straddles a word)
        // The block in pieces of H sites, from the right, exactly as trans_kernel walks it.
        V c0[NP];
#pragma unroll
        for (int h = 0; h < NP; ++h) c0[h] = splat<real>(real(0));
#pragma unroll
        for (int i = 0; i < SPL; ++i) L::set(c0, i, ck_load(&ck[(int64_t)blk * ck_step + L::ck_elem(i, nseq)]));
#pragma unroll 1
        for (int i0 = T - H; i0 >= 0; i0 -= H) {
            if (i0 >= ns) continue;
            V a[NP], a0[NP], al[H][NP];
#pragma unroll
            for (int h = 0; h < NP; ++h) a[h] = c0[h];
#pragma unroll 1
            for (int p0 = 0; p0 < i0; p0 += H) {
#pragma unroll
                for (int j = 0; j < H; ++j) {
                    V e[NP];
                    lane.emis((codes >> (2 * (p0 + j))) & 3, e);
                    real sc;
                    (void)lane.fwd_site(a, e, sc, rescale_after<NRM>(j));
                }
            }
#pragma unroll
            for (int h = 0; h < NP; ++h) a0[h] = a[h];
#pragma unroll
            for (int j = 0; j < H; ++j) {
                const int i = i0 + j;
                if (i < ns) {
                    V e[NP];
                    lane.emis((codes >> (2 * i)) & 3, e);
                    real sc;
                    (void)lane.fwd_site(a, e, sc, rescale_after<NRM>(j));
                }
#pragma unroll
                for (int h = 0; h < NP; ++h) al[j][h] = a[h];
            }
            // beta pass, right to left: the outer product of site t0 + i from alpha before it and w = e .* beta, then beta <- A w
#pragma unroll
            for (int j = H - 1; j >= 0; --j) {
                const int i = i0 + j;
                if (i < ns) {
                    const int64_t t = t0 + i;
                    V e[NP];
                    lane.emis((codes >> (2 * i)) & 3, e);
                    if (t <= t_top && t >= t_bot) {
                        const V(&ap)[NP] = j > 0 ? al[j > 0 ? j - 1 : 0] : a0;
                        V pre[NP], suf[NP], w[NP], sum[NP];
                        lane.scans(ap, pre, suf);
#pragma unroll
                        for (int h = 0; h < NP; ++h) {
                            w[h] = beta[h] * e[h];
                            const V ps = (lane.d[h] * ap[h]) * w[h];
                            const V pu = (lane.v[h] * pre[h]) * w[h];
                            const V pd = (lane.b[h] * suf[h]) * w[h];
                            sum[h] = (ps + pu) + pd;
                        }
                        const real z = lane.total(sum);
                        const bool own = t < len;
                        risky = risky || (own && !(z > real(0)));
                        const V iz = splat<real>(own && z > real(0) ? real(1) / z : real(0));
                        V az[NP];  // alpha_{t-1} / Z_t: 0 for a site past the row's own length
#pragma unroll
                        for (int h = 0; h < NP; ++h) az[h] = ap[h] * iz;
                        if constexpr (MFMA) {
#pragma unroll
                            for (int m = 0; m < 4; ++m)
#pragma unroll
                                for (int n = 0; n < 4; ++n)
                                    tile[m][n] = __builtin_amdgcn_mfma_f32_4x4x1f32((float)L::get(az, m), (float)L::get(w, n), tile[m][n], 0, 0, 0);
                        } else {
#pragma unroll
                            for (int r = 0; r < RT; ++r) {
                                const real ar = pairs_bcast<R>(L::get(az, r % SPL), src0 + r / SPL);
#pragma unroll
                                for (int n = 0; n < SPL; ++n) acc[r][n] = fma_(ar, L::get(w, n), acc[r][n]);
                            }
                        }
                    }
                    const int ex = lane.bt_site(beta, e, rescale_after<NRM>(H - 1 - j));
                    if (NRM > 1 && rescale_after<NRM>(H - 1 - j)) risky = risky || ex < RISK_EXP;
                }
            }
        }
        if constexpr (F32ACC) {
            since += T;
            if (since >= PAIRS_FLUSH_SITES) {
                flush();
                since = 0;
            }
        }
    }
    flush();
    if (risky && active && A.risk != nullptr) atomicOr(A.risk, FLAG_UNDERFLOW);
}

// counts[b, s, i, j] = A[i, j] * (sum over the units, in index order, of their partials), in float64.  A from the parameter
// block with the factors of column j as the sweep held them: folded where the sequence folds (Lane::try_fold), the pre-folded
// block where the call brought one.
template <typename real, int K>
__global__ void pairs_finalize_kernel(KArgs A, PArgs D, int units) {
    const int64_t nloc = A.B * A.S;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nloc * K * K) return;
    const int64_t seq = idx / (K * K);
    const int ij = (int)(idx - seq * (K * K)), i = ij / K, j = ij - i * K;
    const int64_t ss = seq / A.B, bb = seq - ss * A.B;  // chunk-major order (see SeqMap)
    const int64_t oseq = bb * A.S + ss;                   // ... the caller's, for the output
    const real* p = (const real*)A.params + bb * A.pstride_b + ss * A.pstride_s;
    bool fold = (sizeof(real) == 4 || PHK_FOLD_F64 != 0) && PHK_FOLD != 0;
    for (int k = 0; k < K; ++k) fold = fold && p[4 * K + k] > (real)RATIO_MIN_EMIS0;  // (Lane::emissions_foldable)
    const real* pf = prefold_block<real>(A, bb, ss);
    real bj = p[0 * K + j], dj = p[1 * K + j], vj = p[3 * K + j];
    if (fold) {
        if (pf != nullptr) {
            bj = pf[0 * K + j];
            dj = pf[1 * K + j];
            vj = pf[2 * K + j];
        } else {
            const real e0 = p[4 * K + j];
            bj = bj * e0;
            dj = dj * e0;
            vj = vj * e0;
        }
    }
    const double aij = i > j ? (double)bj : (i == j ? (double)dj : (double)p[2 * K + i] * (double)vj);
    double s = 0.0;
    for (int u = 0; u < units; ++u) s += D.part[((int64_t)u * nloc + seq) * (K * K) + ij];
    D.counts[oseq * (K * K) + ij] = s * aij;
}

template <int T, int NRM>
static hipError_t pairs_tn(const KArgs& a, const PArgs& d, int units, int nt, hipStream_t st) {
    using L = Lane<PHK_REAL, PHK_K, SWEEP_R>;
    const int64_t nseq = (a.seq_end > 0 ? a.seq_end : a.B * a.S) - a.seq_begin;
    const int spb = nt / SWEEP_R;
    const size_t lds = (size_t)L::ETAB_STRIDE * nt * sizeof(PHK_REAL);
    const dim3 grid((unsigned)((nseq + spb - 1) / spb), (unsigned)(units <= 0 ? 1 : units)), block(nt);
    constexpr int step = pairs_mfma<PHK_REAL, PHK_K>() ? PHK_K : pairs_rt<PHK_REAL, PHK_K>();
    for (int row0 = 0; row0 < PHK_K; row0 += step) {  // one launch per row tile
        PArgs dd = d;
        dd.row0 = row0;
        if (units <= 0) hipLaunchKernelGGL((pairs_kernel<PHK_REAL, PHK_K, SWEEP_R, T, NRM, false>), grid, block, lds, st, a, dd);
        else hipLaunchKernelGGL((pairs_kernel<PHK_REAL, PHK_K, SWEEP_R, T, NRM, true>), grid, block, lds, st, a, dd);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

PHK_SWEEP_DISPATCH(pairs, PArgs)

// T: the checkpoint spacing of the forward kernel that ran before; nrm: its rescale interval; units <= 0: one serial sweep per
// sequence, else the segment layout of the segmented plan (KArgs::seg_blocks, bseg).  Zeroes the partials, sweeps, finalizes.
hipError_t PHK_CAT(launch_pairs_, PHK_SUFFIX)(int T, int nrm, const KArgs& a, const PArgs& d, int units, int nt, hipStream_t st) {
    if (d.counts == nullptr) return hipSuccess;  // (W = L: no scored site, nothing to write)
    const int64_t nseq = a.B * a.S;
    const int nu = units > 0 ? units : 1;
    hipError_t e = hipMemsetAsync(d.part, 0, (size_t)nu * (size_t)nseq * PHK_K * PHK_K * sizeof(double), st);
    if (e != hipSuccess) return e;
    e = pairs_any(T, nrm, a, d, units, nt, st);
    if (e != hipSuccess) return e;
    const int64_t n = nseq * PHK_K * PHK_K;
    hipLaunchKernelGGL((pairs_finalize_kernel<PHK_REAL, PHK_K>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, d, nu);
    return hipGetLastError();
}

}  // namespace phk
