// Tract-posterior sweep: for every bin of scored sites, E[prod_{t in bin} m(z_t) | o] -- for an indicator m of a state set S the
// posterior probability that EVERY site of the bin has its state in S.  One translation unit per (real, K), compiled with
// -DPHK_REAL=float|double -DPHK_K=<K> -DPHK_SUFFIX=<tag> (see the Makefile: launch_tract_<real>_<K>.o).
//
// This is loo_kernel (launch_loo.hip) with a second backward vector q in place of the cavity term: the same units, bin
// ownership, beta seeds, forward re-run, rescale schedule and lens select.  For the bin of sites s .. e,
//     q_e = beta_e,      q_{t-1} = A (m .* e_{o_t} .* q_t)   for t = e, e-1, .., s,
//     tract = sum_i alpha_{s-1}(i) q_{s-1}(i) / sum_i alpha_{s-1}(i) beta_{s-1}(i).
// q runs through beta's own recursion (Lane::scans_adj / Lane::beta_prev) with the site's table row multiplied by m, so the folded
// model needs no unfolding, and it is multiplied by every power of two that rescales beta: the two share a scale, and alpha's
// cancels in the ratio.  Every operation of the q step is the beta step's with one non-negative factor made smaller, and rounding
// is monotone, so q <= beta holds elementwise in the computed numbers too: a tract is never above 1, and a smaller set never has
// the larger tract.  A site at or past its row's own length is stepped with m = 1.
//
// One value per bin and sequence (every lane of the group holds the same bits); one writer per bin, no atomics.
#include "psmc_kernels.hip"
#include "sweep_common.h"

namespace phk {

// kernel ids of the tract sweep in the overrun record (KArgs::risk[1]; phk_underflow_risk names them)
constexpr int OVERRUN_TRACT_SERIAL = 14;
constexpr int OVERRUN_TRACT_SEG = 15;

// (q <- A (em .* q) is tract_step of sweep_common.h: Lane::bt_site's recursion without a rescale of its own -- q takes beta's)

// SEG = false: one unit per sequence walks every block.  SEG = true: blockIdx.y picks a unit of the segment layout, seeded from
// the beta scan's value at its right edge (see decode_kernel: the units, their bins and their seeds are the same).
template <typename real, int K, int R, int T, int NRM, bool SEG>
__global__ __launch_bounds__(NT_MAX, (sweep_waves_per_simd<real>(sweep_hold<real, T>()))) void tract_kernel(KArgs A, QArgs D) {
    using L = Lane<real, K, R>;
    using V = typename L::V;
    constexpr int SPL = L::SPL, NP = L::NP;
    static_assert(T <= 16 && 16 % T == 0 && T % NRM == 0, "block / rescale schedule");
    // sites whose alphas are held at once: the whole block, but a quarter of a 16-site float64 block, as trans_kernel and
    // loo_kernel.  A piece re-runs the forward steps of the block's sites before it: 24 extra steps per block of 16.
    constexpr int H = sweep_hold<real, T>();
    static_assert(T % H == 0 && H % NRM == 0, "pieces / rescale schedule");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x;
    const int64_t nseq = A.B * A.S;
    const int64_t seq_hi = A.seq_end > 0 ? A.seq_end : nseq;
    const int64_t gid = A.seq_begin + (int64_t)blockIdx.x * (blockDim.x / R) + tid / R;
    const bool active = gid < seq_hi;
    const int64_t seq = active ? gid : seq_hi - 1;  // (idle groups repeat the last sequence: same bits, no stores)
    const int rank = tid & (R - 1);
    const int64_t ss = seq / A.B, bb = seq - ss * A.B;  // chunk-major order (see SeqMap)
    const int64_t oseq = bb * A.S + ss;                   // ... the caller's, for the outputs

    // Sites and bins of this unit: the same for every sequence of the launch, so the control flow -- the reset of q at a bin's
    // last site and the store at its first -- is wave-uniform and the DPP reductions see every lane (the row's own length and
    // the site's code enter through selects only).
    const int64_t Lt = A.Ltot, W = A.W, bin = D.bin;
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
    // owned bins [kmin, kmax]: those whose last site lies in [s_lo, s_hi)
    const int64_t kmax = s_hi >= Lt ? D.nbin - 1 : (s_hi > W ? (s_hi - W) / bin - 1 : -1);
    const int64_t kmin = (blk_lo == 0 || s_lo <= W) ? 0 : (s_lo - W) / bin;
    if (kmin > kmax || blk_hi <= blk_lo) return;
    const int64_t t_top = (W + (kmax + 1) * bin < Lt ? W + (kmax + 1) * bin : Lt) - 1;  // last owned site
    const int64_t t_bot = W + kmin * bin;                                               // first owned site
    const int b_bot = (int)(t_bot / T);

    L lane;
    V pi[NP];
    lane.load((const real*)A.params + bb * A.pstride_b + ss * A.pstride_s, rank, (real*)smem_raw + (size_t)tid * L::ETAB_STRIDE, pi);
    const real* pfb = prefold_block<real>(A, bb, ss);
    (void)lane.try_fold(pfb != nullptr ? pfb + rank * SPL : nullptr);  // the forward kernel's factors, to the bit

    // the particle's weight row, rounded to the kernel's type, once per group
    V m[NP];
    {
        const double* src = D.weights + bb * D.wstride_b + rank * SPL;
#pragma unroll
        for (int h = 0; h < NP; ++h) m[h] = splat<real>(real(0));
#pragma unroll
        for (int i = 0; i < SPL; ++i) L::set(m, i, (real)src[i]);
    }

    // beta at the unit's right edge: 1 at the row's end, else the beta scan's seed (its exponent does not matter here)
    V beta[NP], q[NP];
#pragma unroll
    for (int h = 0; h < NP; ++h) beta[h] = q[h] = splat<real>(real(0));
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

    // the bin of the site being processed and the site's offset in it (sites are visited in descending order)
    const int64_t t_start = s_hi - 1;
    int64_t kcur = t_start >= W ? (t_start - W) / bin : -1;
    int64_t rcur = t_start >= W ? (t_start - W) - kcur * bin : 0;

    int budget = SEG ? A.loop_budget[3] : A.loop_budget[1];  // (see KArgs::loop_budget)
    for (int blk = blk_hi - 1; blk >= b_bot; --blk) {
        if (__builtin_expect(--budget < 0, 0)) {
            report_overrun(A, SEG ? OVERRUN_TRACT_SEG : OVERRUN_TRACT_SERIAL, seq, blk);
            return;
        }
        const int64_t t0 = (int64_t)blk * T;
        const int ns = Lt - t0 < T ? (int)(Lt - t0) : T;
        const uint32_t codes = words[t0 >> 4] >> (2 * (int)(t0 & 15));  // (T divides 16: a block never straddles a word)
        // The block in pieces of H sites, from the right.  Per piece: the forward re-run from the checkpoint up to the piece
        // (nothing kept), a0 = alpha before the piece's first site, al[j] = alpha after its site j; then the beta pass over it.
        V c0[NP];
#pragma unroll
        for (int h = 0; h < NP; ++h) c0[h] = splat<real>(real(0));
#pragma unroll
        for (int i = 0; i < SPL; ++i) L::set(c0, i, ck_load(&ck[(int64_t)blk * ck_step + L::ck_elem(i, nseq)]));
        // (a loop that stays a loop, as in trans_kernel.  H is a multiple of NRM, so the rescale schedule of site i0 + j is j's.)
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
            // beta pass, right to left.  Per site: q = beta at the last site of an owned bin; beta <- A (e .* beta) and
            // q <- A (m .* e .* q), q scaled by beta's power of two; at the bin's first site the two sums against the alpha
            // before it, and the store.
#pragma unroll
            for (int j = H - 1; j >= 0; --j) {
                const int i = i0 + j;
                if (i < ns) {
                    const int64_t t = t0 + i;
                    const int code = (codes >> (2 * i)) & 3;
                    const bool owned = t <= t_top && t >= t_bot;
                    if (owned && (rcur == bin - 1 || t == Lt - 1)) {
#pragma unroll
                        for (int h = 0; h < NP; ++h) q[h] = beta[h];
                    }
                    V e[NP], em[NP];
                    lane.emis(code, e);
                    const bool own = t < len;
#pragma unroll
                    for (int h = 0; h < NP; ++h) em[h] = own ? e[h] * m[h] : e[h];
                    tract_step(lane, q, em);
                    const bool SC = rescale_after<NRM>(H - 1 - j);
                    const int ex = lane.bt_site(beta, e, SC);
                    if (SC) {
                        const V s2 = splat<real>(ldexp_(real(1), -ex));  // exact power of two: q keeps beta's scale
#pragma unroll
                        for (int h = 0; h < NP; ++h) q[h] = q[h] * s2;
                        if (NRM > 1) risky = risky || ex < RISK_EXP;
                    }
                    if (owned && rcur == 0) {
                        const V(&ap)[NP] = j > 0 ? al[j > 0 ? j - 1 : 0] : a0;
                        V xq[NP], xb[NP];
#pragma unroll
                        for (int h = 0; h < NP; ++h) {
                            xq[h] = ap[h] * q[h];
                            xb[h] = ap[h] * beta[h];
                        }
                        const real num = lane.total(xq), den = lane.total(xb);
                        // (t is the bin's first site: the bin has a site of the row's own exactly when t has)
                        const bool ok = own && den > real(0);
                        risky = risky || (own && !(den > real(0)));
                        const real val = ok ? num / den : real(0);
                        if (active && rank == 0) ((real*)D.tract)[oseq * D.nbin + kcur] = val;
                    }
                    if (--rcur < 0) {
                        --kcur;
                        rcur = bin - 1;
                    }
                }
            }
        }
    }
    if (risky && active && A.risk != nullptr) atomicOr(A.risk, FLAG_UNDERFLOW);
}

PHK_SWEEP_LAUNCHER(tract, QArgs, 1)

}  // namespace phk
