// Posterior decoding sweep (psmc -d semantics): per-site hidden-state posteriors gamma_t = alpha_t .* beta_t / sum, reduced
// to means over bins of scored sites.  One translation unit per (real, K), compiled with -DPHK_REAL=float|double -DPHK_K=<K>
// -DPHK_SUFFIX=<tag> (see the Makefile: launch_decode_<real>_<K>.o).  The kernel reuses what the gradient plan's forward
// kernel and beta scan leave behind -- alpha checkpoints every T sites (KArgs::ckpt) and, for the segmented plan, the beta
// seeds at segment starts (KArgs::bseg) -- and replaces the gradient sweep.
//
// Per block of T sites, walked from the right: the forward re-run from the block's checkpoint keeps the T alpha vectors in
// registers (the same Lane::fwd_site steps, folded factors and rescale schedule as the forward kernel), then the beta pass
// runs right to left over them, forming p = alpha .* beta at every site, normalising it across the sequence's R lanes (one
// DPP row reduction) and adding it to the bin's running sum in registers.  A bin is written once, by its owner, when its
// first site has been added: the unit whose site range holds the bin's LAST site.  An owner walks on past its left edge
// until the bin is complete (the checkpoints are there, and its beta is the true beta there), so no unit needs another
// unit's partial sums: no atomics, no finalize kernel, and the same bits whatever order the units run in.
//
// Lanes per sequence: R = K / 4 (4 states per lane) for every (real, K).  That is the layout the segment sweep prefers
// where its block fits in registers, it gives a 16-site block of float64 alphas 128 VGPRs, and it keeps every lane's
// slice of a marginals row one 16- or 32-byte piece.
#include "psmc_kernels.hip"
#include "sweep_common.h"

namespace phk {

// kernel ids of the decode sweep in the overrun record (KArgs::risk[1]; phk_underflow_risk names them)
constexpr int OVERRUN_DECODE_SERIAL = 5;
constexpr int OVERRUN_DECODE_SEG = 6;

// SEG = false: one unit per sequence walks every block.  SEG = true: blockIdx.y picks a unit with the block range of the
// segment sweep (unit 0: every segment up to the one holding the warm-up boundary), seeded from the beta scan's value at its
// right edge.  The seeds left of the warm-up boundary are the plain beta (the scan does not know W), and decoding has no
// warm-up correction, so every unit is independent.
template <typename real, int K, int R, int T, int NRM, bool SEG>
__global__ __launch_bounds__(NT_MAX, (sweep_waves_per_simd<real>(T))) void decode_kernel(KArgs A, DArgs D) {
    using L = Lane<real, K, R>;
    using V = typename L::V;
    constexpr int SPL = L::SPL, NP = L::NP;
    static_assert(T <= 16 && 16 % T == 0 && T % NRM == 0, "block / rescale schedule");
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

    // Sites and bins of this unit.  Everything below is the same for every sequence of the launch (one Ltot, W, bin and
    // unit per launch), so the control flow is wave-uniform and the DPP reductions see every lane.
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

    double f[SPL];
#pragma unroll
    for (int i = 0; i < SPL; ++i) f[i] = D.values != nullptr ? D.values[bb * D.vstride_b + rank * SPL + i] : 0.0;

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

    const uint32_t* words = A.packed + checked_row(A, ss) * A.Lw;
    const int64_t ck_step = nseq * K;
    const real* ck = (const real*)A.ckpt + L::ck_lane(nseq, seq, rank);
    constexpr int RISK_EXP = sizeof(real) == 4 ? RISK_EXP_F32 : RISK_EXP_F64;
    bool risky = false;

    // the bin of the site being processed and the site's offset in it (sites are visited in descending order)
    const int64_t t_start = s_hi - 1;
    int64_t kcur = t_start >= W ? (t_start - W) / bin : -1;
    int64_t rcur = t_start >= W ? (t_start - W) - kcur * bin : 0;
    V acc[NP];
#pragma unroll
    for (int h = 0; h < NP; ++h) acc[h] = splat<real>(real(0));
    int cnt = 0;
    auto flush = [&](const int64_t kb) {
        const real invn = real(1) / real(cnt);
        if (D.marg != nullptr && active) {
            real* dst = (real*)D.marg + (oseq * D.nbin + kb) * K + rank * SPL;
#pragma unroll
            for (int i = 0; i < SPL; ++i) dst[i] = L::get(acc, i) * invn;
        }
        if (D.mean != nullptr) {
            double m = 0.0;
#pragma unroll
            for (int i = 0; i < SPL; ++i) m = fma_(f[i], (double)L::get(acc, i), m);
            m = Group<double, R>().sum(m);
            if (active && rank == 0) ((real*)D.mean)[oseq * D.nbin + kb] = (real)(m / (double)cnt);
        }
#pragma unroll
        for (int h = 0; h < NP; ++h) acc[h] = splat<real>(real(0));
        cnt = 0;
    };

    int budget = SEG ? A.loop_budget[3] : A.loop_budget[1];  // (see KArgs::loop_budget)
    for (int blk = blk_hi - 1; blk >= b_bot; --blk) {
        if (__builtin_expect(--budget < 0, 0)) {
            report_overrun(A, SEG ? OVERRUN_DECODE_SEG : OVERRUN_DECODE_SERIAL, seq, blk);
            return;
        }
        const int64_t t0 = (int64_t)blk * T;
        const int ns = Lt - t0 < T ? (int)(Lt - t0) : T;
        const uint32_t codes = words[t0 >> 4] >> (2 * (int)(t0 & 15));  // (T divides 16: a block never straddles a word)
        // forward re-run from the checkpoint: al[i] = alpha after site t0 + i
        V a[NP], al[T][NP];
#pragma unroll
        for (int h = 0; h < NP; ++h) a[h] = splat<real>(real(0));
#pragma unroll
        for (int i = 0; i < SPL; ++i) L::set(a, i, ck_load(&ck[(int64_t)blk * ck_step + L::ck_elem(i, nseq)]));
#pragma unroll
        for (int i = 0; i < T; ++i) {
            if (i < ns) {
                V e[NP];
                lane.emis((codes >> (2 * i)) & 3, e);
                real sc;
                (void)lane.fwd_site(a, e, sc, rescale_after<NRM>(i));
            }
#pragma unroll
            for (int h = 0; h < NP; ++h) al[i][h] = a[h];
        }
        // beta pass, right to left: gamma of site t0 + i, then beta <- A (e .* beta)
#pragma unroll
        for (int i = T - 1; i >= 0; --i) {
            if (i < ns) {
                const int64_t t = t0 + i;
                if (t <= t_top && t >= t_bot) {
                    V p[NP];
#pragma unroll
                    for (int h = 0; h < NP; ++h) p[h] = al[i][h] * beta[h];
                    real z = lane.total(p);
                    risky = risky || !(z > real(0));
                    // (a model with massless states: beta is scaled by its total over ALL states, and the live states' share of
                    // it can fall below 1 / FLT_MAX -- dead states that explain the hets better, 1e6 per het for a lone live
                    // state 0 -- so that z > 0 and 1 / z = inf: gamma came back as inf and NaN with the flag clear,
                    // tests/test_massless_fuzz.py.  Such a z, subnormal ones included, is scaled up first, with its products.)
                    constexpr real Z_TINY = sizeof(real) == 4 ? real(0x1p-100) : real(0x1p-900);
                    if (__builtin_expect(z < Z_TINY, 0)) {
                        const V up = splat<real>(sizeof(real) == 4 ? real(0x1p64) : real(0x1p200));
#pragma unroll
                        for (int h = 0; h < NP; ++h) p[h] = p[h] * up;
                        z = z * up[0];
                    }
                    const V iz = splat<real>(z > real(0) ? real(1) / z : real(0));
#pragma unroll
                    for (int h = 0; h < NP; ++h) acc[h] = fma2<real>(p[h], iz, acc[h]);
                    ++cnt;
                    if (rcur == 0) flush(kcur);
                }
                if (--rcur < 0) {
                    --kcur;
                    rcur = bin - 1;
                }
                V e[NP];
                lane.emis((codes >> (2 * i)) & 3, e);
                const int ex = lane.bt_site(beta, e, rescale_after<NRM>(T - 1 - i));
                if (NRM > 1 && rescale_after<NRM>(T - 1 - i)) risky = risky || ex < RISK_EXP;
            }
        }
    }
    if (risky && active && A.risk != nullptr) atomicOr(A.risk, FLAG_UNDERFLOW);
}

PHK_SWEEP_LAUNCHER(decode, DArgs, 1)

}  // namespace phk
