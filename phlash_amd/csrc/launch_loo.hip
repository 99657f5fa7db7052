// Leave-one-out predictive sweep: P(o_t = het | o_{-t}) of every scored site and its log score, reduced over bins of scored
// sites.  One translation unit per (real, K), compiled with -DPHK_REAL=float|double -DPHK_K=<K> -DPHK_SUFFIX=<tag> (see the
// Makefile: launch_loo_<real>_<K>.o).
//
// This is trans_kernel (launch_trans.hip) with the cavity term in place of the pair term: the same units, bin ownership, beta
// seeds, forward re-run, rescale schedule and lens select.  With A[i,j] = b_j (i > j), d_j (i = j), u_i v_j (i < j),
//     c_t(k) = (alpha_{t-1} A)(k) beta_t(k) = (d_k alpha_{t-1}(k) + v_k pre_k(u .* alpha_{t-1}) + b_k suf_k(alpha_{t-1})) beta_t(k)
// is everything the row says about z_t except site t's own emission, and
//     n0_t = sum_k c_t(k) row_hom(k)      n1_t = sum_k c_t(k) row_het(k)      phet_t = n1_t / (n0_t + n1_t)
//     score_t = log(n_{o_t} / (n0_t + n1_t)) at an observed site, 0 at a missing one.
// The folded model carries emis0 in b, d, v and keeps 1 and emis1 / emis0 in the table's hom and het rows, so the two products
// are the same numbers in either form and the sweep reads the table rows as they are; alpha_{t-1} and beta_t may sit on
// different power-of-two scales, which the ratio removes.  The site's own emission enters only afterwards, in beta <- A (e .* beta).
//
// Per group three float64 sums per bin (every lane of the group holds the same bits); one writer per bin, no atomics.
#include "psmc_kernels.hip"
#include "sweep_common.h"

namespace phk {

// kernel ids of the predictive sweep in the overrun record (KArgs::risk[1]; phk_underflow_risk names them)
constexpr int OVERRUN_LOO_SERIAL = 12;
constexpr int OVERRUN_LOO_SEG = 13;

__device__ __forceinline__ float loo_log(float x) { return logf(x); }
__device__ __forceinline__ double loo_log(double x) { return log(x); }

// SEG = false: one unit per sequence walks every block.  SEG = true: blockIdx.y picks a unit of the segment layout, seeded from
// the beta scan's value at its right edge (see decode_kernel: the units, their bins and their seeds are the same).
template <typename real, int K, int R, int T, int NRM, bool SEG>
__global__ __launch_bounds__(NT_MAX, (sweep_waves_per_simd<real>(sweep_hold<real, T>()))) void loo_kernel(KArgs A, LArgs D) {
    using L = Lane<real, K, R>;
    using V = typename L::V;
    constexpr int SPL = L::SPL, NP = L::NP;
    static_assert(T <= 16 && 16 % T == 0 && T % NRM == 0, "block / rescale schedule");
    // sites whose alphas are held at once: the whole block, but a quarter of a 16-site float64 block, as trans_kernel.  The
    // cavity term keeps three float64 scalars per group where the pair term keeps three accumulator vectors, but the 16
    // unrolled float64 logarithms take more than that gives back: the compiler's report for K = 16 is 256 VGPRs + 114 AGPR
    // copies at one wave per SIMD for a whole block, 256 VGPRs + 116 bytes of scratch for a half, 186 VGPRs and neither for
    // a quarter.  A piece re-runs the forward steps of the block's sites before it: 24 extra steps per block of 16.
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

    // Sites and bins of this unit: the same for every sequence of the launch, so the control flow is wave-uniform and the
    // DPP reductions see every lane (the row's own length and the site's code enter through selects only).
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

    // the bin of the site being processed and the site's offset in it (sites are visited in descending order)
    const int64_t t_start = s_hi - 1;
    int64_t kcur = t_start >= W ? (t_start - W) / bin : -1;
    int64_t rcur = t_start >= W ? (t_start - W) - kcur * bin : 0;
    double acc_o = 0.0, acc_m = 0.0, acc_l = 0.0;  // bin sums of phet at observed sites, phet at missing sites, the log score
    auto flush = [&](const int64_t kb) {
        if (active && rank == 0) {
            real* dst = (real*)D.track + (oseq * D.nbin + kb) * 3;
            dst[0] = (real)acc_o;
            dst[1] = (real)acc_m;
            dst[2] = (real)acc_l;
        }
        acc_o = acc_m = acc_l = 0.0;
    };

    int budget = SEG ? A.loop_budget[3] : A.loop_budget[1];  // (see KArgs::loop_budget)
    for (int blk = blk_hi - 1; blk >= b_bot; --blk) {
        if (__builtin_expect(--budget < 0, 0)) {
            report_overrun(A, SEG ? OVERRUN_LOO_SEG : OVERRUN_LOO_SERIAL, seq, blk);
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
            // beta pass, right to left: the cavity term of site t0 + i from alpha before it and beta after it, then
            // beta <- A (e .* beta)
#pragma unroll
            for (int j = H - 1; j >= 0; --j) {
                const int i = i0 + j;
                if (i < ns) {
                    const int64_t t = t0 + i;
                    const int code = (codes >> (2 * i)) & 3;
                    if (t <= t_top && t >= t_bot) {
                        const V(&ap)[NP] = j > 0 ? al[j > 0 ? j - 1 : 0] : a0;
                        V pre[NP], suf[NP], e0[NP], e1[NP], m0[NP], m1[NP];
                        lane.scans(ap, pre, suf);
                        lane.emis(0, e0);
                        lane.emis(1, e1);
#pragma unroll
                        for (int h = 0; h < NP; ++h) {
                            const V c = (((lane.d[h] * ap[h]) + (lane.v[h] * pre[h])) + (lane.b[h] * suf[h])) * beta[h];
                            m0[h] = c * e0[h];
                            m1[h] = c * e1[h];
                        }
                        const real n0 = lane.total(m0), n1 = lane.total(m1);
                        const real tot = n0 + n1;
                        const bool own = t < len;
                        const bool ok = own && tot > real(0);
                        risky = risky || (own && !(tot > real(0)));
                        const bool miss = code == 2;
                        const real it = ok ? real(1) / tot : real(0);
                        const real ph = n1 * it;
                        // (the log of 1 where the site adds nothing: no log of a zero that a select would then have to hide; a
                        // share is at most 1, whatever the reciprocal's last bit: a score is never positive)
                        const real share = (code == 1 ? n1 : n0) * it;
                        const real lg = loo_log(ok && !miss && share < real(1) ? share : real(1));
                        acc_o += (double)(miss ? real(0) : ph);
                        acc_m += (double)(miss ? ph : real(0));
                        acc_l += (double)lg;
                        if (rcur == 0) flush(kcur);
                    }
                    if (--rcur < 0) {
                        --kcur;
                        rcur = bin - 1;
                    }
                    V e[NP];
                    lane.emis(code, e);
                    const int ex = lane.bt_site(beta, e, rescale_after<NRM>(H - 1 - j));
                    if (NRM > 1 && rescale_after<NRM>(H - 1 - j)) risky = risky || ex < RISK_EXP;
                }
            }
        }
    }
    if (risky && active && A.risk != nullptr) atomicOr(A.risk, FLAG_UNDERFLOW);
}

PHK_SWEEP_LAUNCHER(loo, LArgs, 1)

}  // namespace phk
