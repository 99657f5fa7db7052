// Transition-posterior sweep: the pair posterior xi_t(i, j) = P(z_{t-1} = i, z_t = j | o) of every scored site, split by how
// the state at the site was reached -- stay (i = j), up (i < j: a move to an older state), down (i > j) -- and reduced over bins
// of scored sites.  One translation unit per (real, K), compiled with -DPHK_REAL=float|double -DPHK_K=<K> -DPHK_SUFFIX=<tag>
// (see the Makefile: launch_trans_<real>_<K>.o).
//
// This is decode_kernel (launch_decode.hip) with the pair term in place of alpha .* beta: the same units, bin ownership, beta
// seeds, forward re-run and rescale schedule.  With A[i,j] = b_j (i > j), d_j (i = j), u_i v_j (i < j) and w = e_{o_t} .* beta_t,
//     stay_t(k) = alpha_{t-1}(k) d_k w(k)         up_t(k) = pre_k(u .* alpha_{t-1}) v_k w(k)         down_t(k) = suf_k(alpha_{t-1}) b_k w(k)
// each over Z_t, the sum of all three over k: the exclusive prefix and suffix are the two scans of Lane::fwd_site, taken of the
// alpha BEFORE the site (al[i - 1]; the block's checkpoint for its first site), so a site costs O(K), not a K x K tile.  The
// folded model multiplies column j of A by a factor that the table row of the site divides out again, so the three products are
// the same numbers in either form; alpha_{t-1} and beta_t may sit on different power-of-two scales, which Z_t removes.
//
// Rows of their own length (TArgs::lens): every sequence of a launch walks the same blocks; a site at or past the row's own
// length is added with weight 0 (a select, not a divergent bound) and is not counted in the bin's mean.
#include "psmc_kernels.hip"
#include "sweep_common.h"

namespace phk {

// kernel ids of the transition sweep in the overrun record (KArgs::risk[1]; phk_underflow_risk names them)
constexpr int OVERRUN_TRANS_SERIAL = 10;
constexpr int OVERRUN_TRANS_SEG = 11;

// SEG = false: one unit per sequence walks every block.  SEG = true: blockIdx.y picks a unit of the segment layout, seeded from
// the beta scan's value at its right edge (see decode_kernel: the units, their bins and their seeds are the same).
template <typename real, int K, int R, int T, int NRM, bool SEG>
__global__ __launch_bounds__(NT_MAX, (sweep_waves_per_simd<real>(sweep_hold<real, T>()))) void trans_kernel(KArgs A, TArgs D) {
    using L = Lane<real, K, R>;
    using V = typename L::V;
    constexpr int SPL = L::SPL, NP = L::NP;
    static_assert(T <= 16 && 16 % T == 0 && T % NRM == 0, "block / rescale schedule");
    // sites whose alphas are held at once: the whole block, but a quarter of a 16-site float64 block.  Three accumulator sets
    // and the pair term's scans beside 16 float64 alphas do not fit 256 VGPRs, and neither does a half: an 8-site float64
    // block takes 240 as it is, and the checkpoint kept for the second piece tips it into scratch.  A piece re-runs the
    // forward steps of the block's sites before it: 24 extra steps per block of 16.
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
    // DPP reductions see every lane (the row's own length enters through selects only).
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
    V acc_s[NP], acc_u[NP], acc_d[NP];  // bin sums of stay, up, down
#pragma unroll
    for (int h = 0; h < NP; ++h) acc_s[h] = acc_u[h] = acc_d[h] = splat<real>(real(0));
    auto flush = [&](const int64_t kb) {
        // the row's own sites in the bin: [W + kb bin, min(W + (kb + 1) bin, len))
        const int64_t lo = W + kb * bin;
        const int64_t hi = lo + bin < len ? lo + bin : len;
        const int64_t own = hi > lo ? hi - lo : 0;
        const real invn = own > 0 ? real(1) / real(own) : real(0);
        if (D.arr != nullptr && active) {
            real* dst = (real*)D.arr + (oseq * D.nbin + kb) * 3 * K + rank * SPL;
#pragma unroll
            for (int i = 0; i < SPL; ++i) {
                dst[i] = L::get(acc_s, i) * invn;
                dst[K + i] = L::get(acc_u, i) * invn;
                dst[2 * K + i] = L::get(acc_d, i) * invn;
            }
        }
        if (D.chg != nullptr) {
            double up = 0.0, dn = 0.0;
#pragma unroll
            for (int i = 0; i < SPL; ++i) {
                up += (double)L::get(acc_u, i);
                dn += (double)L::get(acc_d, i);
            }
            up = Group<double, R>().sum(up);
            dn = Group<double, R>().sum(dn);
            if (active && rank == 0) {
                real* dst = (real*)D.chg + (oseq * D.nbin + kb) * 2;
                dst[0] = (real)up;
                dst[1] = (real)dn;
            }
        }
#pragma unroll
        for (int h = 0; h < NP; ++h) acc_s[h] = acc_u[h] = acc_d[h] = splat<real>(real(0));
    };

    int budget = SEG ? A.loop_budget[3] : A.loop_budget[1];  // (see KArgs::loop_budget)
    for (int blk = blk_hi - 1; blk >= b_bot; --blk) {
        if (__builtin_expect(--budget < 0, 0)) {
            report_overrun(A, SEG ? OVERRUN_TRANS_SEG : OVERRUN_TRANS_SERIAL, seq, blk);
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
        // (a loop that stays a loop: unrolled, the scheduler runs the next piece's forward steps beside this piece's beta
        // pass and both pieces' alphas are live at once.  H is a multiple of NRM, so the rescale schedule of site i0 + j is j's.)
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
            // beta pass, right to left: the pair term of site t0 + i from alpha before it and w = e .* beta, then beta <- A w
#pragma unroll
            for (int j = H - 1; j >= 0; --j) {
                const int i = i0 + j;
                if (i < ns) {
                    const int64_t t = t0 + i;
                    V e[NP];
                    lane.emis((codes >> (2 * i)) & 3, e);
                    if (t <= t_top && t >= t_bot) {
                        const V(&ap)[NP] = j > 0 ? al[j > 0 ? j - 1 : 0] : a0;
                        V pre[NP], suf[NP], ps[NP], pu[NP], pd[NP], sum[NP];
                        lane.scans(ap, pre, suf);
#pragma unroll
                        for (int h = 0; h < NP; ++h) {
                            const V w = beta[h] * e[h];
                            ps[h] = (lane.d[h] * ap[h]) * w;
                            pu[h] = (lane.v[h] * pre[h]) * w;
                            pd[h] = (lane.b[h] * suf[h]) * w;
                            sum[h] = (ps[h] + pu[h]) + pd[h];
                        }
                        const real z = lane.total(sum);
                        const bool own = t < len;
                        risky = risky || (own && !(z > real(0)));
                        const V iz = splat<real>(own && z > real(0) ? real(1) / z : real(0));
#pragma unroll
                        for (int h = 0; h < NP; ++h) {
                            acc_s[h] = fma2<real>(ps[h], iz, acc_s[h]);
                            acc_u[h] = fma2<real>(pu[h], iz, acc_u[h]);
                            acc_d[h] = fma2<real>(pd[h], iz, acc_d[h]);
                        }
                        if (rcur == 0) flush(kcur);
                    }
                    if (--rcur < 0) {
                        --kcur;
                        rcur = bin - 1;
                    }
                    const int ex = lane.bt_site(beta, e, rescale_after<NRM>(H - 1 - j));
                    if (NRM > 1 && rescale_after<NRM>(H - 1 - j)) risky = risky || ex < RISK_EXP;
                }
            }
        }
    }
    if (risky && active && A.risk != nullptr) atomicOr(A.risk, FLAG_UNDERFLOW);
}

PHK_SWEEP_LAUNCHER(trans, TArgs, 1)

}  // namespace phk
