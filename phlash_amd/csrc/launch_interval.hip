// Interval-tract sweep: for every interval of a per-row list, log P(EVERY site of the interval has its state in the interval's
// own set | o).  One translation unit per (real, K), compiled with -DPHK_REAL=float|double -DPHK_K=<K> -DPHK_SUFFIX=<tag> (see the
// Makefile: launch_interval_<real>_<K>.o).
//
// This is tract_kernel (launch_tract.hip) with local_kernel's exponent (launch_local.hip): the same units, beta seeds, forward
// re-run and rescale schedule.  For the interval of sites s .. e with the indicator m of its set,
//     q_e = beta_e,      q_{t-1} = A (m .* e_{o_t} .* q_t)   for t = e, e-1, .., s,
//     logp = log sum_i alpha_{s-1}(i) q_{s-1}(i) - log sum_i alpha_{s-1}(i) beta_{s-1}(i).
// q runs through beta's own recursion (tract_step) and carries an integer power-of-two exponent qe RELATIVE to beta: where beta is
// rescaled q is renormalised to its own sum and qe takes the difference of the two exponents, so a tract of a few thousand sites
// whose probability is far below the float range keeps its digits; the log (local_log, in float64 for either type) is taken at
// the store.  With every bit of the model's states set q steps through beta's operations on beta's bits: q == beta, qe == 0 and
// logp is exactly 0.  With no bit set q is 0 and logp is -inf.
//
// What differs from the two kernels is where a "bin" begins and ends and which m applies.  The intervals come from per-row lists
// (IArgs, CSR over the call's chunk positions), so the groups of one wave -- up to three data rows, chunk-major -- are at
// different places of different lists.  The control flow stays the launch's: the reset q = beta at an interval's last site and
// the change of m are selects, the store at its first site is predicated, and the two sums against alpha run for the whole wave
// whenever a wave vote finds some group at a first site.  Each group keeps a cursor into its row's list -- found once, by a
// binary search of a fixed number of steps, at the unit's right edge -- with the current interval's first site, last site and m
// in registers; the cursor moves (three loads, no cross-lane operation) behind a store.  Between intervals q keeps stepping with
// the last m: it is overwritten at the next interval's last site.
//
// An interval belongs to the unit that holds its last site; the unit walks left past its own edge to the leftmost first site any
// sequence of the call needs from it (IArgs::left, written by interval_check_kernel, which also checks the lists: a list that
// fails is not swept at all).  One value per interval and particle; one writer, no atomics.
#include "psmc_kernels.hip"
#include "sweep_common.h"

namespace phk {

// kernel ids of the interval sweep in the overrun record (KArgs::risk[1]; phk_underflow_risk names them)
constexpr int OVERRUN_INTERVAL_SERIAL = 23;
constexpr int OVERRUN_INTERVAL_SEG = 24;

// SEG = false: one unit per sequence walks every block.  SEG = true: blockIdx.y picks a unit of the segment layout, seeded from
// the beta scan's value at its right edge (see decode_kernel: the units and their seeds are the same).
template <typename real, int K, int R, int T, int NRM, bool SEG>
__global__ __launch_bounds__(NT_MAX, (sweep_waves_per_simd<real>(sweep_hold<real, T>()))) void interval_kernel(KArgs A, IArgs D) {
    using L = Lane<real, K, R>;
    using V = typename L::V;
    constexpr int SPL = L::SPL, NP = L::NP;
    static_assert(T <= 16 && 16 % T == 0 && T % NRM == 0, "block / rescale schedule");
    static_assert(K <= 64, "a state set is a 64-bit mask");
    // sites whose alphas are held at once: the whole block, but a quarter of a 16-site float64 block, as tract_kernel
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

    // Sites of this unit: the same for every sequence of the launch, and so is how far it walks (D.left).
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
    const unsigned long long left = D.left[SEG ? blockIdx.y : 0];  // first site of the leftmost interval whose last site is here
    if (blk_hi <= blk_lo || left >= (unsigned long long)s_hi) return;
    const int b_bot = (int)((int64_t)left / T);

    L lane;
    V pi[NP];
    lane.load((const real*)A.params + bb * A.pstride_b + ss * A.pstride_s, rank, (real*)smem_raw + (size_t)tid * L::ETAB_STRIDE, pi);
    const real* pfb = prefold_block<real>(A, bb, ss);
    (void)lane.try_fold(pfb != nullptr ? pfb + rank * SPL : nullptr);  // the forward kernel's factors, to the bit

    // The group's list and its cursor: the last interval whose last site is below s_hi (ends ascend: a binary search, a step
    // count of the launch's), kept while the interval's last site is at or above s_lo.
    const int64_t cs = D.s0 + ss;  // chunk position in the call
    const int64_t n_iv = D.iv_off[D.S_call];
    const int64_t lo = D.iv_off[cs];
    const int64_t hi = D.bad[cs] ? lo : D.iv_off[cs + 1];
    const uint64_t* mrow = D.masks + (D.b0 + bb) * D.mstride_b;
    double* const out = D.logp + (D.b0 + bb) * n_iv;
    int64_t cur = lo;
    {
        int64_t n = hi - lo;  // cur <- lo + #{j : W + end_j <= s_hi}
        for (int it = 0; it < D.search_iters; ++it) {
            if (n > 0) {
                const int64_t half = n >> 1;
                const bool below = W + D.iv_end[cur + half] <= s_hi;
                cur = below ? cur + half + 1 : cur;
                n = below ? n - half - 1 : half;
            }
        }
        --cur;
    }
    int64_t t_first = -1, t_last = -1;  // sites of the current interval (-1: the group has none left in this unit)
    V m[NP];
#pragma unroll
    for (int h = 0; h < NP; ++h) m[h] = splat<real>(real(0));
    // the interval at the cursor, if it is this unit's: its sites, and m from the mask bits rank * SPL + i
    const auto fetch = [&]() {
        t_first = t_last = -1;
        uint64_t bits = 0;
        if (cur >= lo) {
            const int64_t e = W + D.iv_end[cur] - 1;
            if (e >= s_lo) {
                t_last = e;
                t_first = W + D.iv_start[cur];
                bits = mrow[cur];
            }
        }
        const uint32_t mine = (uint32_t)(bits >> (rank * SPL)) & ((1u << SPL) - 1u);
#pragma unroll
        for (int i = 0; i < SPL; ++i) L::set(m, i, ((mine >> i) & 1u) ? real(1) : real(0));
    };
    fetch();

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
    int qe = 0;  // q's exponent relative to beta: the q of the definition, on beta's scale, is q 2^qe

    const int64_t row = checked_row(A, ss);
    const uint32_t* words = A.packed + row * A.Lw;
    const int64_t ck_step = nseq * K;
    const real* ck = (const real*)A.ckpt + L::ck_lane(nseq, seq, rank);
    constexpr int RISK_EXP = sizeof(real) == 4 ? RISK_EXP_F32 : RISK_EXP_F64;
    bool risky = false;

    int budget = SEG ? A.loop_budget[3] : A.loop_budget[1];  // (see KArgs::loop_budget)
    for (int blk = blk_hi - 1; blk >= b_bot; --blk) {
        if (__builtin_expect(--budget < 0, 0)) {
            report_overrun(A, SEG ? OVERRUN_INTERVAL_SEG : OVERRUN_INTERVAL_SERIAL, seq, blk);
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
            // beta pass, right to left.  Per site: q = beta (qe = 0) where the group's interval ends; beta <- A (e .* beta) and
            // q <- A (m .* e .* q); where beta is rescaled, q is renormalised to its own sum and qe takes the difference of the
            // two exponents; where some group's interval begins the two sums against the alpha before the site, that group's
            // log and store, and its cursor moves on.
#pragma unroll
            for (int j = H - 1; j >= 0; --j) {
                const int i = i0 + j;
                if (i < ns) {
                    const int64_t t = t0 + i;
                    const int code = (codes >> (2 * i)) & 3;
                    const bool ends = t == t_last;
#pragma unroll
                    for (int h = 0; h < NP; ++h) q[h] = ends ? beta[h] : q[h];
                    qe = ends ? 0 : qe;
                    V e[NP], em[NP];
                    lane.emis(code, e);
#pragma unroll
                    for (int h = 0; h < NP; ++h) em[h] = e[h] * m[h];  // (a missing site has e = 1 and is restricted all the same)
                    tract_step(lane, q, em);
                    const bool SC = rescale_after<NRM>(H - 1 - j);
                    const int ex = lane.bt_site(beta, e, SC);
                    if (SC) {
                        const int xq = frexp_exp_(lane.total(q));        // (0 for a sum of 0: q stays as it is)
                        const V s2 = splat<real>(ldexp_(real(1), -xq));  // exact power of two
#pragma unroll
                        for (int h = 0; h < NP; ++h) q[h] = q[h] * s2;
                        qe += xq - ex;
                        if (NRM > 1) risky = risky || ex < RISK_EXP;
                    }
                    const bool begins = t == t_first;
                    if (__any(begins)) {  // (a vote: the sums cross lanes and need the whole wave)
                        const V(&ap)[NP] = j > 0 ? al[j > 0 ? j - 1 : 0] : a0;
                        V xq[NP], xb[NP];
#pragma unroll
                        for (int h = 0; h < NP; ++h) {
                            xq[h] = ap[h] * q[h];
                            xb[h] = ap[h] * beta[h];
                        }
                        const real num = lane.total(xq), den = lane.total(xb);
                        const bool ok = den > real(0);
                        risky = risky || (begins && !ok);
                        const double val = ok ? local_log<double>((double)num / (double)den, qe) : 0.0;
                        if (begins && active && rank == 0) out[cur] = val;
                    }
                    if (begins) {
                        --cur;
                        fetch();
                    }
                }
            }
        }
    }
    if (risky && active && A.risk != nullptr) atomicOr(A.risk, FLAG_UNDERFLOW);
}

PHK_SWEEP_LAUNCHER(interval, IArgs, 1)

}  // namespace phk
