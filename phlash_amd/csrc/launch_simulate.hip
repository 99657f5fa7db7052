// Posterior predictive simulation (phk_simulate): replicate observation rows drawn from the HMM itself, n_rep per
// (particle, row), under the row's own accessibility mask; stored as rows, or reduced on the fly to het counts per bin and
// a histogram of the lengths of hom runs, or both.  One translation unit, float64 only, K a run-time value in [2, 64].
//
// The definition (include/phlash_hip.h, phk_simulate, states it in full; the tests restate it with loops on the CPU).
// Row i of the transition matrix is b_j (j < i), d_i, u_i v_j (j > i), so with the serial prefix sums cb, cv of b, v a
// transition draw from state i is theta = U1 (cb_{i-1} + d_i + u_i (cv_{K-1} - cv_i)), three comparisons, and -- only when
// the state moves -- a search in cb below i or in u_i (cv_k - cv_i) above it.  Uniforms: Philox4x32-10 with phk_sample_paths'
// key and constants; the block at counter (t, r, q lo, q hi) gives U1_t (words 0, 1: the transition into site t) and U2_t
// (words 2, 3: the emission at site t); site 0xFFFFFFFF gives the start.  No division anywhere, every operation IEEE
// float64 in the order the header writes (-ffp-contract=off), so the result is equal to the CPU restatement's, not close to it.
//
// simulate_kernel<ROWS, STATS>: one lane per sequence (b, s, r); a 64-lane workgroup takes sequences that share a parameter
// block and builds its nine tables in LDS once (4.5 KB: cp, cb, cv, the exclusive cb, d, u, tot, emis0 + emis1, emis1).  The
// five numbers a draw needs of the CURRENT state (exclusive cb, d, tot, emis0 + emis1, emis1) live in registers and are
// read again only when the state moves, so the serial chain of a site is a multiply, a subtraction and two comparisons.  A
// state or emission row without mass is rewritten in the tables so that the same comparisons make the state stay and the
// code 0 (tot = 0, exclusive cb = 0, d = +inf; emis sum = 0, emis1 = -inf); the sentinels raise the flag.
// Sites go in blocks of SIM_T = 16: the 16 Philox blocks do not depend on the state and are generated ahead of the chain;
// the 16 codes / states are packed into four registers each and leave as ONE 16-byte store per lane and output; the tail
// (L mod 16 sites) goes site by site with byte stores and writes nothing at or past L.  The run histogram (32 counters
// indexed by a run-time bucket) is a [32][64] int table in LDS, 8 KB, bucket-major: lane l owns column l and the 64 lanes of
// an access fall on 64 consecutive words.  Every loop is counted: the site loop by the host's L / 16, the search by
// ceil(log2 K).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "simulate_args.h"

namespace phk {

namespace {

constexpr int SIM_CP = 0, SIM_CB = 1, SIM_CV = 2, SIM_PB = 3, SIM_D = 4, SIM_U = 5, SIM_TOT = 6, SIM_ES = 7, SIM_E1 = 8, SIM_NTAB = 9;

// Philox4x32-10 (Salmon et al., SC'11), all four output words
__device__ __forceinline__ void sim_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&x)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x[0] = c0;
    x[1] = c1;
    x[2] = c2;
    x[3] = c3;
}
__device__ __forceinline__ double sim_u53(uint32_t x0, uint32_t x1) {
    return (double)(((uint64_t)x0 << 21) + (uint64_t)(x1 >> 11)) * 0x1p-53;
}

struct SimState {
    int z;
    double pb, d, tot, es, e1;  // of state z: exclusive cb, diagonal, row total, emis0 + emis1, emis1 (sentinels: see above)
    __device__ __forceinline__ void load(const double* tab, int j) {
        z = j;
        pb = tab[SIM_PB * SIM_MAXK + j];
        d = tab[SIM_D * SIM_MAXK + j];
        tot = tab[SIM_TOT * SIM_MAXK + j];
        es = tab[SIM_ES * SIM_MAXK + j];
        e1 = tab[SIM_E1 * SIM_MAXK + j];
    }
};

// the transition into a site and the emission there: -> 1 (het) or 0
__device__ __forceinline__ int sim_site(const double* tab, int K, int nsearch, SimState& st, double U1, double U2, bool& bad) {
    bad |= st.d == INFINITY;
    const double th = U1 * st.tot;
    const bool left = th < st.pb;
    const double phi = th - st.pb;
    if (left || !(phi < st.d)) {
        // the state moves: count the entries of one monotone table that do not exceed the target, by bisection.
        // below i: cb_k <= theta, k in [0, i);  above i: u_i (cv_k - cv_i) <= psi, k in (i, K-2]
        const int i = st.z;
        const double uu = left ? 1.0 : tab[SIM_U * SIM_MAXK + i];
        const double cc = left ? 0.0 : tab[SIM_CV * SIM_MAXK + i];
        const double target = left ? th : phi - st.d;
        const int off = left ? SIM_CB * SIM_MAXK : SIM_CV * SIM_MAXK;
        int lo = left ? 0 : i + 1, hi = left ? i : K - 1;
        for (int it = 0; it < nsearch; ++it) {
            if (lo >= hi) break;
            const int mid = (lo + hi) >> 1;
            if (uu * (tab[off + mid] - cc) <= target) lo = mid + 1;  // (1 (x - 0) is x: the same comparison on either side)
            else hi = mid;
        }
        st.load(tab, lo < K - 1 ? lo : K - 1);
    }
    bad |= st.e1 == -INFINITY;
    return U2 * st.es < st.e1 ? 1 : 0;
}

struct SimStats {
    int32_t* het;  // this sequence's [nbin], or NULL
    int bin, pos, count;
    int64_t bi;
    uint32_t run;
    __device__ __forceinline__ void site(int code, int* hist) {
        count += code == 1;
        if (++pos == bin) {
            if (het) het[bi] = count;
            ++bi;
            count = 0;
            pos = 0;
        }
        if (code == 0) {
            ++run;
        } else if (run) {
            hist[(31 - __clz(run)) * SIM_NT] += 1;
            run = 0;
        }
    }
    __device__ __forceinline__ void finish(int* hist) {
        if (pos > 0 && het) het[bi] = count;
        if (run) hist[(31 - __clz(run)) * SIM_NT] += 1;
    }
};

template <bool ROWS, bool STATS>
__global__ __launch_bounds__(SIM_NT) void simulate_kernel(SimArgs A) {
    __shared__ double tab[SIM_NTAB * SIM_MAXK];
    __shared__ int hist_s[STATS ? 32 * SIM_NT : 1];
    const int K = A.K, tid = threadIdx.x;
    const int64_t pbk = (int64_t)blockIdx.x / A.chunks;  // parameter block
    const int64_t idx = ((int64_t)blockIdx.x - pbk * A.chunks) * SIM_NT + tid;
    const int64_t b = A.per_row ? pbk / A.S : pbk;
    const int64_t s_blk = A.per_row ? pbk - b * A.S : 0;
    const double* P = A.params + b * A.pstride_b + s_blk * A.pstride_s;

    // ---- tables: serial sums in ascending index, as the definition has them ----------------------------------------
    if (tid == 0) {
        double cp = 0.0, cb = 0.0, cv = 0.0;
        for (int k = 0; k < K; ++k) {
            tab[SIM_PB * SIM_MAXK + k] = cb;
            cb += P[0 * K + k];
            cv += P[3 * K + k];
            cp += P[6 * K + k];
            tab[SIM_CP * SIM_MAXK + k] = cp;
            tab[SIM_CB * SIM_MAXK + k] = cb;
            tab[SIM_CV * SIM_MAXK + k] = cv;
        }
    }
    __syncthreads();
    if (tid < K) {
        const double pb = tab[SIM_PB * SIM_MAXK + tid], d = P[1 * K + tid], u = P[2 * K + tid];
        const double sv = tab[SIM_CV * SIM_MAXK + K - 1] - tab[SIM_CV * SIM_MAXK + tid];
        const double tot = pb + d + u * sv;
        const bool ok = tot > 0.0 && tot < INFINITY;
        tab[SIM_U * SIM_MAXK + tid] = u;
        tab[SIM_TOT * SIM_MAXK + tid] = ok ? tot : 0.0;
        tab[SIM_D * SIM_MAXK + tid] = ok ? d : INFINITY;
        const double e1 = P[5 * K + tid], es = P[4 * K + tid] + e1;
        const bool eok = es > 0.0 && es < INFINITY;
        tab[SIM_ES * SIM_MAXK + tid] = eok ? es : 0.0;
        tab[SIM_E1 * SIM_MAXK + tid] = eok ? e1 : -INFINITY;
    }
    __syncthreads();
    if (tid < K) {
        if (!(tab[SIM_TOT * SIM_MAXK + tid] > 0.0)) tab[SIM_PB * SIM_MAXK + tid] = 0.0;
    }
    __syncthreads();
    if (idx >= A.per_block) return;

    const int64_t s = A.per_row ? s_blk : idx / A.n_rep;
    const int64_t r = A.per_row ? idx : idx - s * A.n_rep;
    const uint64_t q = (uint64_t)(A.seq0 + b * A.S + s);
    const uint32_t qlo = (uint32_t)q, qhi = (uint32_t)(q >> 32), rr = (uint32_t)r;
    const int64_t seq = (b * A.S + s) * A.n_rep + r;  // the sequence's row in every output
    const int8_t* mrow = A.mask ? A.mask + s * A.mask_stride : nullptr;
    int8_t* orow = ROWS && A.obs ? A.obs + seq * A.row_stride : nullptr;
    uint8_t* prow = ROWS && A.paths ? A.paths + seq * A.row_stride : nullptr;
    int* hist = hist_s + tid;
    SimStats stats;
    if constexpr (STATS) {
#pragma unroll
        for (int k = 0; k < 32; ++k) hist[k * SIM_NT] = 0;
        stats.het = A.het ? A.het + seq * A.nbin : nullptr;
        stats.bin = (int)A.bin;
        stats.pos = 0;
        stats.count = 0;
        stats.bi = 0;
        stats.run = 0;
    }
    int nsearch = 0;  // ceil(log2 K) halvings close any range of at most K - 1 entries
    while ((1 << nsearch) < K) ++nsearch;

    // ---- the state before site 0 -----------------------------------------------------------------------------------
    bool bad = false;
    SimState st;
    {
        const double cpK = tab[SIM_CP * SIM_MAXK + K - 1];
        int z = 0;
        if (cpK > 0.0 && cpK < INFINITY) {
            uint32_t x[4];
            sim_philox(0xFFFFFFFFu, rr, qlo, qhi, A.key0, A.key1, x);
            const double th = sim_u53(x[0], x[1]) * cpK;
            for (int k = 0; k < K - 1; ++k) z += tab[SIM_CP * SIM_MAXK + k] <= th;
        } else {
            bad = true;
        }
        st.load(tab, z);
    }

    // ---- whole blocks of SIM_T sites -------------------------------------------------------------------------------
    for (int64_t blk = 0; blk < A.nfull; ++blk) {
        const int64_t t0 = blk * SIM_T;
        uint32_t mk[4] = {0u, 0u, 0u, 0u};
        if (mrow) {
            if (A.mask_vec) {
                const uint4 m4 = *reinterpret_cast<const uint4*>(mrow + t0);
                mk[0] = m4.x;
                mk[1] = m4.y;
                mk[2] = m4.z;
                mk[3] = m4.w;
            } else {
#pragma unroll
                for (int k = 0; k < SIM_T; ++k) mk[k >> 2] |= (uint32_t)(uint8_t)mrow[t0 + k] << (8 * (k & 3));
            }
        }
        double U1[SIM_T], U2[SIM_T];
#pragma unroll
        for (int k = 0; k < SIM_T; ++k) {
            uint32_t x[4];
            sim_philox((uint32_t)t0 + (uint32_t)k, rr, qlo, qhi, A.key0, A.key1, x);
            U1[k] = sim_u53(x[0], x[1]);
            U2[k] = sim_u53(x[2], x[3]);
        }
        uint32_t ow[4] = {0u, 0u, 0u, 0u}, pw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < SIM_T; ++k) {
            const int het = sim_site(tab, K, nsearch, st, U1[k], U2[k], bad);
            const int code = (mk[k >> 2] >> (8 * (k & 3))) & 0x80u ? -1 : het;
            if constexpr (ROWS) {
                ow[k >> 2] |= (uint32_t)(uint8_t)code << (8 * (k & 3));
                pw[k >> 2] |= (uint32_t)st.z << (8 * (k & 3));
            }
            if constexpr (STATS) stats.site(code, hist);
        }
        if constexpr (ROWS) {
            if (orow) *reinterpret_cast<uint4*>(orow + t0) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
            if (prow) *reinterpret_cast<uint4*>(prow + t0) = make_uint4(pw[0], pw[1], pw[2], pw[3]);
        }
    }
    // ---- the tail: L mod SIM_T sites, one at a time, nothing written at or past L ----------------------------------
    const int rem = (int)(A.L - A.nfull * SIM_T);
    for (int k = 0; k < rem; ++k) {
        const int64_t t = A.nfull * SIM_T + k;
        uint32_t x[4];
        sim_philox((uint32_t)t, rr, qlo, qhi, A.key0, A.key1, x);
        const int het = sim_site(tab, K, nsearch, st, sim_u53(x[0], x[1]), sim_u53(x[2], x[3]), bad);
        const int code = mrow && mrow[t] < 0 ? -1 : het;
        if constexpr (ROWS) {
            if (orow) orow[t] = (int8_t)code;
            if (prow) prow[t] = (uint8_t)st.z;
        }
        if constexpr (STATS) stats.site(code, hist);
    }
    if constexpr (STATS) {
        stats.finish(hist);
        if (A.runs) {
            int32_t* out = A.runs + seq * 32;
#pragma unroll
            for (int k = 0; k < 32; ++k) out[k] = hist[k * SIM_NT];
        }
    }
    if (bad) *A.flags = 1;
}

}  // namespace

hipError_t launch_simulate(const SimArgs& a, hipStream_t st) {
    const bool rows = a.obs || a.paths, stats = a.het || a.runs;
    const dim3 grid((unsigned)((a.per_row ? a.B * a.S : a.B) * a.chunks)), block(SIM_NT);
    if (rows && stats) hipLaunchKernelGGL((simulate_kernel<true, true>), grid, block, 0, st, a);
    else if (rows) hipLaunchKernelGGL((simulate_kernel<true, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((simulate_kernel<false, true>), grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace phk
