// Arguments of the sweeps that run behind the forward pass, beside KArgs: one struct per sweep, shared between its kernels
// (launch_<sweep>.hip) and the host side (phk_api.hip).  A layout is a kernel-argument layout: fields keep their order.
#pragma once
#include <stdint.h>

namespace phk {

// posterior decoding (launch_decode.hip)
struct DArgs {
    int64_t bin;           // scored sites per bin (>= 1)
    int64_t nbin;          // bins per sequence: ceil((Ltot - W) / bin)
    const double* values;  // [B|1, K] value of every state (row stride vstride_b; 0 = shared), or null (no mean)
    int64_t vstride_b;
    void* mean;            // [B, S, nbin] real: mean over the bin of sum_k values_k gamma_t(k), or null
    void* marg;            // [B, S, nbin, K] real: mean over the bin of gamma_t, or null
};

// Viterbi decoding (launch_viterbi.hip)
struct VArgs {
    const int64_t* lens;  // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    uint8_t* path;        // [B, S, path_stride]: states at sites W .. len - 1, then 255
    int64_t path_stride;  // >= Ltot - W
};

// path-sampling traceback (launch_sample.hip)
struct SArgs {
    uint8_t* paths;       // [B, S, n_samples, path_stride] of the CALL: states at sites W .. Ltot - 1
    int64_t path_stride;  // >= Ltot - W
    int64_t n_samples;    // samples per sequence (>= 1)
    uint64_t seed;        // Philox key
    int64_t b0, s0;       // position of the slab in the call, and ...
    int64_t S_call;       // ... the call's S: q = (b0 + b) * S_call + (s0 + s) numbers the sequences of the call
};

// sampled tract spectra (launch_sample_tracts.hip): the traceback of SArgs with the paths reduced in place of stored
constexpr int TRACT_MAX_EDGES = 15;
struct XArgs {
    int32_t* stats;         // [B, S, n_samples, 4 + C] of the CALL, zeroed before the first launch (C = n_edges + 1)
    int32_t* cover;         // [B, S, nbin] of the CALL, zeroed before the first launch, or null
    int32_t* diff;          // workspace [B S of the launch, nbin], zeroed before the launch: +1 / -1 at the first / behind the last
                            // bin a qualifying tract covers whole (null exactly when cover is)
    const uint64_t* masks;  // [B] (mask_stride = 1) or [1] (0) of the launch: bit k set = state k is inside the set
    int64_t mask_stride;
    const int64_t* lens;    // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    int64_t n_samples;      // samples per sequence (>= 1)
    uint64_t seed;          // Philox key
    int64_t b0, s0;         // position of the slab in the call, and ...
    int64_t S_call;         // ... the call's S: q = (b0 + b) * S_call + (s0 + s) numbers the sequences of the call
    int32_t bin;            // reported sites per bin of cover (>= 1)
    int32_t nbin;           // bins per sequence: ceil((Ltot - W) / bin)
    int32_t min_len;        // cover counts the sites of tracts at least this long (>= 1)
    int32_t ncol;           // 4 + C
    int32_t edges[TRACT_MAX_EDGES];  // class of a tract of n sites = #{e : edges[e] <= n}; unused entries INT32_MAX
};

// transition posteriors (launch_trans.hip)
struct TArgs {
    int64_t bin;          // scored sites per bin (>= 1)
    int64_t nbin;         // bins per sequence: ceil((Ltot - W) / bin)
    const int64_t* lens;  // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    void* arr;            // [B, S, nbin, 3, K] real: mean over the bin's own sites of (stay, up, down), or null
    void* chg;            // [B, S, nbin, 2] real: sum over the bin's own sites of (sum_k up, sum_k down), or null
};

// leave-one-out predictive decoding (launch_loo.hip)
struct LArgs {
    int64_t bin;          // scored sites per bin (>= 1)
    int64_t nbin;         // bins per sequence: ceil((Ltot - W) / bin)
    const int64_t* lens;  // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    void* track;          // [B, S, nbin, 3] real: sums over the bin's own sites of (phet at observed sites, phet at missing
                          // sites, log score)
};

// tract posteriors (launch_tract.hip)
struct QArgs {
    int64_t bin;            // scored sites per bin (>= 1)
    int64_t nbin;           // bins per sequence: ceil((Ltot - W) / bin)
    const int64_t* lens;    // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    const double* weights;  // [B, K] (row stride wstride_b) or [K] (wstride_b = 0): the per-state weight m in [0, 1]
    int64_t wstride_b;
    void* tract;            // [B, S, nbin] real: E[prod of m(z_t) over the bin's own sites | o]
};

// bin moments (launch_moments.hip)
struct MArgs {
    int64_t bin;           // scored sites per bin (>= 1)
    int64_t nbin;          // bins per sequence: ceil((Ltot - W) / bin)
    const int64_t* lens;   // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    const double* values;  // [B, K] (row stride vstride_b) or [K] (vstride_b = 0): the per-state value v in [-1, 1]
    int64_t vstride_b;
    double* m1;            // [B, S, nbin]: E[S | o], S the sum of v(z_t) over the bin's own sites
    double* m2;            // [B, S, nbin]: E[S^2 | o]
};

// local likelihood-ratio scans (launch_local.hip)
struct RArgs {
    int64_t bin;           // scored sites per bin (>= 1)
    int64_t nbin;          // bins per sequence: ceil((Ltot - W) / bin)
    const int64_t* lens;   // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    const void* alt;       // [B, S|1, 7, K] real: the alternative blocks, laid out like KArgs::params (their pi row is not read)
    int64_t astride_b;     // element strides of alt
    int64_t astride_s;     // 0: one block per particle, broadcast over chunks
    const float* alt_prefold;  // pre-folded factors of the alternative blocks [B, S|1, 5, K] (float32 kernels), or null
    int64_t apfstride_b, apfstride_s;
    void* logratio;        // [B, S, nbin] real: log P(o | bin under the alternative) - log P(o)
};

// interval tracts (launch_interval.hip; interval_check_kernel in phk_api.hip).  The lists are the CALL's, in CSR form over its
// chunk positions: chunk position s owns the intervals iv_off[s] .. iv_off[s + 1] - 1, sorted, disjoint, half-open, in reported
// sites (position p is site W + p); n_iv = iv_off[S_call].
struct IArgs {
    const int64_t* lens;      // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    const int64_t* iv_off;    // [S_call + 1]
    const int64_t* iv_start;  // [n_iv]
    const int64_t* iv_end;    // [n_iv]: 0 <= start < end <= len - W
    const uint64_t* masks;    // [B, n_iv] (mstride_b = n_iv) or [n_iv] (0) of the call: bit k set = state k is inside the interval's set
    int64_t mstride_b;
    int64_t b0, s0;           // position of the slab in the call, and ...
    int64_t S_call;           // ... the call's S
    double* logp;             // [B, n_iv] of the call: log P(every site of the interval has its state in the set | o)
    // workspace written by interval_check_kernel before the first slab's sweep
    const unsigned long long* left;  // [max(units, 1)]: the leftmost site any sequence of the call needs from the unit (none: huge)
    const int32_t* bad;       // [S_call]: 1 = the chunk position's list failed the check: nothing of it is swept (its logp are NaN)
    int32_t search_iters;     // iterations of the cursor's binary search: bit length of Ltot - W, an upper bound on a list's length
};

// pair counts (launch_pairs.hip)
struct PArgs {
    const int64_t* lens;  // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    double* part;         // workspace [max(units, 1), B S of the launch, K, K]: every unit's own sum of raw outer products
    double* counts;       // [B, S, K, K] of the launch, the caller's order: expected moves from state i (first) to state j
    int row0;             // first origin state of the row tile this launch accumulates (set by the launcher; 0 on the matrix path)
};

}  // namespace phk
