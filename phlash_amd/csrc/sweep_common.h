// What the sweep translation units (launch_<sweep>.hip, one object per (real, K)) share beside the kernels of
// psmc_kernels.hip: include it after psmc_kernels.hip.  Every unit is compiled with -DPHK_REAL=float|double -DPHK_K=<K>
// -DPHK_SUFFIX=<tag> (see the Makefile) and runs 4 states per lane (R = K / 4).
#pragma once
#include "sweep_args.h"

#ifndef PHK_REAL
#error "compile with -DPHK_REAL=float|double -DPHK_K=<K> -DPHK_SUFFIX=<tag>"
#endif

#define PHK_CAT2(a, b) a##b
#define PHK_CAT(a, b) PHK_CAT2(a, b)

namespace phk {

constexpr int SWEEP_SPL = 4;  // states per lane
constexpr int SWEEP_R = PHK_K / SWEEP_SPL;

// own length of the sequence's data row, clamped to (W, Ltot] (out of range: FLAG_BAD_INDEX, as a bad chunk index)
template <typename DA>
__device__ __forceinline__ int64_t sweep_len(const KArgs& A, const DA& D, int64_t row) {
    if (D.lens == nullptr) return A.Ltot;
    int64_t n = D.lens[row];
    if (n <= A.W || n > A.Ltot) {
        if (A.risk != nullptr) atomicOr(A.risk, FLAG_BAD_INDEX);
        n = n > A.Ltot ? A.Ltot : A.W + 1;
    }
    return n;
}

// sites whose alphas a sweep with per-site terms holds at once: the whole block, but a quarter of a 16-site float64 block
// (see trans_kernel)
template <typename real, int T>
constexpr int sweep_hold() { return sizeof(real) == 8 && T == 16 ? 4 : T; }
// waves per SIMD the launch bounds ask for: two where `held` alpha vectors fit in 256 bytes of registers per lane
template <typename real>
constexpr int sweep_waves_per_simd(int held) { return held * SWEEP_SPL * (int)sizeof(real) <= 256 ? 2 : 1; }

// q <- A (em .* q): Lane::bt_site's recursion without a rescale of its own (the tract sweep's q takes beta's, the interval
// sweep renormalises q itself)
template <typename L>
__device__ __forceinline__ void tract_step(const L& lane, typename L::V (&q)[L::NP], const typename L::V (&em)[L::NP]) {
    using V = typename L::V;
    constexpr int NP = L::NP;
    V w[NP], svw[NP], pbw[NP], cb;
#pragma unroll
    for (int h = 0; h < NP; ++h) w[h] = q[h] * em[h];
    lane.scans_adj(w, svw, pbw, cb);
#pragma unroll
    for (int h = 0; h < NP; ++h) q[h] = lane.beta_prev(h, w, svw, pbw, cb);
}

__device__ __forceinline__ float log_(float x) { return logf(x); }
__device__ __forceinline__ double log_(double x) { return log(x); }
__device__ __forceinline__ float frexp_(float x, int* e) { return frexpf(x, e); }
__device__ __forceinline__ double frexp_(double x, int* e) { return frexp(x, e); }

// log(r 2^qe) for r >= 0: the exponent is folded into the ratio while the product is a normal number (exact: r = 1, qe = 0
// gives 0), and added in the log domain where it is not
template <typename real>
__device__ __forceinline__ real local_log(real r, int qe) {
    constexpr int LIM = sizeof(real) == 4 ? 120 : 1000;
    int er;
    const real m = frexp_(r, &er);  // r = m 2^er, m in [0.5, 1) (0 for r = 0)
    const int E = er + qe;
    if (E > -LIM && E < LIM) return log_(ldexp_(m, E));
    // E ln 2 + log m with ln 2 in two parts of the kernel's type (the first exact in a product with |E| < 2^11)
    constexpr real LN2_HI = sizeof(real) == 4 ? real(0x1.62ep-1) : real(0x1.62e42fefa38p-1);
    constexpr real LN2_LO = real(0.6931471805599453094 - (double)LN2_HI);
    return fma_(real(E), LN2_HI, fma_(real(E), LN2_LO, log_(m)));
}

// Host launchers of a sweep whose kernel is <stem>_kernel<real, K, R, T, NRM, SEG>(KArgs, DA).
// PHK_SWEEP_TN: <stem>_tn<T, NRM>(a, d, units, nt, st), one launch; units <= 0: one serial sweep per sequence, else the
// segment layout of the segmented plan (KArgs::seg_blocks, bseg).  TABLES: emission tables per thread in LDS (one per model).
#define PHK_SWEEP_TN(stem, DA, TABLES)                                                                                                    \
    template <int T, int NRM>                                                                                                             \
    static hipError_t stem##_tn(const KArgs& a, const DA& d, int units, int nt, hipStream_t st) {                                         \
        using L = Lane<PHK_REAL, PHK_K, SWEEP_R>;                                                                                         \
        const int64_t nseq = (a.seq_end > 0 ? a.seq_end : a.B * a.S) - a.seq_begin;                                                       \
        const int spb = nt / SWEEP_R;                                                                                                     \
        const size_t lds = (size_t)(TABLES) * L::ETAB_STRIDE * nt * sizeof(PHK_REAL);                                                     \
        const dim3 grid((unsigned)((nseq + spb - 1) / spb), (unsigned)(units <= 0 ? 1 : units)), block(nt);                               \
        if (units <= 0) hipLaunchKernelGGL((stem##_kernel<PHK_REAL, PHK_K, SWEEP_R, T, NRM, false>), grid, block, lds, st, a, d);         \
        else hipLaunchKernelGGL((stem##_kernel<PHK_REAL, PHK_K, SWEEP_R, T, NRM, true>), grid, block, lds, st, a, d);                     \
        return hipGetLastError();                                                                                                         \
    }
// PHK_SWEEP_DISPATCH: <stem>_any(T, nrm, ...) picks <stem>_tn<T, NRM>.  T: the checkpoint spacing of the forward kernel that
// ran before; nrm: its rescale interval.
#define PHK_SWEEP_DISPATCH(stem, DA)                                                                                                      \
    template <int T>                                                                                                                      \
    static hipError_t stem##_t(int nrm, const KArgs& a, const DA& d, int units, int nt, hipStream_t st) {                                 \
        if (nrm == 1) return stem##_tn<T, 1>(a, d, units, nt, st);                                                                        \
        if (nrm == 2) return stem##_tn<T, 2>(a, d, units, nt, st);                                                                        \
        if (nrm == 4) return stem##_tn<T, 4>(a, d, units, nt, st);                                                                        \
        return hipErrorInvalidValue;                                                                                                      \
    }                                                                                                                                     \
    static hipError_t stem##_any(int T, int nrm, const KArgs& a, const DA& d, int units, int nt, hipStream_t st) {                        \
        if (T == 8) return stem##_t<8>(nrm, a, d, units, nt, st);                                                                         \
        if (T == 16) return stem##_t<16>(nrm, a, d, units, nt, st);                                                                       \
        return hipErrorInvalidValue;                                                                                                      \
    }
// PHK_SWEEP_LAUNCHER: both, and the exported launch_<stem>_<suffix>(T, nrm, a, d, units, nt, st)
#define PHK_SWEEP_LAUNCHER(stem, DA, TABLES)                                                                                              \
    PHK_SWEEP_TN(stem, DA, TABLES)                                                                                                        \
    PHK_SWEEP_DISPATCH(stem, DA)                                                                                                          \
    hipError_t PHK_CAT(launch_##stem##_, PHK_SUFFIX)(int T, int nrm, const KArgs& a, const DA& d, int units, int nt, hipStream_t st) {    \
        return stem##_any(T, nrm, a, d, units, nt, st);                                                                                   \
    }

}  // namespace phk
