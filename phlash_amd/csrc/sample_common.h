// What the kernels that trace sampled paths back share (launch_sample.hip: the paths stored; launch_sample_tracts.hip: the
// paths reduced to tract statistics): the generator, one draw, and the samples a unit carries.  Include it after psmc_kernels.hip
// and sweep_common.h.  The draws of the two kernels are the same because this code is the same.
#pragma once

namespace phk {

// Samples per unit where a call asks for more than one (one sample: NS = 1).  Chosen per (real, K) from the compiler's
// resource report: the largest of {1, 2, 4} at which no kernel of the unit has scratch or AGPR copies.
template <typename real, int K>
constexpr int sample_ns() { return sizeof(real) == 8 || K == 4 ? 2 : 4; }


template <int CTRL>
__device__ __forceinline__ int dppi_(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, false);
}

// Philox4x32-10 (Salmon et al., SC'11): words x0, x1 of the output block
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t& x0,
                                              uint32_t& x1) {
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
    x0 = c0;
    x1 = c1;
}
// U in [0, 1): 53 bits for the float64 kernels, the top 24 of the same number for the float32 ones
__device__ __forceinline__ void uniform_of(uint32_t x0, uint32_t x1, double& U) {
    U = (double)(((uint64_t)x0 << 21) + (uint64_t)(x1 >> 11)) * 0x1p-53;
}
__device__ __forceinline__ void uniform_of(uint32_t x0, uint32_t, float& U) { U = (float)(x0 >> 8) * 0x1p-24f; }

// every lane reads the value of the lane at byte address `addr` (4 x lane number) of its wave
__device__ __forceinline__ float lane_read(float x, int addr) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, x)));
}
__device__ __forceinline__ double lane_read(double x, int addr) {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)(u >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

template <typename real, int K, int R>
struct SampleLane {
    using L = Lane<real, K, R>;
    using V = typename L::V;
    static constexpr int SPL = L::SPL, NP = L::NP;
    static_assert(SPL == SWEEP_SPL, "four states per lane");
    real u[SPL];
    int k0;

    __device__ __forceinline__ void init(const L& lane, int rank) {
        k0 = rank * SPL;
#pragma unroll
        for (int i = 0; i < SPL; ++i) u[i] = L::get(lane.u, i);
    }
    // sum over the R lanes of the group (every lane gets it)
    static __device__ __forceinline__ int isum(int x) {
        if constexpr (R >= 2) x += dppi_<QP(1, 0, 3, 2)>(x);
        if constexpr (R >= 4) x += dppi_<QP(2, 3, 0, 1)>(x);
        if constexpr (R >= 8) x += dppi_<ROW_HALF_MIRROR>(x);
        if constexpr (R >= 16) x += dppi_<ROW_MIRROR>(x);
        return x;
    }
    // One draw.  x: alpha after the site; cur: the state at the next site (the same in every lane of the group), or, with
    // `last` (the row's last site), nothing.  fac: the group's factors in LDS, [b | d | v][K].  Returns the state drawn (the same
    // in every lane of the group); ok = false where the weights have no mass.
    __device__ __forceinline__ int draw(const L& lane, const V (&x)[NP], const int cur, const bool last, const real U, const real* fac,
                                        bool& ok) const {
        const real bj = fac[cur], dj = fac[K + cur], vj = fac[2 * K + cur];
        real c[SPL], run = real(0);
#pragma unroll
        for (int i = 0; i < SPL; ++i) {
            const int k = k0 + i;
            const real xi = L::get(x, i);
            const real lo = (u[i] * xi) * vj;
            const real hi = (k == cur ? dj : bj) * xi;
            const real w = last ? xi : (k < cur ? lo : hi);
            run = run + w;
            c[i] = run;
        }
        const real tot = lane.g.sum(run);
        const real off = lane.g.excl_prefix(run);
        const real theta = U * tot;
        ok = ok && tot > real(0);
        int n = 0;
#pragma unroll
        for (int i = 0; i < SPL; ++i) n += (k0 + i <= K - 2 && off + c[i] <= theta) ? 1 : 0;
        return isum(n);
    }
};

}  // namespace phk
