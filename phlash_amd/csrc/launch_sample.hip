// Posterior path sampling (forward-filtering backward-sampling): whole hidden paths z ~ P(z | o), n_samples per sequence.
// One translation unit per (real, K), compiled with -DPHK_REAL=float|double -DPHK_K=<K> -DPHK_SUFFIX=<tag> (see the
// Makefile: launch_sample_<real>_<K>.o).  The kernel runs after the plan's forward kernel and reads its alpha checkpoints
// (KArgs::ckpt), as the posterior-decoding sweep does; it needs no beta.
//
// The definition (include/phlash_hip.h, phk_sample_paths, states it in full).  With alpha_t the forward vector after site t:
// the state at the last site is drawn with weights alpha_{L-1}(i); the state at site t < L - 1 given state j at site t + 1
// with weights
//     (u_i alpha_t(i)) v_j  (i < j),     d_j alpha_t(j)  (i = j),     b_j alpha_t(i)  (i > j)
// -- the products VitLane::predecessor compares, here summed: column j of A times alpha_t.  The folded factors of column
// j (Lane::try_fold) multiply every candidate alike, so the folded model is as valid here as in the other kernels.  One
// draw: c = inclusive prefix sum of the weights, theta = U c_{K-1}, state = #{i <= K - 2 : c_i <= theta}.  U comes from
// Philox4x32-10 with counter (site, sample, sequence of the call lo, hi) and key (seed lo, hi): a draw depends on nothing
// but (seed, sequence, sample, site) and the alphas, so neither the slabs, nor the samples that share a unit, nor the
// lane that happened to generate a uniform show in the result.
//
// sample_back_kernel: blockIdx.x picks the sequences as decode_kernel does, blockIdx.y a group of NS samples.  The unit
// walks the blocks right to left; per block it re-runs the T forward steps from the checkpoint keeping the T alpha vectors
// in registers (the same Lane::fwd_site steps, folded factors and rescale schedule as the forward kernel), then traces
// each of its NS samples back through the block: per site the factors b, d, v of the sample's current state from an LDS
// table by state (vit_back_kernel's `fac`), a serial prefix sum inside the lane, an exclusive sum scan over the R lanes,
// and an integer sum of the per-lane counts.  The NS chains of a unit are independent and interleave.  The R lanes of a
// sequence generate the uniforms of different sites of the block and hand them round (ds_bpermute).
//
// Lanes per sequence: R = K / 4 (4 states per lane) for every (real, K), as the posterior-decoding sweep and Viterbi.
#include "psmc_kernels.hip"
#include "sweep_common.h"
#include "sample_common.h"

namespace phk {

// kernel id in the overrun record (KArgs::risk[1]; phk_underflow_risk names it)
constexpr int OVERRUN_SAMPLE_BACK = 9;

template <typename real, int K, int R, int T, int NRM, int NS>
__global__ __launch_bounds__(NT_MAX, (sweep_waves_per_simd<real>(T))) void sample_back_kernel(KArgs A, SArgs D) {
    using L = Lane<real, K, R>;
    using V = typename L::V;
    constexpr int SPL = L::SPL, NP = L::NP;
    constexpr int NU = (T + R - 1) / R;  // uniforms a lane generates per block and sample
    static_assert(T <= 16 && 16 % T == 0 && T % NRM == 0, "block / rescale schedule");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x;
    const int64_t nseq = A.B * A.S;
    const int64_t gid = (int64_t)blockIdx.x * (blockDim.x / R) + tid / R;
    const bool active = gid < nseq;
    const int64_t seq = active ? gid : nseq - 1;  // (idle groups repeat the last sequence: same bits, no stores)
    const int rank = tid & (R - 1);
    const int64_t ss = seq / A.B, bb = seq - ss * A.B;                // chunk-major order (see SeqMap)
    const uint64_t q = (uint64_t)((D.b0 + bb) * D.S_call + D.s0 + ss);  // ... the call's, for the outputs and the generator

    const int64_t Lt = A.Ltot, W = A.W;
    const int nblk = (int)((Lt + T - 1) / T);
    const int b_bot = (int)(W / T);  // the block of the first reported site

    L lane;
    V pi[NP];
    lane.load((const real*)A.params + bb * A.pstride_b + ss * A.pstride_s, rank, (real*)smem_raw + (size_t)tid * L::ETAB_STRIDE, pi);
    const real* pfb = prefold_block<real>(A, bb, ss);
    (void)lane.try_fold(pfb != nullptr ? pfb + rank * SPL : nullptr);  // the forward kernel's factors, to the bit
    SampleLane<real, K, R> sl;
    sl.init(lane, rank);
    // the group's factors b, d, v by state, behind the workgroup's emission tables: a draw reads those of ONE state
    real* fac = (real*)smem_raw + (size_t)blockDim.x * L::ETAB_STRIDE + (size_t)(tid - rank) * 3 * SPL;
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
        fac[rank * SPL + i] = L::get(lane.b, i);
        fac[K + rank * SPL + i] = L::get(lane.d, i);
        fac[2 * K + rank * SPL + i] = L::get(lane.v, i);
    }
    __syncthreads();

    const uint32_t* words = A.packed + checked_row(A, ss) * A.Lw;
    const int64_t ck_step = nseq * K;
    const real* ck = (const real*)A.ckpt + L::ck_lane(nseq, seq, rank);
    const int group_addr = 4 * ((tid & 63) - rank);  // ds_bpermute address of the group's first lane
    const uint32_t key0 = (uint32_t)D.seed, key1 = (uint32_t)(D.seed >> 32);
    const int64_t r0 = (int64_t)blockIdx.y * NS;

    uint8_t* prow[NS];  // indexed by site
    bool store[NS], aligned[NS];
    int cur[NS];  // state of sample s at the site drawn last (the same in every lane of the group)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        store[s] = active && r0 + s < D.n_samples;
        const int64_t r = r0 + s < D.n_samples ? r0 + s : D.n_samples - 1;
        prow[s] = D.paths + ((int64_t)q * D.n_samples + r) * D.path_stride - W;
        aligned[s] = (((uintptr_t)prow[s]) & 3) == 0;  // (block starts are multiples of T)
        cur[s] = 0;
    }
    bool ok = true;

    int budget = A.loop_budget[1];
    uint32_t wnext = words[((int64_t)(nblk - 1) * T) >> 4];
    real xnext[SPL];
#pragma unroll
    for (int i = 0; i < SPL; ++i) xnext[i] = ck_load(&ck[(int64_t)(nblk - 1) * ck_step + L::ck_elem(i, nseq)]);
    for (int blk = nblk - 1; blk >= b_bot; --blk) {
        if (__builtin_expect(--budget < 0, 0)) {
            report_overrun(A, OVERRUN_SAMPLE_BACK, seq, blk);
            return;
        }
        const int64_t t0 = (int64_t)blk * T;
        const int ns = Lt - t0 < T ? (int)(Lt - t0) : T;
        const uint32_t codes = wnext >> (2 * (int)(t0 & 15));  // (T divides 16: a block never straddles a word)
        V a[NP], al[T][NP];
#pragma unroll
        for (int h = 0; h < NP; ++h) a[h] = splat<real>(real(0));
#pragma unroll
        for (int i = 0; i < SPL; ++i) L::set(a, i, xnext[i]);
        if (blk > b_bot) {  // the next block's checkpoint and word, requested a block ahead
            wnext = words[(t0 - T) >> 4];
#pragma unroll
            for (int i = 0; i < SPL; ++i) xnext[i] = ck_load(&ck[(int64_t)(blk - 1) * ck_step + L::ck_elem(i, nseq)]);
        }
        // the uniforms of the block: lane `rank` generates those of sites t0 + rank + R m
        real ur[NS][NU];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int m = 0; m < NU; ++m) {
                uint32_t x0, x1;
                philox4x32_10((uint32_t)(t0 + rank + R * m), (uint32_t)(r0 + s), (uint32_t)q, (uint32_t)(q >> 32), key0, key1, x0, x1);
                uniform_of(x0, x1, ur[s][m]);
            }
        }
        // forward re-run from the checkpoint: al[i] = alpha after site t0 + i
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
        // trace, right to left: the state of every sample at site t0 + i given its state at the site after
        uint32_t out[NS][T / 4];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int w = 0; w < T / 4; ++w) out[s][w] = 0u;
        }
#pragma unroll
        for (int i = T - 1; i >= 0; --i) {
            const int64_t t = t0 + i;
            if (i < ns && t >= W) {
                const bool last = t == Lt - 1;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const real U = R > 1 ? lane_read(ur[s][i / R], group_addr + 4 * (i % R)) : ur[s][i / R];
                    cur[s] = sl.draw(lane, al[i], cur[s], last, U, fac, ok);
                    out[s][i >> 2] |= (uint32_t)cur[s] << (8 * (i & 3));
                }
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (!store[s]) continue;
            if (aligned[s] && t0 >= W && t0 + T <= Lt) {  // T / 4 dwords, one per lane (R < 4: several)
#pragma unroll
                for (int w = 0; w < T / 4; ++w)
                    if ((R <= 4 ? (w & (R - 1)) : w) == rank) *(uint32_t*)(prow[s] + t0 + 4 * w) = out[s][w];
            } else {
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    const int64_t t = t0 + i;
                    if (t >= W && t < Lt && (i & (R - 1)) == rank) prow[s][t] = (uint8_t)(out[s][i >> 2] >> (8 * (i & 3)));
                }
            }
        }
    }
    if (!ok && active && A.risk != nullptr) atomicOr(A.risk, FLAG_UNDERFLOW);
}

template <int T, int NRM, int NS>
static hipError_t sample_tnn(const KArgs& a, const SArgs& d, int nt, hipStream_t st) {
    using L = Lane<PHK_REAL, PHK_K, SWEEP_R>;
    const int64_t nseq = a.B * a.S;
    const int spb = nt / SWEEP_R;
    const int64_t groups = (d.n_samples + NS - 1) / NS;
    if (groups > 65535) return hipErrorInvalidValue;
    // emission tables + the factors by state (sample_back_kernel: fac)
    const size_t lds = ((size_t)L::ETAB_STRIDE + 3 * SWEEP_SPL) * nt * sizeof(PHK_REAL);
    const dim3 grid((unsigned)((nseq + spb - 1) / spb), (unsigned)groups), block(nt);
    hipLaunchKernelGGL((sample_back_kernel<PHK_REAL, PHK_K, SWEEP_R, T, NRM, NS>), grid, block, lds, st, a, d);
    return hipGetLastError();
}

template <int T, int NRM>
static hipError_t sample_tn(const KArgs& a, const SArgs& d, int nt, hipStream_t st) {
    constexpr int NS = sample_ns<PHK_REAL, PHK_K>();
    if (NS == 1 || d.n_samples == 1) return sample_tnn<T, NRM, 1>(a, d, nt, st);
    return sample_tnn<T, NRM, NS>(a, d, nt, st);
}

template <int T>
static hipError_t sample_t(int nrm, const KArgs& a, const SArgs& d, int nt, hipStream_t st) {
    if (nrm == 1) return sample_tn<T, 1>(a, d, nt, st);
    if (nrm == 2) return sample_tn<T, 2>(a, d, nt, st);
    if (nrm == 4) return sample_tn<T, 4>(a, d, nt, st);
    return hipErrorInvalidValue;
}

// T: the checkpoint spacing of the forward kernel that ran before; nrm: its rescale interval
hipError_t PHK_CAT(launch_sample_, PHK_SUFFIX)(int T, int nrm, const KArgs& a, const SArgs& d, int nt, hipStream_t st) {
    if (T == 8) return sample_t<8>(nrm, a, d, nt, st);
    if (T == 16) return sample_t<16>(nrm, a, d, nt, st);
    return hipErrorInvalidValue;
}

}  // namespace phk
