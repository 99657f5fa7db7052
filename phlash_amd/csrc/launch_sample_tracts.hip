// Sampled tract spectra: the paths of posterior path sampling (launch_sample.hip) reduced inside the traceback, never stored.
// One translation unit per (real, K), compiled with -DPHK_REAL=float|double -DPHK_K=<K> -DPHK_SUFFIX=<tag> (see the
// Makefile: launch_sample_tracts_<real>_<K>.o).  The definition is in include/phlash_hip.h, phk_sample_tracts.
//
// sample_tracts_kernel is sample_back_kernel with the path words and stores taken out: the same grid (blockIdx.x picks the
// sequences, blockIdx.y a group of NS samples), the same forward re-run from the alpha checkpoints, the same uniforms (Philox
// counters and hand-round) and the same SampleLane::draw in the same order, so sample r of sequence q is the path
// phk_sample_paths stores for (seed, q, r).  What a sample carries instead of its bytes is scalar per group -- the state drawn
// is the same in every lane of the group --:
//     inb   per block, one bit per site: the state drawn is inside the set (in place of the path words)
//     chb   per block, one bit per site: the state drawn differs from the one at the site after
//     run   length of the run of own reported sites inside the set that ends, to the right, just above the block being traced
//     chg   column 3 of the stats row, the changes of state
// A site costs a shift, an and and a shift-or into inb and an xor, a min and a shift-or into chb beside its draw.  The row's
// own length enters once per block, as a mask over the bits of both words.  Behind the trace of a block, tract_block reads the
// runs of ones off inb with count-leading-zeros, highest site first (the walk goes right to left): a run that ends inside the block
// is a tract closed; one that reaches bit 0 stays open in `run`.  A site the block does not report (before W, past the row's
// end) has bit 0, which closes a tract at W as at any other site outside the set; where W starts a block, the run left
// open behind the last block is closed there.  tract_block is a loop of at most T / 2 + 1 turns that is NOT unrolled: one
// copy of the closing code per sample of the unit, not one per site.
// Closing is rare beside sites and is the only place that touches memory: the group's first lane adds the tract to columns
// 0 - 2 and to the histogram column of its own stats row (a row has one writer: integer adds and a maximum on zeroed memory,
// the same in any order) and, where cover is wanted and the tract is long enough, the tract's partial overlaps to its first
// and last bin of cover and +1 / -1 to the difference row at the first bin it covers whole and at its last bin: four more
// integer atomics per tract, no loop over its length.  The units of different sample groups add to the same (sequence,
// bin); integer adds commute, so cover does not depend on their order.  cover_finalize_kernel (phk_api.hip) adds bin x the
// prefix sum of the difference row.
#include "psmc_kernels.hip"
#include "sweep_common.h"
#include "sample_common.h"

namespace phk {

// kernel id in the overrun record (KArgs::risk[1]; phk_underflow_risk names it)
constexpr int OVERRUN_SAMPLE_TRACTS = 22;

// Samples per unit where a call asks for more than one, chosen like sample_ns from the compiler's resource report: the largest
// of {1, 2, 4} at which no kernel of the unit has scratch or AGPR copies ("Sampled tract spectra").  The
// kernel holds its own arguments beside the traceback's, and float64 with K >= 16 has no room for a second sample at T = 16.
template <typename real, int K>
constexpr int sample_tracts_ns() { return sizeof(real) == 8 ? (K <= 8 ? 2 : 1) : (K == 4 ? 2 : 4); }

// The tract of n sites from reported site a (site W + a) on, closed: columns 0 - 2 and the histogram column of the sample's
// stats row and, for a tract of min_len sites or more, its sites per bin.  One lane of the group calls it.
__device__ __forceinline__ void tract_emit(const XArgs& D, int32_t* srow, int32_t* crow, int32_t* drow, int a, int n) {
    int cls = 0;
    if (D.ncol > 5) {
#pragma unroll
        for (int e = 0; e < TRACT_MAX_EDGES; ++e) cls += D.edges[e] <= n ? 1 : 0;
    }
    atomicAdd(srow, n);
    atomicAdd(srow + 1, 1);
    atomicMax(srow + 2, n);
    atomicAdd(srow + 4 + cls, 1);
    if (crow != nullptr && n >= D.min_len) {
        const uint32_t bin = (uint32_t)D.bin;
        const int g0 = (int)((uint32_t)a / bin), g1 = (int)((uint32_t)(a + n - 1) / bin);
        if (g0 == g1) {
            atomicAdd(crow + g0, n);
        } else {
            atomicAdd(crow + g0, (g0 + 1) * D.bin - a);
            atomicAdd(crow + g1, a + n - g1 * D.bin);
            if (g1 > g0 + 1) {
                atomicAdd(drow + g0 + 1, 1);
                atomicAdd(drow + g1, -1);
            }
        }
    }
}

// The tracts of one sample that end inside a block of T sites.  inb: bit i set = site i of the block is inside; run: the run of
// inside sites just above the block, on return the run that reaches the block's first site; a0: reported index of the block's
// first site (negative in the block that holds W: its bits before W are 0 and no tract starts there).
template <int T>
__device__ __forceinline__ void tract_block(const XArgs& D, bool emit, int32_t* srow, int32_t* crow, int32_t* drow, uint32_t inb, int a0,
                                            int& run) {
    constexpr uint32_t ALL = T == 32 ? 0xffffffffu : (1u << T) - 1u;
    if (inb == ALL) {  // (the common block inside a long tract)
        run += T;
        return;
    }
    if (inb == 0u && run == 0) return;  // (and the common block outside every tract)
    int p = T;  // bits [0, p) are still to be read
#pragma unroll 1
    for (int it = 0; it < T / 2 + 1; ++it) {
        const uint32_t below = p >= 32 ? 0xffffffffu : (1u << p) - 1u;
        const uint32_t out = ~inb & below;
        if (out == 0u) {  // ones down to bit 0: the run stays open
            run += p;
            break;
        }
        const int h = 31 - __clz(out);  // the highest site outside the set
        run += p - 1 - h;
        if (run > 0 && emit) tract_emit(D, srow, crow, drow, a0 + h + 1, run);
        run = 0;
        const uint32_t rest = inb & ((1u << h) - 1u);
        if (rest == 0u) break;
        p = 32 - __clz(rest);  // just above the next site inside
    }
}

template <typename real, int K, int R, int T, int NRM, int NS>
__global__ __launch_bounds__(NT_MAX, (sweep_waves_per_simd<real>(T))) void sample_tracts_kernel(KArgs A, XArgs D) {
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

    const int64_t row = checked_row(A, ss);
    const uint32_t* words = A.packed + row * A.Lw;
    const int64_t len = sweep_len(A, D, row);
    const int64_t ck_step = nseq * K;
    const real* ck = (const real*)A.ckpt + L::ck_lane(nseq, seq, rank);
    const int group_addr = 4 * ((tid & 63) - rank);  // ds_bpermute address of the group's first lane
    const uint32_t key0 = (uint32_t)D.seed, key1 = (uint32_t)(D.seed >> 32);
    const int64_t r0 = (int64_t)blockIdx.y * NS;
    const uint64_t mask = D.masks[bb * D.mask_stride];

    // the stats row of the unit's first sample; one lane of the group owns the writes, and none where the sample does not exist
    int32_t* const srow0 = D.stats + ((int64_t)q * D.n_samples + r0) * D.ncol;
    const int nwr = active && rank == 0 ? (int)(D.n_samples - r0 < NS ? D.n_samples - r0 : NS) : 0;
    int cur[NS];  // state of sample s at the site drawn last (the same in every lane of the group)
    int run[NS], chg[NS];
    using mask_t = typename std::conditional<(K <= 32), uint32_t, uint64_t>::type;
    const mask_t mk = (mask_t)mask;
#pragma unroll
    for (int s = 0; s < NS; ++s) cur[s] = run[s] = chg[s] = 0;
    int32_t* const crow = D.cover != nullptr ? D.cover + (int64_t)q * D.nbin : nullptr;
    int32_t* const drow = D.cover != nullptr ? D.diff + seq * D.nbin : nullptr;
    bool ok = true;

    int budget = A.loop_budget[1];
    uint32_t wnext = words[((int64_t)(nblk - 1) * T) >> 4];
    real xnext[SPL];
#pragma unroll
    for (int i = 0; i < SPL; ++i) xnext[i] = ck_load(&ck[(int64_t)(nblk - 1) * ck_step + L::ck_elem(i, nseq)]);
    for (int blk = nblk - 1; blk >= b_bot; --blk) {
        if (__builtin_expect(--budget < 0, 0)) {
            report_overrun(A, OVERRUN_SAMPLE_TRACTS, seq, blk);
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
        // trace, right to left: the state of every sample at site t0 + i given its state at the site after, and whether it is
        // inside the set.  A site at or past the row's own length is drawn and counts for nothing.
        uint32_t inb[NS], chb[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) inb[s] = chb[s] = 0u;
#pragma unroll
        for (int i = T - 1; i >= 0; --i) {
            const int64_t t = t0 + i;
            if (i < ns && t >= W) {
                const bool last = t == Lt - 1;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const real U = R > 1 ? lane_read(ur[s][i / R], group_addr + 4 * (i % R)) : ur[s][i / R];
                    const int z = sl.draw(lane, al[i], cur[s], last, U, fac, ok);
                    const uint32_t moved = (uint32_t)(z ^ cur[s]);  // (at the row's last site cur is no state: masked below)
                    chb[s] |= (moved < 1u ? moved : 1u) << i;
                    cur[s] = z;
                    inb[s] |= ((uint32_t)(mk >> z) & 1u) << i;
                }
            }
        }
        // the row's own sites of the block, and those whose right neighbour is one of the row's own as well
        // (the right neighbour of the block's last site is the first site of the block above)
        const int64_t left = len - t0;
        const uint32_t ownb = left >= T ? (1u << T) - 1u : (left > 0 ? (1u << (int)left) - 1u : 0u);
        const uint32_t pairb = left > T ? (1u << T) - 1u : (left > 1 ? (1u << (int)(left - 1)) - 1u : 0u);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            chg[s] += __popc(chb[s] & pairb);
            tract_block<T>(D, s < nwr, srow0 + s * D.ncol, crow, drow, inb[s] & ownb, (int)(t0 - W), run[s]);
        }
    }
    // a tract that reaches the first reported site ends there: counted at its visible length
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s < nwr) {
            if (run[s] > 0) tract_emit(D, srow0 + s * D.ncol, crow, drow, 0, run[s]);
            srow0[s * D.ncol + 3] = chg[s];
        }
    }
    if (!ok && active && A.risk != nullptr) atomicOr(A.risk, FLAG_UNDERFLOW);
}

template <int T, int NRM, int NS>
static hipError_t sample_tracts_tnn(const KArgs& a, const XArgs& d, int nt, hipStream_t st) {
    using L = Lane<PHK_REAL, PHK_K, SWEEP_R>;
    const int64_t nseq = a.B * a.S;
    const int spb = nt / SWEEP_R;
    const int64_t groups = (d.n_samples + NS - 1) / NS;
    if (groups > 65535) return hipErrorInvalidValue;
    // emission tables + the factors by state (sample_tracts_kernel: fac)
    const size_t lds = ((size_t)L::ETAB_STRIDE + 3 * SWEEP_SPL) * nt * sizeof(PHK_REAL);
    const dim3 grid((unsigned)((nseq + spb - 1) / spb), (unsigned)groups), block(nt);
    hipLaunchKernelGGL((sample_tracts_kernel<PHK_REAL, PHK_K, SWEEP_R, T, NRM, NS>), grid, block, lds, st, a, d);
    return hipGetLastError();
}

template <int T, int NRM>
static hipError_t sample_tracts_tn(const KArgs& a, const XArgs& d, int nt, hipStream_t st) {
    constexpr int NS = sample_tracts_ns<PHK_REAL, PHK_K>();
    if (NS == 1 || d.n_samples == 1) return sample_tracts_tnn<T, NRM, 1>(a, d, nt, st);
    return sample_tracts_tnn<T, NRM, NS>(a, d, nt, st);
}

template <int T>
static hipError_t sample_tracts_t(int nrm, const KArgs& a, const XArgs& d, int nt, hipStream_t st) {
    if (nrm == 1) return sample_tracts_tn<T, 1>(a, d, nt, st);
    if (nrm == 2) return sample_tracts_tn<T, 2>(a, d, nt, st);
    if (nrm == 4) return sample_tracts_tn<T, 4>(a, d, nt, st);
    return hipErrorInvalidValue;
}

// T: the checkpoint spacing of the forward kernel that ran before; nrm: its rescale interval
hipError_t PHK_CAT(launch_sample_tracts_, PHK_SUFFIX)(int T, int nrm, const KArgs& a, const XArgs& d, int nt, hipStream_t st) {
    if (T == 8) return sample_tracts_t<8>(nrm, a, d, nt, st);
    if (T == 16) return sample_tracts_t<16>(nrm, a, d, nt, st);
    return hipErrorInvalidValue;
}

}  // namespace phk
