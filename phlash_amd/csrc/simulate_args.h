// Arguments of the posterior predictive simulator (launch_simulate.hip); shared with the host side (phk_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace phk {

constexpr int SIM_MAXK = 64;  // hidden states: any K in [2, SIM_MAXK], no padding
constexpr int SIM_T = 16;     // sites per block of the site loop (one 16-byte store per lane and output)
constexpr int SIM_NT = 64;    // threads per workgroup: one wave (the run histogram in LDS is sized by it)

struct SimArgs {
    int K;
    const double* params;          // [B, S or 1, 7, K], element strides
    int64_t pstride_b, pstride_s;  // pstride_s = 0: one block per particle
    int64_t B, S, n_rep, L;
    uint32_t key0, key1;           // Philox key (seed lo, hi)
    int64_t seq0;                  // q = seq0 + b S + s
    const int8_t* mask;            // [S, mask_stride] or NULL
    int64_t mask_stride;
    int mask_vec;                  // mask base and stride are multiples of 16: whole blocks are read 16 bytes at a time
    int8_t* obs;                   // [B, S, n_rep, row_stride] or NULL
    uint8_t* paths;                // likewise
    int64_t row_stride;
    int64_t bin, nbin;
    int32_t* het;                  // [B, S, n_rep, nbin] or NULL
    int32_t* runs;                 // [B, S, n_rep, 32] or NULL
    int32_t* flags;
    int per_row;                   // 1: a workgroup's sequences share (b, s); 0: they share b (pstride_s = 0)
    int64_t per_block;             // sequences per parameter block: n_rep or S n_rep
    int64_t chunks;                // workgroups per parameter block
    int64_t nfull;                 // whole SIM_T-site blocks of a row: the site loop's trip count
};

hipError_t launch_simulate(const SimArgs& a, hipStream_t st);

}  // namespace phk
