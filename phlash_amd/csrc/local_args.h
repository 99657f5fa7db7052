// Arguments of the local likelihood-ratio sweep (launch_local.hip) beside KArgs; shared with the host side (phk_api.hip).
#pragma once
#include <stdint.h>

namespace phk {

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

}  // namespace phk
