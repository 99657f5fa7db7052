// Arguments of the transition-posterior sweep (launch_trans.hip) beside KArgs; shared with the host side (phk_api.hip).
#pragma once
#include <stdint.h>

namespace phk {

struct TArgs {
    int64_t bin;          // scored sites per bin (>= 1)
    int64_t nbin;         // bins per sequence: ceil((Ltot - W) / bin)
    const int64_t* lens;  // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    void* arr;            // [B, S, nbin, 3, K] real: mean over the bin's own sites of (stay, up, down), or null
    void* chg;            // [B, S, nbin, 2] real: sum over the bin's own sites of (sum_k up, sum_k down), or null
};

}  // namespace phk
