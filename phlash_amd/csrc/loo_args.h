// Arguments of the leave-one-out predictive sweep (launch_loo.hip) beside KArgs; shared with the host side (phk_api.hip).
#pragma once
#include <stdint.h>

namespace phk {

struct LArgs {
    int64_t bin;          // scored sites per bin (>= 1)
    int64_t nbin;         // bins per sequence: ceil((Ltot - W) / bin)
    const int64_t* lens;  // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    void* track;          // [B, S, nbin, 3] real: sums over the bin's own sites of (phet at observed sites, phet at missing
                          // sites, log score)
};

}  // namespace phk
