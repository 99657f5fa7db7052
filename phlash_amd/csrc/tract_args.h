// Arguments of the tract-posterior sweep (launch_tract.hip) beside KArgs; shared with the host side (phk_api.hip).
#pragma once
#include <stdint.h>

namespace phk {

struct QArgs {
    int64_t bin;            // scored sites per bin (>= 1)
    int64_t nbin;           // bins per sequence: ceil((Ltot - W) / bin)
    const int64_t* lens;    // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    const double* weights;  // [B, K] (row stride wstride_b) or [K] (wstride_b = 0): the per-state weight m in [0, 1]
    int64_t wstride_b;
    void* tract;            // [B, S, nbin] real: E[prod of m(z_t) over the bin's own sites | o]
};

}  // namespace phk
