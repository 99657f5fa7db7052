// Arguments of the pair-count sweep (launch_pairs.hip) beside KArgs; shared with the host side (phk_api.hip).
#pragma once
#include <stdint.h>

namespace phk {

struct PArgs {
    const int64_t* lens;  // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    double* part;         // workspace [max(units, 1), B S of the launch, K, K]: every unit's own sum of raw outer products
    double* counts;       // [B, S, K, K] of the launch, the caller's order: expected moves from state i (first) to state j
    int row0;             // first origin state of the row tile this launch accumulates (set by the launcher; 0 on the matrix path)
};

}  // namespace phk
