// Arguments of the Viterbi kernels (launch_viterbi.hip) beside KArgs; shared with the host side (phk_api.hip).
#pragma once
#include <stdint.h>

namespace phk {

struct VArgs {
    const int64_t* lens;  // [N] own length of every data row (W < len <= Ltot), or null: Ltot for all
    uint8_t* path;        // [B, S, path_stride]: states at sites W .. len - 1, then 255
    int64_t path_stride;  // >= Ltot - W
};

}  // namespace phk
