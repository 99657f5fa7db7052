// Arguments of the path-sampling traceback (launch_sample.hip) beside KArgs; shared with the host side (phk_api.hip).
#pragma once
#include <stdint.h>

namespace phk {

struct SArgs {
    uint8_t* paths;       // [B, S, n_samples, path_stride] of the CALL: states at sites W .. Ltot - 1
    int64_t path_stride;  // >= Ltot - W
    int64_t n_samples;    // samples per sequence (>= 1)
    uint64_t seed;        // Philox key
    int64_t b0, s0;       // position of the slab in the call, and ...
    int64_t S_call;       // ... the call's S: q = (b0 + b) * S_call + (s0 + s) numbers the sequences of the call
};

}  // namespace phk
