// Arguments of the posterior-decoding sweep (launch_decode.hip) beside KArgs; shared with the host side (phk_api.hip).
#pragma once
#include <stdint.h>

namespace phk {

struct DArgs {
    int64_t bin;           // scored sites per bin (>= 1)
    int64_t nbin;          // bins per sequence: ceil((Ltot - W) / bin)
    const double* values;  // [B|1, K] value of every state (row stride vstride_b; 0 = shared), or null (no mean)
    int64_t vstride_b;
    void* mean;            // [B, S, nbin] real: mean over the bin of sum_k values_k gamma_t(k), or null
    void* marg;            // [B, S, nbin, K] real: mean over the bin of gamma_t, or null
};

}  // namespace phk
