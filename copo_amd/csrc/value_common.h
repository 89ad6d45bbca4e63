// The value pass of a seated bank (copo_value_obs_seats_f32): the argument struct and the launcher that
// value_kernels.hip defines and capi_value.hip checks arguments for.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/copo_hip.h"

namespace copo {

struct ValueSeatArgs {
    copo_ppo_cfg c;
    const float* theta;       // [n_members][member_stride]
    const float* theta_t;     // the transposed mirror, same strides
    int64_t member_stride;
    const int64_t* rows;      // [n_members][cap]
    const int32_t* counts;    // [n_members]
    int64_t cap, n_out;
    const float* src;         // [n_out][val[h].in_dim]: cc_src, or obs_src where there is none
    float* values;            // [n_out][n_value_heads]
    int32_t n_members;
};

// dynamic LDS of a workgroup, bytes, for the widest value net of the configuration; 0 for a hidden width without an instantiation
size_t value_seats_lds_bytes(const copo_ppo_cfg& c);
// grid ceil(cap / 16) x n_members x n_value_heads; hipErrorInvalidValue for a hidden width outside {64, 128, 256, 512}
hipError_t launch_value_seats(const ValueSeatArgs& a, hipStream_t stream);

}  // namespace copo
