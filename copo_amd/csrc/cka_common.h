// Representation similarity (include/copo_hip.h): the launches of cka_kernels.hip that capi_cka.hip calls, and the
// geometry both sides agree on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/copo_hip.h"
#include "gram_common.h"      // GRAM_TILE: a workgroup owns a 64 x 64 tile of one S[a, b, l]

namespace copo {

struct CkaArgs {
    const float* hidden;      // [n_members][cap][2][H]
    const int32_t* panel;     // [M]
    const int64_t* rows;      // [cap]
    const int32_t* count;     // [1]
    const uint8_t* flags;     // [n_out]
    const int32_t* seat;      // [n_out]
    int64_t cap, n_out;
    int32_t H, M, rows_of, R, K;      // K: members the workspace holds (a panel entry outside [0, K) adds nothing)
    double* S;                // [R][P][2][H][H]
    double* s;                // [R][M][2][H]
    int64_t* n;               // [R]
};

hipError_t launch_cka_accumulate(const CkaArgs& a, hipStream_t stream);
hipError_t launch_cka_finish(const double* S, const double* s, const int64_t* n, int32_t M, int32_t H, int32_t R, double* hsic, int64_t* n_out,
                             double* mean, double* var, hipStream_t stream);

}  // namespace copo
