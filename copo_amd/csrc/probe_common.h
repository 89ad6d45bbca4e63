// Linear probes (include/copo_hip.h): the launches of probe_kernels.hip that capi_probe.hip calls, and the geometry
// both sides agree on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/copo_hip.h"
#include "gram_common.h"      // GRAM_TILE: a workgroup owns a 64 x 64 tile of one G[f, b]

namespace copo {

constexpr int PROBE_PANEL = COPO_PROBE_PANEL;                 // the columns of a target row: Q targets, zeros, the ones column
constexpr int PROBE_MAX_TILES = COPO_PROBE_MAX_WIDTH / GRAM_TILE;

struct ProbeTargetArgs {
    const float* obs;         // [n_out][O]
    const float* trig;        // [num_lasers][2]: cos, sin of the beam's angle
    const uint8_t* flags;     // [n_out]
    const float* reward;      // [n_out]
    const int64_t* rows;      // [cap]
    const int32_t* count;     // [1]
    int64_t cap, n_out;
    int32_t O, Op, lidar_lo, num_lasers;
    float* targets;           // [cap][16]
    float* xobs;              // [cap][Op]
};

struct ProbeArgs {
    const float* x;               // the feature workspace, x_floats floats
    const int64_t* block_base;    // [B]: offset of block b's position 0, in floats
    const float* targets;         // [cap][16]
    const int64_t* rows;          // [cap]
    const int32_t* count;         // [1]
    const uint8_t* flags;         // [n_out]
    const int32_t* seat;          // [n_out]
    const uint8_t* fold;          // [n_out / slots]
    int64_t x_floats, pos_stride, cap, n_out;
    int32_t B, D, slots, rows_of, R;
    double* G;                    // [R][2][B][D][D]
    double* C;                    // [R][2][B][D][16]
    double* T;                    // [R][2][16][16]
};

hipError_t launch_probe_targets(const ProbeTargetArgs& a, hipStream_t stream);
hipError_t launch_probe_accumulate(const ProbeArgs& a, hipStream_t stream);

}  // namespace copo
