// Shared by the fault kernels (fault_kernels.hip) and their C entry points (capi.hip): the random streams, the layout of a level row
// and the launch declarations.  The rules are DESIGN.md section 8l; tests/fault_numpy.py restates them as python loops.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace copo {

// Streams of hash_rng (sim_math.h) that the simulator does not use (sim_common.h: 1, 2, 3, 4 and 16).  Every draw is
// hash_rng(fault_seed, row, tick[row], c, stream): c = the beam for the three LiDAR streams, the action component for ACT_A / ACT_B, 0
// for STICKY.
enum : uint32_t {
    RNG_FAULT_DROP = 32,       // Bernoulli: the beam reads dropout_value
    RNG_FAULT_LIDAR_A = 33,    // the two hashes behind a beam's z
    RNG_FAULT_LIDAR_B = 34,
    RNG_FAULT_STICKY = 35,     // Bernoulli: the action repeats the previous one
    RNG_FAULT_ACT_A = 36,      // the two hashes behind an action component's z
    RNG_FAULT_ACT_B = 37,
};

// words of a level row (COPO_FAULT_LEVEL_WORDS of them; 5..7 are zero)
enum : int { FAULT_W_LIDAR_SIGMA = 0, FAULT_W_DROPOUT_THR = 1, FAULT_W_DROPOUT_VALUE = 2, FAULT_W_ACT_SIGMA = 3, FAULT_W_STICKY_THR = 4 };

constexpr float kFaultZOffset = 131070.0f;             // 4 * 65535 / 2: the mean of the sum of four 16-bit halves
constexpr float kFaultZScale = 0x1.bb67aep-16f;        // (float)(sqrt(3) / 65536), bits 0x37ddb3d7: the sum's variance is (2^32 - 1) / 3

hipError_t launch_fault_obs(const float* obs, float* obs_seen, int32_t E, int32_t N, int32_t O, int32_t col_lo, int32_t col_hi,
                            const int32_t* seat, const int32_t* group, int32_t K, int32_t G, const int32_t* level_of,
                            const uint32_t* levels, int32_t L, const int32_t* tick, uint64_t fault_seed, hipStream_t stream);
hipError_t launch_fault_act(float* act, float* prev, const uint8_t* flags_prev, int32_t E, int32_t N, const int32_t* seat,
                            const int32_t* group, int32_t K, int32_t G, const int32_t* level_of, const uint32_t* levels, int32_t L,
                            int32_t* tick, uint64_t fault_seed, hipStream_t stream);

}  // namespace copo
