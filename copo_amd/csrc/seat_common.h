// Shared declaration of the seat tally (seat_kernels.hip) and its C entry point (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace copo {

// cross-play: one step's flags / rewards folded per (scene group, bank member) into out[G][K][COPO_SEAT_WORDS] (one launch)
hipError_t launch_seat_tally(const uint8_t* flags, const float* rew, const int32_t* seat, const int32_t* group, int32_t E, int32_t N,
                             int32_t K, int32_t G, int64_t* out, hipStream_t stream);

// certified bounds of one step folded per (scene group, bank member) into out[G][K][COPO_CERT_TALLY_WORDS] (one launch)
hipError_t launch_certify_tally(const uint8_t* flags, const float* bounds, const int32_t* seat, const int32_t* group, const int32_t* level_of,
                                const float* levels, int32_t E, int32_t N, int32_t K, int32_t G, int32_t L, int64_t* out, hipStream_t stream);

// one step's jury verdicts folded per (scene group, driving member, judging member) into out[G][K][K][COPO_JURY_WORDS] (one launch)
hipError_t launch_jury_tally(const uint8_t* flags, const float* dist, const float* verdict, const int32_t* seat, const int32_t* group,
                             const int32_t* judges, int32_t E, int32_t N, int32_t K, int32_t G, float delta_steer, float delta_throttle,
                             int64_t* out, hipStream_t stream);

}  // namespace copo
