// Shared declarations of the interaction meter (interact_kernels.hip) and its C entry points (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace copo {

// per-slot accumulator, 32-bit words [INTERACT_ACC_WORDS][E][N] (steps == 0: the slot holds no open agent)
enum : int {
    IA_AID = 0, IA_EPISODE, IA_STEPS, IA_MIN_GAP, IA_MIN_TTC, IA_TET_STEPS, IA_NEAR_EVENTS, IA_IN_NEAR, IA_BRAKE_EVENTS, IA_LAST_SPEED,
    INTERACT_ACC_WORDS
};
// scene totals: counts [E][INTERACT_COUNTS] int64, sums [E][INTERACT_SUMS] fp64
enum : int { IC_AGENTS = 0, IC_STEPS, IC_TET_STEPS, IC_NEAR_EVENTS, IC_BRAKE_EVENTS, IC_FINITE_TTC, INTERACT_COUNTS };
enum : int { IS_MIN_GAP = 0, IS_MIN_TTC, IS_TIT, INTERACT_SUMS };

// Arguments of one record / totals launch (passed by value).  Device pointers; `state` / `env` are the simulator's own.
struct InteractArgs {
    const float* state;            // [COPO_STATE_FIELDS][E][N]
    const int32_t* env;            // [E][4]
    int32_t E, N;
    float hl, hw, dt;
    float horizon_s, ttc_crit_s, gap_near_m, brake_mps2;
    int32_t* acc;                  // [INTERACT_ACC_WORDS][E][N]
    double* tit;                   // [E][N] time-integrated TTC of the open agent (s^2)
    long long* counts;             // [E][INTERACT_COUNTS]
    double* sums;                  // [E][INTERACT_SUMS]
};

// one workgroup per scene: per-slot minimum gap / TTC of the current state into gap / ttc ([E][N], either may be NULL), accumulators updated
hipError_t launch_interact_record(const InteractArgs& a, float* gap, float* ttc, hipStream_t stream);
// copy the scene totals out; flush_open: plus, in slot order, the agents still open (the accumulators are left as they are)
hipError_t launch_interact_totals(const InteractArgs& a, long long* counts_out, double* sums_out, int flush_open, hipStream_t stream);

}  // namespace copo
