// Shared declarations of the traffic gates (gate_kernels.hip) and their C entry points (capi.hip).
#pragma once
#include "grid_common.h"

namespace copo {

constexpr int GATE_MAX_GATES = 32;         // (a lane keeps the gates it crossed forward in one 32-bit word)
constexpr int GATE_MAX_SECTIONS = 64;
constexpr int GATE_MAX_GROUPS = GRID_MAX_GROUPS;
constexpr int GATE_MAX_BINS = 256;         // time bins of the series
constexpr int GATE_MAX_HIST = 64;          // headway bins, travel-time bins

// Offsets (in int64 words) of the accumulators inside the handle's one block, in the order copo_hip.h documents
struct GateLayout {
    int64_t count, speed_q, series, headway, sec_count, sec_sum, sec_hist, scene_records, alive, words;
};
inline GateLayout gate_layout(int64_t G, int64_t L, int64_t S, int64_t T, int64_t HB, int64_t TB) {
    GateLayout o;
    o.count = 0;
    o.speed_q = o.count + G * L * 2;
    o.series = o.speed_q + G * L * 2;
    o.headway = o.series + G * L * 2 * T;
    o.sec_count = o.headway + G * L * HB;
    o.sec_sum = o.sec_count + G * S;
    o.sec_hist = o.sec_sum + G * S;
    o.scene_records = o.sec_hist + G * S * TB;
    o.alive = o.scene_records + G;
    o.words = o.alive + G;
    return o;
}

// Arguments of one record (passed by value).  Device pointers; `state` and `env` are the simulator's own and are only read.
struct GateArgs {
    const float* state;            // [COPO_STATE_FIELDS][E][N]
    const int32_t* env;            // [E][4]
    int32_t E, N;
    int32_t L, S, G, T, HB, TB, tt_bin;
    int32_t r, tbin;               // this record's number and its bin of the series, min(r / bin_records, T - 1)
    const float4* gates;           // [L] {ax, ay, bx, by}
    const int2* sections;          // [S] {gate_in, gate_out}
    const int32_t* group;          // [E]
    // memory of the previous record, owned by the scene's wave
    uint32_t* mem_x;               // [E][N] raw bits
    uint32_t* mem_y;               // [E][N]
    int32_t* mem_aid;              // [E][N]
    int32_t* mem_episode;          // [E]
    unsigned long long* mem_valid; // [E] bit n: slot n was ALIVE
    int32_t* last_fwd;             // [E][L] record of the last forward crossing, -1: none
    int32_t* entry;                // [E][S][N] record of the slot's last forward crossing of gate_in, -1: none
    long long* acc;                // the accumulators (GateLayout)
    GateLayout at;
};

hipError_t launch_gate_record(const GateArgs& a, hipStream_t stream);

}  // namespace copo
