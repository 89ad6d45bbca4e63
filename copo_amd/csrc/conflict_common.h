// Shared declarations of the conflict log (conflict_kernels.hip) and its C entry points (capi_observers.hip).
#pragma once
#include "rowlog_common.h"

namespace copo {

constexpr int CONFLICT_PAIR_WORDS = 12;    // 32-bit words of a pair's memory: {first_rec, steps, d2min bits, min_off}, pose of a, pose of b
constexpr int CONFLICT_KIND_DONE = 1, CONFLICT_KIND_VANISHED = 2, CONFLICT_KIND_PARTED = 3, CONFLICT_KIND_FLUSH = 4;

// Arguments of one call (passed by value).  Device pointers; `state` and `env` are the simulator's own and are only read.
struct ConflictArgs {
    const float* state;            // [COPO_STATE_FIELDS][E][N]
    const int32_t* env;            // [E][4]
    int32_t E, N;
    int32_t r;                     // this record's number
    float r2_in, r2_out;           // radius^2, leave_radius^2, rounded once on the host
    const uint8_t* flags;          // this record's optional input [E][N], NULL = absent
    unsigned long long* open;      // [E][N] slot a: bit b > a: pair (a, b) has an open encounter
    int32_t* aid;                  // [E][N] the agent id of the previous record
    int32_t* episode;              // [E] the episode word of the previous record
    uint32_t* pairs;               // [E][N (N - 1) / 2][CONFLICT_PAIR_WORDS], pair (a, b) at a (2 N - a - 1) / 2 + b - a - 1
    // between the launches of one call
    unsigned long long* closing;   // [E][N] slot a: bit b: pair (a, b) closes in this call
    int32_t* n_closing;            // [E] closing pairs of the scene
    RowPoolArgs rows;              // the pool; a scene's closes are its closing pairs in ascending (slot a, slot b) order
};

hipError_t launch_conflict_record(const ConflictArgs& a, hipStream_t stream);
hipError_t launch_conflict_flush(const ConflictArgs& a, hipStream_t stream);

}  // namespace copo
