// Shared declarations of the encroachment log (encroach_kernels.hip) and its C entry points (capi_observers.hip).
#pragma once
#include "grid_common.h"
#include "rowlog_common.h"

namespace copo {

constexpr int PET_MAX_WINDOW = 4096;       // records a stamp stays valid for, and bins of a histogram
constexpr int PET_TYPES = 3;               // following, crossing, opposing
constexpr int PET_FOLLOW_Q = 21, PET_OPPOSE_Q = 107;      // of 256 heading steps per turn: 30 and 150 degrees, quantised

// Arguments of one call (passed by value).  Device pointers; `state` and `env` are the simulator's own and are only read.
struct PetArgs {
    const float* state;            // [COPO_STATE_FIELDS][E][N]
    const int32_t* env;            // [E][4]
    int32_t E, N;
    int32_t r;                     // this record's number
    float hl, hw;
    GridSpec grid;
    int32_t window, critical_records;
    SceneGroups groups;
    unsigned long long* stamps;     // [E][H][W] stamps: rec + 1 << 32 | (aid & 0xffff) << 16 | hq << 8 | slot, 0 = empty
    int32_t* aid;                  // [E][N] the agent id of the previous record
    unsigned long long* met;       // [E][N] slot b: bit a: the encounter of b with the agent in slot a has its row
    int32_t* episode;              // [E] the episode word of the previous record
    int32_t* epoch;                // [E] the record of the scene's last episode change: stamps with a record field <= epoch are void
    long long* hist;               // [G][PET_TYPES][window]
    long long* critical;           // [G][H][W]
    // between the launches of one call
    unsigned long long* fresh;     // [E][N] slot b: bit a: the encounter commits its row in this call
    int32_t* n_fresh;              // [E] rows of the scene in this call
    RowPoolArgs rows;              // the pool; a scene's rows are its new encounters in ascending (slot b, slot a) order
};

hipError_t launch_pet_record(const PetArgs& a, hipStream_t stream);
// epoch[e] = r for every scene: every stamp written so far is void
hipError_t launch_pet_forget(int32_t* epoch, int E, int32_t r, hipStream_t stream);

}  // namespace copo
