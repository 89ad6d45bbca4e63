// Shared declarations of the traffic field maps (field_kernels.hip) and their C entry points (capi_observers.hip).
#pragma once
#include "grid_common.h"

namespace copo {

constexpr int FIELD_LAYERS = 10;           // int64 [G][FIELD_LAYERS][H][W]
enum : int { FL_OCCUPANCY = 0, FL_WRECK, FL_VISITS, FL_SPEED_Q, FL_VX_Q, FL_VY_Q, FL_CRASH, FL_OUT, FL_ARRIVE, FL_CRITICAL };
constexpr int FIELD_MAX_SIDE = GRID_MAX_SIDE, FIELD_MAX_GROUPS = GRID_MAX_GROUPS;
constexpr int FIELD_TILE = 32;             // cells per tile side: one workgroup sums a FIELD_TILE x FIELD_TILE tile on chip
constexpr int FIELD_MASK_WORDS = (FIELD_MAX_SIDE / FIELD_TILE) * (FIELD_MAX_SIDE / FIELD_TILE) / 32;      // tile bits per scene block

// Arguments of one record (passed by value).  Device pointers; `state` is the simulator's own and is only read.
struct FieldArgs {
    const float* state;            // [COPO_STATE_FIELDS][E][N]
    int32_t E, N;
    float hl, hw;
    GridSpec grid;
    int32_t block;                 // scenes per workgroup of the tile pass (a multiple of 4)
    float ttc_below;               // 0: the critical layer is off
    SceneGroups groups;
    const uint8_t* flags;          // [E][N] or NULL
    const float* ttc;              // [E][N] or NULL
    int32_t* last;                 // [E][N] centre cell iy * W + ix of the slot in the previous record when it was ALIVE inside the grid, else -1
    uint32_t* mask;                // [ceil(E / block)][FIELD_MASK_WORDS] tiles the bodies of a scene block can reach (zero before the launch)
    long long* maps;               // [G][FIELD_LAYERS][H][W]
    long long* scene_records;      // [G]
};

// events of this record at the remembered cells, then the memory refreshed from the current state; accumulate: also the tile bits of
// every scene block (one launch)
hipError_t launch_field_events(const FieldArgs& a, int accumulate, hipStream_t stream);
// occupancy, wreck, visits, speed, flow and critical layers of the current state (one launch; reads the tile bits of launch_field_events)
hipError_t launch_field_tiles(const FieldArgs& a, hipStream_t stream);

}  // namespace copo
