// Shared declarations of the trip log (trip_kernels.hip) and its C entry points (capi_observers.hip).
#pragma once
#include "rowlog_common.h"

namespace copo {

constexpr int TRIP_KIND_DONE = 1, TRIP_KIND_VANISHED = 2, TRIP_KIND_FLUSH = 3;
// per-slot memory: TRIP_MEM_WORDS planes of [E][N] 32-bit words, owned by the scene's wave
enum { TM_AID = 0, TM_FIRST, TM_ROUTE, TM_LCF, TM_PROG0, TM_PROG1, TM_STEPS, TM_SPEED_SUM, TM_SPEED_MAX, TM_STOPS, TM_REWARD, TM_MIN_GAP,
       TM_MIN_TTC, TRIP_MEM_WORDS };

// Arguments of one call (passed by value).  Device pointers; `state` and `env` are the simulator's own and are only read.
struct TripArgs {
    const float* state;            // [COPO_STATE_FIELDS][E][N]
    const int32_t* env;            // [E][4]
    int32_t E, N;
    int32_t r;                     // this record's number
    float stop_speed;
    // this record's optional inputs, [E][N] each, NULL = absent
    const uint8_t* flags;
    const float *rew, *gap, *ttc;
    unsigned long long* open;      // [E] bit n: a trip is open in slot n
    int32_t* episode;              // [E] the episode word the open trips of the scene were opened under
    uint32_t* mem;                 // [TRIP_MEM_WORDS][E][N]
    // between the launches of one call
    unsigned long long* closing;   // [E] bit n: slot n's trip closes in this call
    uint32_t* endw;                // [E][N] end flags | kind << 8 of the closing slots
    RowPoolArgs rows;              // the pool; a scene's closes are its closing slots in ascending order
};

hipError_t launch_trip_record(const TripArgs& a, hipStream_t stream);
hipError_t launch_trip_flush(const TripArgs& a, hipStream_t stream);

}  // namespace copo
