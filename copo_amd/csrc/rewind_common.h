// Shared declarations of scene rewind (rewind_kernels.hip) and its C entry points (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace copo {

constexpr int REWIND_MAX_DEPTH = 64;       // snapshots per scene ring
constexpr int REWIND_ENV_WORDS = 4;        // per snapshot and scene: the simulator's env words {t_env, episode, next_aid, started}
constexpr int REWIND_TALLY = 8;            // per branch: the RT_* words
enum : int { RT_STEPS = 0, RT_ACTED, RT_ARRIVE, RT_CRASH, RT_OUT, RT_MAXSTEP, RT_WATCH_FLAGS, RT_WATCH_STEP };

// Arguments of the record launch (passed by value).  Device pointers; `state` / `env` are the source simulator's own and are only read.
struct RewindArgs {
    const float* state;            // [COPO_STATE_FIELDS][E][N]
    const int32_t* env;            // [E][4]
    int32_t E, N, depth;
    uint32_t* ring;                // [E][depth][COPO_STATE_FIELDS][N]
    int32_t* ring_env;             // [E][depth][REWIND_ENV_WORDS]
};

// Arguments of the fork launch (passed by value).  `n_records` / `stride` select the snapshot (the count lives on the host).
struct RewindForkArgs {
    const uint32_t* ring;          // source ring, [E][depth][COPO_STATE_FIELDS][N]
    const int32_t* ring_env;       // [E][depth][REWIND_ENV_WORDS]
    const uint64_t* src_seeds;     // [E] the source simulator's seeds (only read)
    int32_t E, N, depth, stride, n_records;
    float* state;                  // target: [COPO_STATE_FIELDS][TE][N]
    int32_t* env;                  // [TE][4]
    uint64_t* seeds;               // [TE]
    int32_t TE, first, S;
    const int32_t* scene;          // [S]
    const int32_t* rec;            // [S]
    const float* lcf;              // [S] or NULL
    const uint64_t* new_seeds;     // [S] or NULL
    const int32_t* watch_slot;     // [S] or NULL
    int32_t* status;               // [S]
    int32_t* watch_aid;            // [S] or NULL
};

// the current state of every scene into ring place `place` (one launch)
hipError_t launch_rewind_record(const RewindArgs& a, int place, hipStream_t stream);
// scene first + j of the target from the source's ring, j < S (one launch)
hipError_t launch_rewind_fork(const RewindForkArgs& a, hipStream_t stream);
// one step's flags [B][N] into the tally rows [B][REWIND_TALLY]; watch_slot [B] or NULL (one launch)
hipError_t launch_rewind_tally(const uint8_t* flags, const int32_t* watch_slot, int32_t* tally, int32_t B, int32_t N, hipStream_t stream);

}  // namespace copo
