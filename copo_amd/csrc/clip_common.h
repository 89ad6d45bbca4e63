// Shared declarations of the event-clip recorder (clip_kernels.hip) and its C entry points (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace copo {

constexpr int CLIP_MAX_CAP = 256;          // snapshots per scene ring: pre + post + 1
constexpr int CLIP_WORDS = 6;              // per snapshot and slot: x, y, heading, speed (raw bits), status byte, agent id
constexpr int CLIP_ENV_WORDS = 2;          // per snapshot and scene: t_env, episode
constexpr int CLIP_HEADER = 8;             // per clip: the CH_* words
enum : int { CH_SCENE = 0, CH_FIRST_REC, CH_LENGTH, CH_TRIG_REC, CH_TRIG_SLOT, CH_KIND, CH_TRIG_AID, CH_N_EVENTS };
enum : int { CLIP_KIND_FLAG = 1, CLIP_KIND_TTC = 2, CLIP_KIND_GAP = 4 };
// per-scene state machine, int32 [E][CLIP_SCENE_WORDS] (idle: CS_ARMED == 0); CS_LO: first record a next clip of the scene may hold
enum : int { CS_ARMED = 0, CS_TRIG_REC, CS_TRIG_SLOT, CS_KIND, CS_TRIG_AID, CS_N_EVENTS, CS_COUNTDOWN, CS_LO, CLIP_SCENE_WORDS };
// device counters, int32 [CLIP_COUNTERS]
enum : int { CC_RECORDS = 0, CC_CLIPS, CC_DROPPED, CLIP_COUNTERS = 4 };

// Arguments of the record / flush launches (passed by value).  Device pointers; `state` / `env` are the simulator's own and are only read.
struct ClipArgs {
    const float* state;            // [COPO_STATE_FIELDS][E][N]
    const int32_t* env;            // [E][4]
    int32_t E, N;
    int32_t pre, post, cap, max_clips;
    uint32_t flag_mask;
    float ttc_below, gap_below;    // 0: that trigger is off
    uint32_t* ring;                // [E][cap][CLIP_WORDS][N]
    int32_t* ring_env;             // [E][cap][CLIP_ENV_WORDS]
    int32_t* scene;                // [E][CLIP_SCENE_WORDS]
    int32_t* ready;                // [E]: 0, or 1 + the last record of the clip the scene commits in this call
    int32_t* cid;                  // [E]: clip id of a ready scene (>= max_clips: dropped)
    int32_t* counters;             // [CLIP_COUNTERS]
    uint32_t* pool;                // [max_clips][cap][CLIP_WORDS][N]
    int32_t* pool_env;             // [max_clips][cap][CLIP_ENV_WORDS]
    int32_t* header;               // [max_clips][CLIP_HEADER]
};

// snapshot of every scene into its ring, triggers, state machines, then the ordered commit of the ready scenes (three launches);
// flags [E][N] uint8, ttc / gap [E][N] fp32, each may be NULL
hipError_t launch_clip_record(const ClipArgs& a, const uint8_t* flags, const float* ttc, const float* gap, hipStream_t stream);
// commit every armed scene with the records it has so far (three launches)
hipError_t launch_clip_flush(const ClipArgs& a, hipStream_t stream);
// frame frame_idx[j] of clip clip_idx[j] (of pool arrays snaps / envw with `cap` frames per clip) into scene j < S of a simulator's state
hipError_t launch_clip_scatter(float* state, int32_t* env, int32_t E, int32_t N, const uint32_t* snaps, const int32_t* envw, int32_t cap,
                               const int32_t* clip_idx, const int32_t* frame_idx, int32_t S, hipStream_t stream);

}  // namespace copo
