// Shared declarations of the top-down renderer (render_kernels.hip) and its C entry points (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace copo {

constexpr int RENDER_MAX_TRAIL = 32;
constexpr int RENDER_MAX_SIZE = 4096;
constexpr int RENDER_ROAD_STRIDE = 20;     // the road record (COPO_SEG_STRIDE floats) + world bounding box {x0, x1, y0, y1}
constexpr int RENDER_LINE_STRIDE = 16;     // the lane-line record (COPO_LINE_STRIDE floats) + world bounding box
constexpr int RENDER_RING_FIELDS = 5;      // per snapshot and slot: x, y, heading, status (low byte of the status word), agent id

// Arguments of one frame batch (passed by value).  Device pointers; `state` / `env` are the simulator's own.
struct RenderArgs {
    const float* state;            // [COPO_STATE_FIELDS][E][N]
    const int32_t* env;            // [E][4]
    int32_t E, N;
    const float* roads;            // [n_roads][RENDER_ROAD_STRIDE]
    const float* lines;            // [n_lines][RENDER_LINE_STRIDE]
    const float* boxes;            // [n_boxes][COPO_BOX_STRIDE]
    int32_t n_roads, n_lines, n_boxes;
    uint32_t box_rgba;             // seen by the LiDAR / hidden colour, chosen at create
    const uint32_t* palette;       // [12] packed RGBA8
    const int32_t* ring;           // [cap][RENDER_RING_FIELDS][E][N]
    const int32_t* ring_ep;        // [cap][E]: the scene's episode counter at the snapshot
    int32_t cap, head;             // ring capacity, slot the next snapshot goes to
    int32_t K, Kd;                 // trail length of the weights, snapshots drawn (min(K, recorded))
    float hl, hw, lane_w;
    const int32_t* scenes;         // [S]
    const float* views;            // [S][3] cx, cy, metres per pixel
    int32_t S, W, H;
    uint32_t* out;                 // [S][H][W] packed RGBA8
};

hipError_t launch_render_frames(const RenderArgs& a, hipStream_t stream);
// copy the current x, y, heading, status, agent id of every slot and each scene's episode counter into ring slot `slot`
hipError_t launch_render_record(const float* state, const int32_t* env, int32_t E, int32_t N, int32_t* ring, int32_t* ring_ep,
                                int32_t slot, hipStream_t stream);

}  // namespace copo
