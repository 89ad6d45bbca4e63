// Traffic field maps over the simulator's scenes (copo_field_*, include/copo_hip.h): where a population drives, queues, crashes and
// comes close, summed over scenes and steps into integer grids per scene group.  Integer accumulators only, so no sum depends on the
// order the workgroups run in.  Two launches per record:
//   events:  one wave per scene, four scenes per workgroup, lane n = slot n.  A slot whose step flags carry DONE counts its crash /
//            out / arrive at the cell the handle remembered for it from the previous record (events are a handful per scene and step:
//            64-bit integer atomics straight into the maps), then the memory is refreshed from the current state.  On a record that
//            accumulates, the workgroup also ORs the tiles its bodies can reach into the tile bits of its scene block.
//   tiles:   one workgroup of 256 per (32 x 32-cell tile, block of scenes, group); gone at once when no body of the block reaches the
//            tile.  Four scenes at a time, one wave each: the bodies are culled against the tile into an LDS list (ballot + prefix
//            count), every lane tests the list against the four cells it owns and counts footprints in registers (no atomic, nothing
//            depends on scheduling); centre-cell layers go by LDS integer atomics into the tile.  At the end the non-zero cells go out
//            as 64-bit integer atomic adds, eight lanes to a row of the tile.  A per-launch partial fits 32 bits (at most 64 scenes x 64
//            slots x 65 280); the maps are int64.
// The grid and the footprint rule are grid_common.h.  The rules are restated in numpy by tests/field_numpy.py.
#include "sim_device.h"
#include "field_common.h"

namespace copo {

namespace {

constexpr int FB = 256, NW = FB / 64, T = FIELD_TILE, TT = T * T;
enum : int { A_VISITS = 0, A_SPEED, A_VX, A_VY, A_CRITICAL, A_LAYERS };
static_assert(FIELD_MASK_WORDS <= FB, "one lane per word of the tile bits");

typedef unsigned long long u64;

}  // namespace

__global__ __launch_bounds__(FB) void field_events_kernel(FieldArgs a, int accumulate) {
    __shared__ uint32_t smask[FIELD_MASK_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < FIELD_MASK_WORDS) smask[tid] = 0u;
    __syncthreads();
    const int e = blockIdx.x * NW + wave;
    if (e < a.E && lane < a.N) {
        const size_t EN = (size_t)a.E * a.N, o = (size_t)e * a.N + lane, HW = (size_t)a.grid.H * a.grid.W;
        const int g = a.groups.of(e);
        const bool routed = g >= 0;
        const int was = a.last[o];
        if (a.flags && routed && was >= 0 && (size_t)was < HW) {
            const uint32_t f = a.flags[o];
            if (f & COPO_F_DONE) {
                u64* M = reinterpret_cast<u64*>(a.maps) + (size_t)g * FIELD_LAYERS * HW + was;
                if (f & COPO_F_CRASH) atomicAdd(M + FL_CRASH * HW, 1ull);
                if (f & COPO_F_OUT) atomicAdd(M + FL_OUT * HW, 1ull);
                if (f & COPO_F_ARRIVE) atomicAdd(M + FL_ARRIVE * HW, 1ull);
            }
        }
        const float x = a.state[o], y = (a.state + EN)[o];
        const int st = st_status((reinterpret_cast<const int32_t*>(a.state) + 13 * EN)[o]);
        a.last[o] = st == ST_ALIVE ? a.grid.cell_of(x, y) : -1;
        if (accumulate && routed && (st == ST_ALIVE || st == ST_WRECK)) {
            int lox, hix, loy, hiy;
            if (a.grid.reach_box(x, y, a.hl, a.hw, lox, hix, loy, hiy)) {
                const int tiles_x = (a.grid.W + T - 1) / T;
                for (int ty = loy / T; ty <= hiy / T; ++ty)
                    for (int tx = lox / T; tx <= hix / T; ++tx) {
                        const int t = ty * tiles_x + tx;
                        atomicOr(&smask[t >> 5], 1u << (t & 31));
                    }
            }
        }
    }
    __syncthreads();
    // (block is a multiple of the four scenes of a workgroup: they share one row of tile bits)
    if (accumulate && tid < FIELD_MASK_WORDS && smask[tid])
        atomicOr(&a.mask[(size_t)(blockIdx.x * NW / a.block) * FIELD_MASK_WORDS + tid], smask[tid]);
}

__global__ __launch_bounds__(FB) void field_tiles_kernel(FieldArgs a) {
    __shared__ uint32_t acc[A_LAYERS][TT];                    // (A_VX / A_VY: two's complement)
    __shared__ float bx[FB], by[FB], bc[FB], bs[FB];          // the bodies that can reach the tile: centre, heading vector
    __shared__ uint32_t bwreck[FB];
    __shared__ int wcnt[NW];
    __shared__ int s_scenes;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_x = (a.grid.W + T - 1) / T;
    const int tile = blockIdx.x, tx = tile % tiles_x, ty = tile / tiles_x, sb = blockIdx.y, g = blockIdx.z;
    // tile 0 counts the scene-records of its group whether a body reaches it or not
    if (tile != 0 && !((a.mask[(size_t)sb * FIELD_MASK_WORDS + (tile >> 5)] >> (tile & 31)) & 1u)) return;
    for (int i = tid; i < A_LAYERS * TT; i += FB) (&acc[0][0])[i] = 0u;
    if (tid == 0) s_scenes = 0;
    // this lane's cells: four in a row of the tile, eight lanes to a row
    const int cx0 = tx * T + (tid & 7) * 4, cy = ty * T + (tid >> 3);
    const float py = a.grid.centre_y(cy);
    float px[4];
    uint32_t occ[4], wrk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        px[q] = a.grid.centre_x(cx0 + q);
        occ[q] = 0u;
        wrk[q] = 0u;
    }
    const float hl = a.hl, hw = a.hw;
    const size_t EN = (size_t)a.E * a.N;
    int n_scenes = 0;
    __syncthreads();
    for (int it = 0; it < a.block; it += NW) {
        const int e = sb * a.block + it + wave;
        const bool mine = e < a.E && a.groups.group[e] == g;     // (the whole wave; g < G is a group of the launch: no range test)
        n_scenes += mine ? 1 : 0;
        bool keep = false;
        float x = 0.0f, y = 0.0f, sn = 0.0f, cs = 0.0f;
        int st = ST_EMPTY;
        if (mine && lane < a.N) {
            const size_t o = (size_t)e * a.N + lane;
            x = a.state[o]; y = (a.state + EN)[o];
            st = st_status((reinterpret_cast<const int32_t*>(a.state) + 13 * EN)[o]);
            if (st == ST_ALIVE || st == ST_WRECK) {
                int lox, hix, loy, hiy;
                keep = a.grid.reach_box(x, y, hl, hw, lox, hix, loy, hiy) &&
                       lox <= tx * T + T - 1 && hix >= tx * T && loy <= ty * T + T - 1 && hiy >= ty * T;
            }
            if (keep) {                                        // (a centre inside the tile is within reach of it)
                sincos_det((a.state + 2 * EN)[o], sn, cs);
                const int cc = st == ST_ALIVE ? a.grid.cell_of(x, y) : -1;
                const int ix = cc >= 0 ? cc % a.grid.W - tx * T : -1, iy = cc >= 0 ? cc / a.grid.W - ty * T : -1;
                if (ix >= 0 && ix < T && iy >= 0 && iy < T) {
                    const int c = iy * T + ix;
                    const float v = (a.state + 3 * EN)[o];
                    const float vc = fminf(fmaxf(v, -255.0f), 255.0f);
                    atomicAdd(&acc[A_VISITS][c], 1u);
                    atomicAdd(&acc[A_SPEED][c], (uint32_t)__float2int_rn(fminf(fmaxf(v, 0.0f), 255.0f) * 256.0f));
                    atomicAdd(&acc[A_VX][c], (uint32_t)__float2int_rn(vc * cs * 256.0f));
                    atomicAdd(&acc[A_VY][c], (uint32_t)__float2int_rn(vc * sn * 256.0f));
                    if (a.ttc && a.ttc_below > 0.0f && a.ttc[o] < a.ttc_below) atomicAdd(&acc[A_CRITICAL][c], 1u);
                }
            }
        }
        // order-preserving compaction over the workgroup (the order does not matter to the counts)
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int c = wcnt[w];
            off += w < wave ? c : 0;
            total += c;
        }
        if (keep) {
            const int pos = off + before;
            bx[pos] = x; by[pos] = y; bc[pos] = cs; bs[pos] = sn; bwreck[pos] = st == ST_WRECK ? 1u : 0u;
        }
        __syncthreads();
        for (int k = 0; k < total; ++k) {
            const float kx = bx[k], kc = bc[k], ks = bs[k], dy = py - by[k];
            const uint32_t kw = bwreck[k];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float dx = px[q] - kx;
                const uint32_t in = covers(dx, dy, kc, ks, hl, hw) ? 1u : 0u;
                occ[q] += in & (kw ^ 1u);
                wrk[q] += in & kw;
            }
        }
        __syncthreads();
    }
    if (lane == 0 && n_scenes) atomicAdd(&s_scenes, n_scenes);
    __syncthreads();
    // ---- the tile into the maps: non-zero cells only ----
    const size_t HW = (size_t)a.grid.H * a.grid.W;
    u64* M = reinterpret_cast<u64*>(a.maps) + (size_t)g * FIELD_LAYERS * HW;
    if (cy < a.grid.H) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (cx0 + q >= a.grid.W) continue;
            u64* C = M + (size_t)cy * a.grid.W + cx0 + q;
            const int c = (tid >> 3) * T + (tid & 7) * 4 + q;
            if (occ[q]) atomicAdd(C + FL_OCCUPANCY * HW, (u64)occ[q]);
            if (wrk[q]) atomicAdd(C + FL_WRECK * HW, (u64)wrk[q]);
            const uint32_t n = acc[A_VISITS][c];
            if (n) {
                atomicAdd(C + FL_VISITS * HW, (u64)n);
                const uint32_t sp = acc[A_SPEED][c], cr = acc[A_CRITICAL][c];
                const int32_t vx = (int32_t)acc[A_VX][c], vy = (int32_t)acc[A_VY][c];
                if (sp) atomicAdd(C + FL_SPEED_Q * HW, (u64)sp);
                if (vx) atomicAdd(C + FL_VX_Q * HW, (u64)(long long)vx);
                if (vy) atomicAdd(C + FL_VY_Q * HW, (u64)(long long)vy);
                if (cr) atomicAdd(C + FL_CRITICAL * HW, (u64)cr);
            }
        }
    }
    if (tile == 0 && tid == 0 && s_scenes) atomicAdd(reinterpret_cast<u64*>(a.scene_records) + g, (u64)s_scenes);
}

hipError_t launch_field_events(const FieldArgs& a, int accumulate, hipStream_t stream) {
    hipLaunchKernelGGL(field_events_kernel, dim3((a.E + NW - 1) / NW), dim3(FB), 0, stream, a, accumulate);
    return hipGetLastError();
}

hipError_t launch_field_tiles(const FieldArgs& a, hipStream_t stream) {
    const int tiles = ((a.grid.W + T - 1) / T) * ((a.grid.H + T - 1) / T);
    hipLaunchKernelGGL(field_tiles_kernel, dim3(tiles, (a.E + a.block - 1) / a.block, a.groups.G), dim3(FB), 0, stream, a);
    return hipGetLastError();
}

}  // namespace copo
