// Top-down rasteriser of the simulator's scenes (copo_render_*, include/copo_hip.h).  One workgroup of 256 threads per (64 x 32
// pixel tile, scene): the map's primitives and the vehicle boxes are culled against the tile's world box into LDS lists (ballot +
// prefix count, in paint order), then every lane shades its 2 x 4 pixels layer by layer and stores each row of 4 as one 16-byte
// word.  The render rules are restated in numpy by tests/render_numpy.py.
#include "sim_device.h"
#include "render_common.h"

namespace copo {

namespace {

constexpr int TW = 64, TH = 32, RB = 256, NW = RB / 64;

__device__ __forceinline__ uint32_t rgba(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16) | 0xff000000u; }
constexpr uint32_t BG = 235u | (235u << 8) | (235u << 16) | 0xff000000u;
constexpr uint32_t ROAD = 90u | (90u << 8) | (90u << 16) | 0xff000000u;
constexpr uint32_t LINE = 0xffffffffu;
constexpr uint32_t WRECK = 220u | (40u << 8) | (40u << 16) | 0xff000000u;

__device__ __forceinline__ uint32_t blend(uint32_t below, uint32_t c, uint32_t w) {
    const uint32_t r = ((below & 0xff) * (256 - w) + (c & 0xff) * w) >> 8;
    const uint32_t g = (((below >> 8) & 0xff) * (256 - w) + ((c >> 8) & 0xff) * w) >> 8;
    const uint32_t b = (((below >> 16) & 0xff) * (256 - w) + ((c >> 16) & 0xff) * w) >> 8;
    return rgba(r, g, b);
}
__device__ __forceinline__ uint32_t marker(uint32_t c) {
    return rgba(((c & 0xff) * 3) >> 2, (((c >> 8) & 0xff) * 3) >> 2, (((c >> 16) & 0xff) * 3) >> 2);
}

// Order-preserving compaction over the workgroup: slot of this thread's item in the list (if `keep`) and the list length.
__device__ __forceinline__ int compact(bool keep, int lane, int wave, int* wcnt, int& total) {
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int c = wcnt[w];
        off += w < wave ? c : 0;
        total += c;
    }
    return off + before;
}

// world box of a primitive {x0, x1, y0, y1} against the tile's, grown by `pad`
__device__ __forceinline__ bool overlaps(const float* bb, float pad, float tx0, float tx1, float ty0, float ty1) {
    return bb[0] - pad <= tx1 && bb[1] + pad >= tx0 && bb[2] - pad <= ty1 && bb[3] + pad >= ty0;
}

// arc length and lateral offset (left +) of (x, y) on a lane-line primitive
__device__ __forceinline__ void project_line(const float* L, float x, float y, float& sl, float& lat) {
    const float kap = L[6];
    if (kap == 0.0f) {
        const float dx = x - L[1], dy = y - L[2];
        sl = fm(dx, L[3], dy * L[4]);
        lat = fm(dy, L[3], -(dx * L[4]));
    } else {
        const float sg = kap > 0.0f ? 1.0f : -1.0f, R = 1.0f / fabsf(kap);
        const float ex = x - L[7], ey = y - L[8];
        const float rho = sqrtf(fm(ex, ex, ey * ey));
        const float ang = atan2_det(sg * fm(L[9], ey, -(L[10] * ex)), fm(L[9], ex, L[10] * ey));
        sl = fm(ang, R, 0.5f * L[5]);
        lat = sg * (R - rho);
    }
}

}  // namespace

__global__ __launch_bounds__(RB) void render_frames_kernel(RenderArgs a) {
    __shared__ int wcnt[NW];
    __shared__ int ilist[RB];
    __shared__ float vx[RB], vy[RB], vc[RB], vs[RB];
    __shared__ uint32_t vcol[RB], vw[RB];      // colour, blend weight (256: opaque vehicle with its heading marker)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_x = (a.W + TW - 1) / TW;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int si = blockIdx.y;
    const int e = a.scenes[si];
    const float cx = a.views[si * 3], cy = a.views[si * 3 + 1], m = a.views[si * 3 + 2];
    const float hW = 0.5f * (float)a.W, hH = 0.5f * (float)a.H;
    const int j0 = tx * TW + (tid & 15) * 4, i0 = ty * TH + (tid >> 4);
    float px[4], py[2];
#pragma unroll
    for (int q = 0; q < 4; ++q) px[q] = cx + (((float)(j0 + q) + 0.5f) - hW) * m;
#pragma unroll
    for (int r = 0; r < 2; ++r) py[r] = cy - (((float)(i0 + 16 * r) + 0.5f) - hH) * m;
    // the tile's pixel centres span [tx0, tx1] x [ty0, ty1]; one pixel of slack for the float rounding of the above
    const float tx0 = cx + (((float)(tx * TW) + 0.5f) - hW) * m - m, tx1 = cx + (((float)(tx * TW + TW - 1) + 0.5f) - hW) * m + m;
    const float ty1 = cy - (((float)(ty * TH) + 0.5f) - hH) * m + m, ty0 = cy - (((float)(ty * TH + TH - 1) + 0.5f) - hH) * m - m;

    uint32_t col[8];
    // ---- 1 road: the lateral rule of the step kernel's out-of-road test (slot_project), without the body margin ----
    {
        bool on[8] = {false, false, false, false, false, false, false, false};
        const float w = a.lane_w;
        for (int base = 0; base < a.n_roads; base += RB) {
            const int i = base + tid;
            const bool keep = i < a.n_roads && overlaps(a.roads + (size_t)i * RENDER_ROAD_STRIDE + 16, 0.0f, tx0, tx1, ty0, ty1);
            int total;
            const int pos = compact(keep, lane, wave, wcnt, total);
            if (keep) ilist[pos] = i;
            __syncthreads();
            for (int k = 0; k < total; ++k) {
                const float* g = a.roads + (size_t)ilist[k] * RENDER_ROAD_STRIDE;
                const float lanes = floorf(g[COPO_SEG_LANES]), len = g[4];
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    float sl, lat, sp;
                    project_seg(g, px[p & 3], py[p >> 2], 1.0f, 0.0f, sl, lat, sp);
                    const float right = (lanes - 0.5f) * w + funnel_extra(g, sl, w);
                    on[p] = on[p] | ((sl >= 0.0f) & (sl <= len) & (lat <= 0.5f * w) & (lat >= -right));
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int p = 0; p < 8; ++p) col[p] = on[p] ? ROAD : BG;
    }
    // ---- 2 lane lines: continuous always, broken where fmod(s, 6) < 3; half width max(0.1 m, m / 2) ----
    {
        const float h = fmaxf(0.1f, 0.5f * m);
        for (int base = 0; base < a.n_lines; base += RB) {
            const int i = base + tid;
            const bool keep = i < a.n_lines && overlaps(a.lines + (size_t)i * RENDER_LINE_STRIDE + 12, h, tx0, tx1, ty0, ty1);
            int total;
            const int pos = compact(keep, lane, wave, wcnt, total);
            if (keep) ilist[pos] = i;
            __syncthreads();
            for (int k = 0; k < total; ++k) {
                const float* L = a.lines + (size_t)ilist[k] * RENDER_LINE_STRIDE;
                const float kind = L[0], len = L[5];
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    float sl, lat;
                    project_line(L, px[p & 3], py[p >> 2], sl, lat);
                    // (every condition evaluated and combined bitwise: no short-circuit branches around the pixel test)
                    const bool dash = (kind == 2.0f) | ((kind == 1.0f) & (fmodf(sl, 6.0f) < 3.0f));
                    const bool in = (sl >= 0.0f) & (sl <= len) & (fabsf(lat) <= h) & dash;
                    col[p] = in ? LINE : col[p];
                }
            }
            __syncthreads();
        }
    }
    // ---- 3 static boxes (at most COPO_MAX_BOXES: a uniform test per box) ----
    for (int b = 0; b < a.n_boxes; ++b) {
        const float* B = a.boxes + b * COPO_BOX_STRIDE;
        const float ext = B[4] + B[5];
        if (B[0] - ext > tx1 || B[0] + ext < tx0 || B[1] - ext > ty1 || B[1] + ext < ty0) continue;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const float dx = px[p & 3] - B[0], dy = py[p >> 2] - B[1];
            const float u = fm(dx, B[2], dy * B[3]), v = fm(dy, B[2], -(dx * B[3]));
            col[p] = (fabsf(u) <= B[4] && fabsf(v) <= B[5]) ? a.box_rgba : col[p];
        }
    }
    // ---- 4 trail (oldest snapshot first, slots in order, blended) and 5 vehicles (slot order, opaque, heading marker) ----
    {
        const int N = a.N, EN = a.E * a.N;
        const int ep_now = a.env[(size_t)e * 4 + 1];
        const int n_items = (a.Kd + 1) * N;
        const float ext = a.hl + a.hw;
        for (int base = 0; base < n_items; base += RB) {
            const int q = base + tid;
            bool keep = false;
            float x = 0.0f, y = 0.0f, th = 0.0f;
            uint32_t c = 0, w = 256;
            if (q < n_items) {
                const int n = q % N, slot_age = a.Kd - q / N;      // snapshots of age Kd .. 1, then the current state (age 0)
                int st, aid;
                if (slot_age > 0) {
                    const int rs = (a.head - slot_age + a.cap) % a.cap;
                    const int32_t* R = a.ring + (size_t)rs * RENDER_RING_FIELDS * EN + (size_t)e * N + n;
                    x = __int_as_float(R[0]); y = __int_as_float(R[(size_t)EN]); th = __int_as_float(R[2 * (size_t)EN]);
                    st = R[3 * (size_t)EN]; aid = R[4 * (size_t)EN];
                    keep = a.ring_ep[(size_t)rs * a.E + e] == ep_now;
                    w = (uint32_t)(160 * (a.K + 1 - slot_age) / (a.K + 1));
                } else {
                    const size_t o = (size_t)e * N + n;
                    const int32_t* si32 = reinterpret_cast<const int32_t*>(a.state);
                    x = a.state[o]; y = a.state[(size_t)EN + o]; th = a.state[2 * (size_t)EN + o];
                    st = st_status(si32[13 * (size_t)EN + o]); aid = si32[14 * (size_t)EN + o];
                    keep = true;
                }
                keep = keep && (st == ST_ALIVE || st == ST_WRECK);
                c = st == ST_WRECK ? WRECK : a.palette[((aid % 12) + 12) % 12];
                keep = keep && x - ext <= tx1 && x + ext >= tx0 && y - ext <= ty1 && y + ext >= ty0;
            }
            int total;
            const int pos = compact(keep, lane, wave, wcnt, total);
            if (keep) {
                float sn, cs;
                sincosf(th, &sn, &cs);
                vx[pos] = x; vy[pos] = y; vc[pos] = cs; vs[pos] = sn; vcol[pos] = c; vw[pos] = w;
            }
            __syncthreads();
            for (int k = 0; k < total; ++k) {
                const float bx = vx[k], by = vy[k], bc = vc[k], bs = vs[k];
                const uint32_t kc = vcol[k], kw = vw[k];
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const float dx = px[p & 3] - bx, dy = py[p >> 2] - by;
                    const float u = fm(dx, bc, dy * bs), v = fm(dy, bc, -(dx * bs));
                    if (fabsf(u) <= a.hl && fabsf(v) <= a.hw)
                        col[p] = kw == 256 ? (u >= 0.5f * a.hl ? marker(kc) : kc) : blend(col[p], kc, kw);
                }
            }
            __syncthreads();
        }
    }
    // ---- store: a row of 4 pixels per 16-byte word when rows are 16-byte aligned ----
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = i0 + 16 * r;
        if (i >= a.H) continue;
        uint32_t* row = a.out + ((size_t)si * a.H + i) * a.W;
        if ((a.W & 3) == 0) {
            if (j0 < a.W) *reinterpret_cast<uint4*>(row + j0) = make_uint4(col[4 * r], col[4 * r + 1], col[4 * r + 2], col[4 * r + 3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (j0 + q < a.W) row[j0 + q] = col[4 * r + q];
        }
    }
}

__global__ __launch_bounds__(256) void render_record_kernel(const float* __restrict__ state, const int32_t* __restrict__ env, int32_t E,
                                                            int32_t N, int32_t* __restrict__ ring, int32_t* __restrict__ ring_ep,
                                                            int32_t slot) {
    const int EN = E * N;
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= EN) return;
    const int32_t* si = reinterpret_cast<const int32_t*>(state);
    int32_t* R = ring + (size_t)slot * RENDER_RING_FIELDS * EN + o;
    R[0] = si[o];
    R[(size_t)EN] = si[(size_t)EN + o];
    R[2 * (size_t)EN] = si[2 * (size_t)EN + o];
    R[3 * (size_t)EN] = st_status(si[13 * (size_t)EN + o]);
    R[4 * (size_t)EN] = si[14 * (size_t)EN + o];
    if (o % N == 0) ring_ep[(size_t)slot * E + o / N] = env[(size_t)(o / N) * 4 + 1];
}

hipError_t launch_render_frames(const RenderArgs& a, hipStream_t stream) {
    const dim3 grid(((a.W + TW - 1) / TW) * ((a.H + TH - 1) / TH), a.S);
    hipLaunchKernelGGL(render_frames_kernel, grid, dim3(RB), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_render_record(const float* state, const int32_t* env, int32_t E, int32_t N, int32_t* ring, int32_t* ring_ep,
                                int32_t slot, hipStream_t stream) {
    const int EN = E * N;
    hipLaunchKernelGGL(render_record_kernel, dim3((EN + 255) / 256), dim3(256), 0, stream, state, env, E, N, ring, ring_ep, slot);
    return hipGetLastError();
}

}  // namespace copo
