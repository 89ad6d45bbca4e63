// C ABI of the handles that observe a simulator (include/copo_hip.h): renderer, interaction meter, event clips, scene rewind, field
// maps, traffic gates, trip log, conflict log, encroachment log.  Each owns its device buffers through a DevPool (capi_common.h) on the simulator's device; every call but
// *_destroy reads the simulator, which therefore has to be alive.  All launches are asynchronous on the caller's stream.
#include <algorithm>
#include <array>
#include <cmath>
#include <new>
#include <set>
#include <vector>

#include "capi_common.h"
#include "render_common.h"
#include "interact_common.h"
#include "clip_common.h"
#include "rewind_common.h"
#include "field_common.h"
#include "gate_common.h"
#include "trip_common.h"
#include "conflict_common.h"
#include "encroach_common.h"

using namespace copo;

// ---- top-down renderer (render_kernels.hip) ----------------------------------------------------------------

struct copo_render {
    copo_sim* sim;
    DevPool mem;
    int W, H, cap, head, count;
    int n_roads, n_lines;
    uint32_t box_rgba;
    DevBuf<float> roads;       // [n_roads][RENDER_ROAD_STRIDE] deduplicated road records + world boxes
    DevBuf<float> lines;       // [n_lines][RENDER_LINE_STRIDE]
    DevBuf<uint32_t> palette;  // [12]
    DevBuf<int32_t> ring;      // [cap][RENDER_RING_FIELDS][E][N]
    DevBuf<int32_t> ring_ep;   // [cap][E]
};

// world box {x0, x1, y0, y1} of the points at lateral offsets lat0 and lat1 (left +) of a straight or arc of `len` metres starting at
// (x0, y0) with heading (c, s) and curvature kap; sampled finely enough that 0.5 m of padding covers the chords
static void prim_box(double x0, double y0, double c, double s, double len, double kap, double lat0, double lat1, float* bb) {
    double lo_x = 1e30, hi_x = -1e30, lo_y = 1e30, hi_y = -1e30;
    const int n = 129;
    for (int k = 0; k < n; ++k) {
        const double sl = len * k / (n - 1), a = kap * sl;
        double px, py, hc, hs;
        if (kap == 0.0) {
            px = x0 + c * sl; py = y0 + s * sl; hc = c; hs = s;
        } else {
            const double r = 1.0 / kap;       // signed
            hc = c * std::cos(a) - s * std::sin(a);
            hs = s * std::cos(a) + c * std::sin(a);
            px = x0 + r * (hs - s); py = y0 - r * (hc - c);
        }
        for (double lat : {lat0, lat1}) {
            const double qx = px - hs * lat, qy = py + hc * lat;
            lo_x = std::min(lo_x, qx); hi_x = std::max(hi_x, qx); lo_y = std::min(lo_y, qy); hi_y = std::max(hi_y, qy);
        }
    }
    bb[0] = (float)(lo_x - 0.5); bb[1] = (float)(hi_x + 0.5); bb[2] = (float)(lo_y - 0.5); bb[3] = (float)(hi_y + 0.5);
}

extern "C" int copo_render_create(copo_sim* sim, int32_t width, int32_t height, int32_t trail, const uint8_t* palette_rgb,
                                  copo_render** out) {
    if (!sim || !palette_rgb || !out) return fail(COPO_ERR_NULL, "copo_render_create: NULL argument");
    *out = nullptr;
    if (width < 1 || width > RENDER_MAX_SIZE || height < 1 || height > RENDER_MAX_SIZE || trail < 0 || trail > RENDER_MAX_TRAIL)
        return fail(COPO_ERR_DIM, "copo_render_create: %d x %d pixels (1..%d each), trail %d (0..%d)", width, height, RENDER_MAX_SIZE,
                    trail, RENDER_MAX_TRAIL);
    HIP_TRY(hipSetDevice(sim->device));
    copo_render* r = new (std::nothrow) copo_render();
    if (!r) return fail(COPO_ERR_DEVICE, "out of host memory");
    r->sim = sim; r->mem.device = sim->device; r->W = width; r->H = height; r->cap = trail; r->head = 0; r->count = 0;
    const SimParams& p = sim->p;
    const double w = p.lane_width;
    // road records of every route, deduplicated on the fields the road rule reads (routes share their roads)
    std::vector<float> roads;
    std::set<std::array<float, 10>> seen;
    for (int q = 0; q < p.n_routes; ++q) {
        const int nseg = (int)sim->h_meta[(size_t)q * 4 + 1];
        for (int k = 0; k < nseg; ++k) {
            const float* g = sim->h_segs.data() + ((size_t)q * p.seg_rows + k) * COPO_SEG_STRIDE;
            const std::array<float, 10> key = {g[0], g[1], g[2], g[3], g[4], g[5], floorf(g[COPO_SEG_LANES]), g[12], g[14], g[15]};
            if (!seen.insert(key).second) continue;
            const size_t o = roads.size();
            roads.resize(o + RENDER_ROAD_STRIDE);
            std::copy(g, g + COPO_SEG_STRIDE, roads.begin() + o);
            const double lanes = std::floor((double)g[COPO_SEG_LANES]);
            const double funnel = (g[5] == 0.0f && g[12] != 0.0f) ? std::fabs((double)g[14]) : 0.0;
            prim_box(g[0], g[1], g[2], g[3], g[4], g[5], 0.5 * w, -((lanes - 0.5) * w + funnel), roads.data() + o + 16);
        }
    }
    std::vector<float> lines;
    const int nl = (int)(sim->h_lines.size() / COPO_LINE_STRIDE);
    for (int k = 0; k < nl; ++k) {
        const float* L = sim->h_lines.data() + (size_t)k * COPO_LINE_STRIDE;
        const size_t o = lines.size();
        lines.resize(o + RENDER_LINE_STRIDE);
        std::copy(L, L + COPO_LINE_STRIDE, lines.begin() + o);
        prim_box(L[1], L[2], L[3], L[4], L[5], L[6], 0.0, 0.0, lines.data() + o + 12);
    }
    uint32_t pal[12];
    for (int k = 0; k < 12; ++k)
        pal[k] = (uint32_t)palette_rgb[3 * k] | ((uint32_t)palette_rgb[3 * k + 1] << 8) | ((uint32_t)palette_rgb[3 * k + 2] << 16) | 0xff000000u;
    r->n_roads = (int)(roads.size() / RENDER_ROAD_STRIDE);
    r->n_lines = nl;
    r->box_rgba = sim->boxes_hidden ? (190u | (150u << 8) | (110u << 16) | 0xff000000u) : (120u | (80u << 8) | (50u << 16) | 0xff000000u);
    const size_t EN = (size_t)p.E * p.N;
    r->roads = r->mem.upload(roads.data(), roads.size());
    r->lines = r->mem.upload(lines.data(), lines.size());
    r->palette = r->mem.upload(pal, 12);
    r->ring = r->mem.alloc<int32_t>((size_t)trail * RENDER_RING_FIELDS * EN);      // (trail 0: never indexed)
    r->ring_ep = r->mem.alloc<int32_t>((size_t)trail * p.E);
    return finish_create(r, out, "copo_render_create");
}

extern "C" int copo_render_destroy(copo_render* r) { return destroy_handle(r, "copo_render_destroy"); }

extern "C" int copo_render_record(copo_render* r, void* stream) {
    if (!r) return fail(COPO_ERR_NULL, "copo_render_record: NULL handle");
    if (r->cap == 0) return COPO_OK;
    const SimParams& p = r->sim->p;
    HIP_TRY(launch_render_record(p.state, p.env, p.E, p.N, r->ring, r->ring_ep, r->head, static_cast<hipStream_t>(stream)));
    r->head = (r->head + 1) % r->cap;
    r->count = std::min(r->count + 1, r->cap);
    return COPO_OK;
}

extern "C" int copo_render_clear(copo_render* r, void* stream) {
    (void)stream;
    if (!r) return fail(COPO_ERR_NULL, "copo_render_clear: NULL handle");
    r->head = 0;
    r->count = 0;
    return COPO_OK;
}

extern "C" int copo_render_frames(copo_render* r, const int32_t* scenes, int32_t S, const float* views, int32_t trail, uint32_t* rgba,
                                  void* stream) {
    if (!r || !scenes || !views || !rgba) return fail(COPO_ERR_NULL, "copo_render_frames: NULL argument");
    const SimParams& p = r->sim->p;
    if (S < 1 || S > p.E) return fail(COPO_ERR_DIM, "copo_render_frames: S=%d scenes (1..%d)", S, p.E);
    if (trail < 0 || trail > r->cap) return fail(COPO_ERR_DIM, "copo_render_frames: trail=%d (0..%d, the capacity at create)", trail, r->cap);
    RenderArgs a;
    a.state = p.state; a.env = p.env; a.E = p.E; a.N = p.N;
    a.roads = r->roads; a.lines = r->lines; a.boxes = p.boxes;
    a.n_roads = r->n_roads; a.n_lines = r->n_lines; a.n_boxes = p.n_boxes;
    a.box_rgba = r->box_rgba; a.palette = r->palette;
    a.ring = r->ring; a.ring_ep = r->ring_ep; a.cap = r->cap; a.head = r->head;
    a.K = trail; a.Kd = std::min(trail, r->count);
    a.hl = p.hl; a.hw = p.hw; a.lane_w = p.lane_width;
    a.scenes = scenes; a.views = views; a.S = S; a.W = r->W; a.H = r->H; a.out = rgba;
    HIP_TRY(launch_render_frames(a, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

// ---- interaction meter (interact_kernels.hip) ----------------------------------------------------------------

struct copo_interact {
    copo_sim* sim;
    DevPool mem;
    copo_interact_cfg cfg;
    DevBuf<int32_t> acc;       // [INTERACT_ACC_WORDS][E][N]
    DevBuf<double> tit;        // [E][N]
    DevBuf<long long> counts;  // [E][INTERACT_COUNTS]
    DevBuf<double> sums;       // [E][INTERACT_SUMS]
};

static InteractArgs interact_args(const copo_interact* h) {
    const SimParams& p = h->sim->p;
    InteractArgs a;
    a.state = p.state; a.env = p.env; a.E = p.E; a.N = p.N;
    a.hl = p.hl; a.hw = p.hw; a.dt = p.dt;
    a.horizon_s = h->cfg.horizon_s; a.ttc_crit_s = h->cfg.ttc_crit_s; a.gap_near_m = h->cfg.gap_near_m; a.brake_mps2 = h->cfg.brake_mps2;
    a.acc = h->acc; a.tit = h->tit; a.counts = h->counts; a.sums = h->sums;
    return a;
}

extern "C" int copo_interact_create(copo_sim* sim, const copo_interact_cfg* cfg, copo_interact** out) {
    if (!sim || !cfg || !out) return fail(COPO_ERR_NULL, "copo_interact_create: NULL argument");
    *out = nullptr;
    if (!(cfg->horizon_s > 0.0f) || !(cfg->brake_mps2 > 0.0f) || !(cfg->ttc_crit_s >= 0.0f) || !(cfg->gap_near_m >= 0.0f) ||
        !std::isfinite(cfg->horizon_s) || !std::isfinite(cfg->brake_mps2) || !std::isfinite(cfg->ttc_crit_s) || !std::isfinite(cfg->gap_near_m))
        return fail(COPO_ERR_CONFIG, "copo_interact_create: horizon_s=%g brake_mps2=%g (> 0), ttc_crit_s=%g gap_near_m=%g (>= 0), all finite",
                    (double)cfg->horizon_s, (double)cfg->brake_mps2, (double)cfg->ttc_crit_s, (double)cfg->gap_near_m);
    HIP_TRY(hipSetDevice(sim->device));
    copo_interact* h = new (std::nothrow) copo_interact();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->sim = sim; h->mem.device = sim->device; h->cfg = *cfg;
    const size_t E = (size_t)sim->p.E, EN = E * sim->p.N;
    h->acc = h->mem.alloc<int32_t>((size_t)INTERACT_ACC_WORDS * EN);
    h->tit = h->mem.alloc<double>(EN);
    h->counts = h->mem.alloc<long long>(E * INTERACT_COUNTS);
    h->sums = h->mem.alloc<double>(E * INTERACT_SUMS);
    return finish_create(h, out, "copo_interact_create");
}

extern "C" int copo_interact_destroy(copo_interact* h) { return destroy_handle(h, "copo_interact_destroy"); }

extern "C" int copo_interact_record(copo_interact* h, float* gap, float* ttc, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_interact_record: NULL handle");
    HIP_TRY(launch_interact_record(interact_args(h), gap, ttc, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_interact_totals(copo_interact* h, int64_t* counts_i64, double* sums_f64, int32_t flush_open, void* stream) {
    if (!h || !counts_i64 || !sums_f64) return fail(COPO_ERR_NULL, "copo_interact_totals: NULL argument");
    if (flush_open != 0 && flush_open != 1) return fail(COPO_ERR_DIM, "copo_interact_totals: flush_open=%d (0 or 1)", flush_open);
    HIP_TRY(launch_interact_totals(interact_args(h), reinterpret_cast<long long*>(counts_i64), sums_f64, flush_open,
                                   static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_interact_reset(copo_interact* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_interact_reset: NULL handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(h->acc.fill(0, st));
    HIP_TRY(h->tit.fill(0, st));
    HIP_TRY(h->counts.fill(0, st));
    HIP_TRY(h->sums.fill(0, st));
    return COPO_OK;
}

// ---- event clips (clip_kernels.hip) ----------------------------------------------------------------------------

struct copo_clip {
    copo_sim* sim;
    DevPool mem;
    copo_clip_cfg cfg;
    int32_t cap;
    DevBuf<uint32_t> ring, pool;
    DevBuf<int32_t> ring_env, scene, ready, cid, counters, pool_env, header;
};

static ClipArgs clip_args(const copo_clip* h) {
    const SimParams& p = h->sim->p;
    ClipArgs a;
    a.state = p.state; a.env = p.env; a.E = p.E; a.N = p.N;
    a.pre = h->cfg.pre; a.post = h->cfg.post; a.cap = h->cap; a.max_clips = h->cfg.max_clips;
    a.flag_mask = h->cfg.flag_mask; a.ttc_below = h->cfg.ttc_below; a.gap_below = h->cfg.gap_below;
    a.ring = h->ring; a.ring_env = h->ring_env; a.scene = h->scene; a.ready = h->ready; a.cid = h->cid; a.counters = h->counters;
    a.pool = h->pool; a.pool_env = h->pool_env; a.header = h->header;
    return a;
}

extern "C" int copo_clip_create(copo_sim* sim, const copo_clip_cfg* cfg, copo_clip** out) {
    if (!sim || !cfg || !out) return fail(COPO_ERR_NULL, "copo_clip_create: NULL argument");
    *out = nullptr;
    if (cfg->pre < 0 || cfg->post < 0 || cfg->pre > COPO_CLIP_MAX_CAP || cfg->post > COPO_CLIP_MAX_CAP || cfg->pre + cfg->post + 1 > COPO_CLIP_MAX_CAP)
        return fail(COPO_ERR_DIM, "copo_clip_create: pre=%d post=%d (>= 0, pre + post + 1 <= %d)", cfg->pre, cfg->post, COPO_CLIP_MAX_CAP);
    if (cfg->max_clips < 1) return fail(COPO_ERR_DIM, "copo_clip_create: max_clips=%d (>= 1)", cfg->max_clips);
    if (!(cfg->ttc_below >= 0.0f) || !(cfg->gap_below >= 0.0f) || !std::isfinite(cfg->ttc_below) || !std::isfinite(cfg->gap_below) ||
        cfg->flag_mask > 0xffu)
        return fail(COPO_ERR_CONFIG, "copo_clip_create: ttc_below=%g gap_below=%g (>= 0, finite; 0 = off), flag_mask=0x%x (COPO_F_* bits)",
                    (double)cfg->ttc_below, (double)cfg->gap_below, cfg->flag_mask);
    static_assert(COPO_CLIP_MAX_CAP == CLIP_MAX_CAP && COPO_CLIP_WORDS == CLIP_WORDS && COPO_CLIP_HEADER == CLIP_HEADER, "copo_hip.h / clip_common.h");
    HIP_TRY(hipSetDevice(sim->device));
    copo_clip* h = new (std::nothrow) copo_clip();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->sim = sim; h->mem.device = sim->device; h->cfg = *cfg; h->cap = cfg->pre + cfg->post + 1;
    const size_t E = (size_t)sim->p.E, N = (size_t)sim->p.N, cap = (size_t)h->cap, C = (size_t)cfg->max_clips;
    // idle state machines, no clip, record 0; the pool is zeroed so that frames beyond a clip's length read 0
    h->ring = h->mem.alloc<uint32_t>(E * cap * CLIP_WORDS * N);
    h->ring_env = h->mem.alloc<int32_t>(E * cap * CLIP_ENV_WORDS);
    h->scene = h->mem.alloc<int32_t>(E * CLIP_SCENE_WORDS);
    h->ready = h->mem.alloc<int32_t>(E);
    h->cid = h->mem.alloc<int32_t>(E);
    h->counters = h->mem.alloc<int32_t>(CLIP_COUNTERS);
    h->pool = h->mem.alloc<uint32_t>(C * cap * CLIP_WORDS * N);
    h->pool_env = h->mem.alloc<int32_t>(C * cap * CLIP_ENV_WORDS);
    h->header = h->mem.alloc<int32_t>(C * CLIP_HEADER);
    return finish_create(h, out, "copo_clip_create");
}

extern "C" int copo_clip_destroy(copo_clip* h) { return destroy_handle(h, "copo_clip_destroy"); }

extern "C" int copo_clip_record(copo_clip* h, const uint8_t* flags, const float* ttc, const float* gap, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_clip_record: NULL handle");
    HIP_TRY(launch_clip_record(clip_args(h), flags, ttc, gap, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_clip_flush(copo_clip* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_clip_flush: NULL handle");
    HIP_TRY(launch_clip_flush(clip_args(h), static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_clip_count(copo_clip* h, int32_t* n_clips, int32_t* dropped, void* stream) {
    if (!h || !n_clips || !dropped) return fail(COPO_ERR_NULL, "copo_clip_count: NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t c[CLIP_COUNTERS];
    HIP_TRY(hipMemcpyAsync(c, h->counters, sizeof(c), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_clips = c[CC_CLIPS];
    *dropped = c[CC_DROPPED];
    return COPO_OK;
}

extern "C" int copo_clip_read(copo_clip* h, int32_t first, int32_t n, int32_t* header_out, uint32_t* snaps_out, int32_t* env_out, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_clip_read: NULL handle");
    if (first < 0 || n < 0 || (int64_t)first + n > h->cfg.max_clips)
        return fail(COPO_ERR_DIM, "copo_clip_read: clips [%d, %d + %d) of a pool of %d", first, first, n, h->cfg.max_clips);
    if (n == 0) return COPO_OK;
    if (!header_out || !snaps_out || !env_out) return fail(COPO_ERR_NULL, "copo_clip_read: NULL output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t per = (size_t)h->cap * CLIP_WORDS * h->sim->p.N, per_env = (size_t)h->cap * CLIP_ENV_WORDS;
    HIP_TRY(hipMemcpyAsync(header_out, h->header.p + (size_t)first * CLIP_HEADER, (size_t)n * CLIP_HEADER * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(snaps_out, h->pool.p + (size_t)first * per, (size_t)n * per * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(env_out, h->pool_env.p + (size_t)first * per_env, (size_t)n * per_env * 4, hipMemcpyDeviceToDevice, st));
    return COPO_OK;
}

// (the ring needs no clearing: a clip never reaches back beyond the records made since)
extern "C" int copo_clip_reset(copo_clip* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_clip_reset: NULL handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(h->scene.fill(0, st));
    HIP_TRY(h->ready.fill(0, st));
    HIP_TRY(h->cid.fill(0, st));
    HIP_TRY(h->counters.fill(0, st));
    HIP_TRY(h->pool.fill(0, st));
    HIP_TRY(h->pool_env.fill(0, st));
    HIP_TRY(h->header.fill(0, st));
    return COPO_OK;
}

extern "C" int copo_clip_scatter(copo_sim* target, const uint32_t* snaps, const int32_t* envw, int32_t cap, int32_t N, const int32_t* clip_idx,
                                 const int32_t* frame_idx, int32_t S, void* stream) {
    if (!target || !snaps || !envw || !clip_idx || !frame_idx) return fail(COPO_ERR_NULL, "copo_clip_scatter: NULL argument");
    if (cap < 1 || cap > COPO_CLIP_MAX_CAP) return fail(COPO_ERR_DIM, "copo_clip_scatter: cap=%d (1..%d)", cap, COPO_CLIP_MAX_CAP);
    if (N != target->p.N) return fail(COPO_ERR_DIM, "copo_clip_scatter: clips of %d slots, a simulator of %d", N, target->p.N);
    if (S < 1 || S > target->p.E) return fail(COPO_ERR_DIM, "copo_clip_scatter: S=%d scenes into a simulator of %d", S, target->p.E);
    HIP_TRY(launch_clip_scatter(target->p.state, target->p.env, target->p.E, N, snaps, envw, cap, clip_idx, frame_idx, S,
                                static_cast<hipStream_t>(stream)));
    target->started = true;
    return COPO_OK;
}

// ---- scene rewind (rewind_kernels.hip) -------------------------------------------------------------------------

struct copo_rewind {
    copo_sim* sim;
    DevPool mem;
    int32_t depth, stride;
    int64_t n_records;             // records made since create / reset (host side: the feature is eager only)
    DevBuf<uint32_t> ring;
    DevBuf<int32_t> ring_env;
};

extern "C" int copo_rewind_create(copo_sim* sim, const copo_rewind_cfg* cfg, copo_rewind** out) {
    if (!sim || !cfg || !out) return fail(COPO_ERR_NULL, "copo_rewind_create: NULL argument");
    *out = nullptr;
    if (cfg->depth < 1 || cfg->depth > COPO_REWIND_MAX_DEPTH || cfg->stride < 1)
        return fail(COPO_ERR_DIM, "copo_rewind_create: depth=%d (1..%d) stride=%d (>= 1)", cfg->depth, COPO_REWIND_MAX_DEPTH, cfg->stride);
    static_assert(COPO_REWIND_MAX_DEPTH == REWIND_MAX_DEPTH && COPO_REWIND_TALLY == REWIND_TALLY, "copo_hip.h / rewind_common.h");
    HIP_TRY(hipSetDevice(sim->device));
    copo_rewind* h = new (std::nothrow) copo_rewind();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->sim = sim; h->mem.device = sim->device; h->depth = cfg->depth; h->stride = cfg->stride; h->n_records = 0;
    const size_t E = (size_t)sim->p.E, N = (size_t)sim->p.N, D = (size_t)cfg->depth;
    h->ring = h->mem.alloc<uint32_t>(E * D * COPO_STATE_FIELDS * N);
    h->ring_env = h->mem.alloc<int32_t>(E * D * REWIND_ENV_WORDS);
    return finish_create(h, out, "copo_rewind_create");
}

extern "C" int copo_rewind_destroy(copo_rewind* h) { return destroy_handle(h, "copo_rewind_destroy"); }

extern "C" int copo_rewind_record(copo_rewind* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_rewind_record: NULL handle");
    const int64_t r = h->n_records;
    if (r >= INT32_MAX) return fail(COPO_ERR_STATE, "copo_rewind_record: 2^31 - 1 records since the last reset");
    if (r % h->stride == 0) {
        const SimParams& p = h->sim->p;
        RewindArgs a;
        a.state = p.state; a.env = p.env; a.E = p.E; a.N = p.N; a.depth = h->depth; a.ring = h->ring; a.ring_env = h->ring_env;
        HIP_TRY(launch_rewind_record(a, (int)((r / h->stride) % h->depth), static_cast<hipStream_t>(stream)));
    }
    h->n_records = r + 1;
    return COPO_OK;
}

// (the ring needs no clearing: a fork never reaches back beyond the records made since)
extern "C" int copo_rewind_reset(copo_rewind* h) {
    if (!h) return fail(COPO_ERR_NULL, "copo_rewind_reset: NULL handle");
    h->n_records = 0;
    return COPO_OK;
}

extern "C" int copo_rewind_count(copo_rewind* h, int32_t* n_records) {
    if (!h || !n_records) return fail(COPO_ERR_NULL, "copo_rewind_count: NULL argument");
    *n_records = (int32_t)h->n_records;
    return COPO_OK;
}

extern "C" int copo_rewind_fork(copo_rewind* h, copo_sim* target, int32_t first, int32_t S, const int32_t* scene, const int32_t* rec,
                                const float* lcf, const uint64_t* seeds, const int32_t* watch_slot, int32_t* status, int32_t* watch_aid,
                                void* stream) {
    if (!h || !target || !scene || !rec || !status) return fail(COPO_ERR_NULL, "copo_rewind_fork: NULL argument");
    const SimParams &sp = h->sim->p, &tp = target->p;
    if (target == h->sim) return fail(COPO_ERR_CONFIG, "copo_rewind_fork: the target is the source simulator");
    if (target->device != h->sim->device)
        return fail(COPO_ERR_CONFIG, "copo_rewind_fork: the target lives on GPU %d, the source on GPU %d", target->device, h->sim->device);
    if (tp.N != sp.N || tp.n_routes != sp.n_routes || tp.n_spawns != sp.n_spawns || tp.O != sp.O)
        return fail(COPO_ERR_DIM, "copo_rewind_fork: target slots / routes / spawns / obs %d / %d / %d / %d, source %d / %d / %d / %d", tp.N,
                    tp.n_routes, tp.n_spawns, tp.O, sp.N, sp.n_routes, sp.n_spawns, sp.O);
    if (S < 1 || first < 0 || (int64_t)first + S > tp.E)
        return fail(COPO_ERR_DIM, "copo_rewind_fork: scenes [%d, %d + %d) of a target of %d", first, first, S, tp.E);
    RewindForkArgs a;
    a.ring = h->ring; a.ring_env = h->ring_env; a.src_seeds = sp.seeds;
    a.E = sp.E; a.N = sp.N; a.depth = h->depth; a.stride = h->stride; a.n_records = (int32_t)h->n_records;
    a.state = tp.state; a.env = tp.env; a.seeds = const_cast<uint64_t*>(tp.seeds); a.TE = tp.E; a.first = first; a.S = S;
    a.scene = scene; a.rec = rec; a.lcf = lcf; a.new_seeds = seeds; a.watch_slot = watch_slot; a.status = status; a.watch_aid = watch_aid;
    HIP_TRY(launch_rewind_fork(a, static_cast<hipStream_t>(stream)));
    target->started = true;
    return COPO_OK;
}

extern "C" int copo_rewind_tally(const uint8_t* flags, const int32_t* watch_slot, int32_t* tally, int32_t B, int32_t N, void* stream) {
    if (!flags || !tally) return fail(COPO_ERR_NULL, "copo_rewind_tally: NULL argument");
    if (B < 0 || N < 1 || N > COPO_MAX_AGENTS) return fail(COPO_ERR_DIM, "copo_rewind_tally: B=%d N=%d (N in 1..%d)", B, N, COPO_MAX_AGENTS);
    if (B == 0) return COPO_OK;
    HIP_TRY(launch_rewind_tally(flags, watch_slot, tally, B, N, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

// ---- scene grid and scene groups of the field maps, the traffic gates and the encroachment log (grid_common.h) --------------------------
// The checks of a grid that are the same for every handle over one, and its GridSpec.  `who`: the entry point, for the error string.
static int make_grid(float x0, float y0, float cell, int32_t W, int32_t H, const char* who, GridSpec* out) {
    if (W < 1 || W > GRID_MAX_SIDE || H < 1 || H > GRID_MAX_SIDE || !(cell > 0.0f) || !std::isfinite(cell))
        return fail(COPO_ERR_DIM, "%s: W=%d H=%d (1..%d) cell=%g (> 0, finite)", who, W, H, GRID_MAX_SIDE, (double)cell);
    const float inv_cell = (float)(1.0 / (double)cell);
    if (!std::isfinite(x0) || !std::isfinite(y0) || !std::isfinite(inv_cell))
        return fail(COPO_ERR_CONFIG, "%s: x0=%g y0=%g 1/cell=%g (finite)", who, (double)x0, (double)y0, (double)inv_cell);
    *out = GridSpec{x0, y0, cell, inv_cell, W, H};
    return COPO_OK;
}

// Host side of the routing of scenes into scene groups: all scenes in group 0 at first
struct GroupTable {
    DevBuf<int32_t> group;                 // [E]
    SceneGroups args(int32_t G) const { return SceneGroups{group, G}; }
    template <typename H> static int set(H* h, const int32_t* group_dev, void* stream, const char* who) {      // (h owns a `groups`)
        if (!h || !group_dev) return fail(COPO_ERR_NULL, "%s: NULL argument", who);
        HIP_TRY(h->groups.group.copy_from(group_dev, static_cast<hipStream_t>(stream)));
        return COPO_OK;
    }
};

// ---- traffic field maps (field_kernels.hip) --------------------------------------------------------------------

struct copo_field {
    copo_sim* sim;
    DevPool mem;
    copo_field_cfg cfg;
    GridSpec grid;
    int32_t block, n_blocks;           // scenes per workgroup of the tile pass, and how many such blocks
    GroupTable groups;
    DevBuf<int32_t> last;              // [E][N]
    DevBuf<uint32_t> mask;             // [n_blocks][FIELD_MASK_WORDS]
    DevBuf<long long> maps;            // [G][FIELD_LAYERS][H][W]
    DevBuf<long long> scene_records;   // [G]
};

static FieldArgs field_args(const copo_field* h, const uint8_t* flags, const float* ttc) {
    const SimParams& p = h->sim->p;
    FieldArgs a;
    a.state = p.state; a.E = p.E; a.N = p.N; a.hl = p.hl; a.hw = p.hw;
    a.grid = h->grid; a.block = h->block; a.ttc_below = h->cfg.ttc_below;
    a.groups = h->groups.args(h->cfg.G); a.flags = flags; a.ttc = ttc; a.last = h->last; a.mask = h->mask; a.maps = h->maps; a.scene_records = h->scene_records;
    return a;
}

extern "C" int copo_field_create(copo_sim* sim, const copo_field_cfg* cfg, copo_field** out) {
    if (!sim || !cfg || !out) return fail(COPO_ERR_NULL, "copo_field_create: NULL argument");
    *out = nullptr;
    static_assert(COPO_FIELD_LAYERS == FIELD_LAYERS && COPO_FIELD_MAX_SIDE == FIELD_MAX_SIDE && COPO_FIELD_MAX_GROUPS == FIELD_MAX_GROUPS,
                  "copo_hip.h / field_common.h");
    if (cfg->G < 1 || cfg->G > FIELD_MAX_GROUPS) return fail(COPO_ERR_DIM, "copo_field_create: G=%d (1..%d)", cfg->G, FIELD_MAX_GROUPS);
    GridSpec grid;
    if (int rc = make_grid(cfg->x0, cfg->y0, cfg->cell, cfg->W, cfg->H, "copo_field_create", &grid)) return rc;
    if (!(cfg->ttc_below >= 0.0f) || !std::isfinite(cfg->ttc_below))
        return fail(COPO_ERR_CONFIG, "copo_field_create: ttc_below=%g (>= 0, finite)", (double)cfg->ttc_below);
    const size_t E = (size_t)sim->p.E, N = (size_t)sim->p.N;
    // scenes per workgroup of the tile pass: 4 (one per wave) while the scenes are few, up to 64 -- every workgroup ends with one
    // pass over its tile, which more scenes share
    const int32_t block = 4 * (int32_t)std::min<size_t>(std::max<size_t>(E / 1024, 1), 16);
    const size_t n_blocks = (E + block - 1) / block;
    if (n_blocks > 65535) return fail(COPO_ERR_DIM, "copo_field_create: %zu scenes (at most %d)", E, 65535 * 64);
    HIP_TRY(hipSetDevice(sim->device));
    copo_field* h = new (std::nothrow) copo_field();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->sim = sim; h->mem.device = sim->device; h->cfg = *cfg; h->grid = grid; h->block = block; h->n_blocks = (int32_t)n_blocks;
    h->groups.group = h->mem.alloc<int32_t>(E);
    h->last = h->mem.alloc<int32_t>(E * N, 0xff);
    h->mask = h->mem.alloc<uint32_t>(n_blocks * FIELD_MASK_WORDS);
    h->maps = h->mem.alloc<long long>((size_t)cfg->G * FIELD_LAYERS * cfg->H * cfg->W);
    h->scene_records = h->mem.alloc<long long>((size_t)cfg->G);
    return finish_create(h, out, "copo_field_create");
}

extern "C" int copo_field_destroy(copo_field* h) { return destroy_handle(h, "copo_field_destroy"); }

extern "C" int copo_field_set_groups(copo_field* h, const int32_t* group_dev, void* stream) { return GroupTable::set(h, group_dev, stream, "copo_field_set_groups"); }

extern "C" int copo_field_record(copo_field* h, const uint8_t* flags, const float* ttc, int32_t accumulate, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_field_record: NULL handle");
    if (accumulate != 0 && accumulate != 1) return fail(COPO_ERR_DIM, "copo_field_record: accumulate=%d (0 or 1)", accumulate);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const FieldArgs a = field_args(h, flags, ttc);
    if (accumulate) HIP_TRY(h->mask.fill(0, st));
    HIP_TRY(launch_field_events(a, accumulate, st));
    if (accumulate) HIP_TRY(launch_field_tiles(a, st));
    return COPO_OK;
}

extern "C" int copo_field_read(copo_field* h, int64_t* maps_dev, int64_t* scene_records_dev, void* stream) {
    if (!h || (!maps_dev && !scene_records_dev)) return fail(COPO_ERR_NULL, "copo_field_read: NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (maps_dev) HIP_TRY(h->maps.copy_to(maps_dev, st));
    if (scene_records_dev) HIP_TRY(h->scene_records.copy_to(scene_records_dev, st));
    return COPO_OK;
}

extern "C" int copo_field_forget(copo_field* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_field_forget: NULL handle");
    HIP_TRY(h->last.fill(0xff, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_field_reset(copo_field* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_field_reset: NULL handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(h->maps.fill(0, st));
    HIP_TRY(h->scene_records.fill(0, st));
    HIP_TRY(h->last.fill(0xff, st));
    return COPO_OK;
}

// ---- traffic gates (gate_kernels.hip) --------------------------------------------------------------------------

struct copo_gate {
    copo_sim* sim;
    DevPool mem;
    copo_gate_cfg cfg;
    GateLayout at;
    int32_t n_records;                     // records since create / reset (host side: eager only)
    DevBuf<float4> gates;                  // [L]
    DevBuf<int2> sections;                 // [S]
    GroupTable groups;
    DevBuf<uint32_t> mem_x, mem_y;         // [E][N]
    DevBuf<int32_t> mem_aid;               // [E][N]
    DevBuf<int32_t> mem_episode;           // [E]
    DevBuf<unsigned long long> mem_valid;  // [E]
    DevBuf<int32_t> last_fwd;              // [E][L]
    DevBuf<int32_t> entry;                 // [E][S][N]
    DevBuf<long long> acc;                 // [at.words]
};

// the slot memory, last_fwd and entry: nothing is followed, nothing crossed
static hipError_t gate_forget(copo_gate* h, hipStream_t st) {
    hipError_t err = h->mem_valid.fill(0, st);
    if (err == hipSuccess) err = h->last_fwd.fill(0xff, st);
    if (err == hipSuccess) err = h->entry.fill(0xff, st);
    return err;
}

extern "C" int copo_gate_create(copo_sim* sim, const copo_gate_cfg* cfg, const float* gates, const int32_t* sections, copo_gate** out) {
    if (!sim || !cfg || !gates || !out || (cfg && cfg->S > 0 && !sections)) return fail(COPO_ERR_NULL, "copo_gate_create: NULL argument");
    *out = nullptr;
    static_assert(COPO_GATE_MAX_GATES == GATE_MAX_GATES && COPO_GATE_MAX_SECTIONS == GATE_MAX_SECTIONS && COPO_GATE_MAX_GROUPS == GATE_MAX_GROUPS &&
                  COPO_GATE_MAX_BINS == GATE_MAX_BINS && COPO_GATE_MAX_HIST == GATE_MAX_HIST, "copo_hip.h / gate_common.h");
    if (cfg->L < 1 || cfg->L > GATE_MAX_GATES || cfg->S < 0 || cfg->S > GATE_MAX_SECTIONS || cfg->G < 1 || cfg->G > GATE_MAX_GROUPS ||
        cfg->T < 1 || cfg->T > GATE_MAX_BINS || cfg->bin_records < 1 || cfg->HB < 1 || cfg->HB > GATE_MAX_HIST || cfg->TB < 1 ||
        cfg->TB > GATE_MAX_HIST || cfg->tt_bin < 1)
        return fail(COPO_ERR_DIM, "copo_gate_create: L=%d (1..%d) S=%d (0..%d) G=%d (1..%d) T=%d (1..%d) bin_records=%d (>= 1) HB=%d TB=%d (1..%d) tt_bin=%d (>= 1)",
                    cfg->L, GATE_MAX_GATES, cfg->S, GATE_MAX_SECTIONS, cfg->G, GATE_MAX_GROUPS, cfg->T, GATE_MAX_BINS, cfg->bin_records, cfg->HB,
                    cfg->TB, GATE_MAX_HIST, cfg->tt_bin);
    for (int s = 0; s < cfg->S; ++s)
        if (sections[2 * s] < 0 || sections[2 * s] >= cfg->L || sections[2 * s + 1] < 0 || sections[2 * s + 1] >= cfg->L)
            return fail(COPO_ERR_DIM, "copo_gate_create: section %d = (%d, %d): gate indices are 0..%d", s, sections[2 * s], sections[2 * s + 1], cfg->L - 1);
    for (int l = 0; l < cfg->L; ++l) {
        const float* q = gates + 4 * l;
        if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2]) || !std::isfinite(q[3]) || (q[0] == q[2] && q[1] == q[3]))
            return fail(COPO_ERR_CONFIG, "copo_gate_create: gate %d = (%g, %g) -> (%g, %g): finite, A != B", l, (double)q[0], (double)q[1], (double)q[2],
                        (double)q[3]);
    }
    const size_t E = (size_t)sim->p.E, N = (size_t)sim->p.N, L = (size_t)cfg->L, S = (size_t)cfg->S;
    HIP_TRY(hipSetDevice(sim->device));
    copo_gate* h = new (std::nothrow) copo_gate();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->sim = sim; h->mem.device = sim->device; h->cfg = *cfg; h->n_records = 0;
    h->at = gate_layout(cfg->G, cfg->L, cfg->S, cfg->T, cfg->HB, cfg->TB);
    h->gates = h->mem.upload(reinterpret_cast<const float4*>(gates), L);
    h->sections = h->mem.upload(reinterpret_cast<const int2*>(sections), S);
    h->groups.group = h->mem.alloc<int32_t>(E);
    h->mem_x = h->mem.alloc<uint32_t>(E * N);
    h->mem_y = h->mem.alloc<uint32_t>(E * N);
    h->mem_aid = h->mem.alloc<int32_t>(E * N);
    h->mem_episode = h->mem.alloc<int32_t>(E);
    h->mem_valid = h->mem.alloc<unsigned long long>(E);
    h->last_fwd = h->mem.alloc<int32_t>(E * L, 0xff);
    h->entry = h->mem.alloc<int32_t>(E * S * N, 0xff);         // (no section: never indexed)
    h->acc = h->mem.alloc<long long>((size_t)h->at.words);
    return finish_create(h, out, "copo_gate_create");
}

extern "C" int copo_gate_destroy(copo_gate* h) { return destroy_handle(h, "copo_gate_destroy"); }

extern "C" int copo_gate_set_groups(copo_gate* h, const int32_t* group_dev, void* stream) { return GroupTable::set(h, group_dev, stream, "copo_gate_set_groups"); }

extern "C" int copo_gate_record(copo_gate* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_gate_record: NULL handle");
    if (h->n_records == INT32_MAX) return fail(COPO_ERR_STATE, "copo_gate_record: %d records made; reset the handle", h->n_records);
    const SimParams& p = h->sim->p;
    GateArgs a;
    a.state = p.state; a.env = p.env; a.E = p.E; a.N = p.N;
    a.L = h->cfg.L; a.S = h->cfg.S; a.G = h->cfg.G; a.T = h->cfg.T; a.HB = h->cfg.HB; a.TB = h->cfg.TB; a.tt_bin = h->cfg.tt_bin;
    a.r = h->n_records; a.tbin = std::min(h->n_records / h->cfg.bin_records, h->cfg.T - 1);
    a.gates = h->gates; a.sections = h->sections; a.group = h->groups.group;
    a.mem_x = h->mem_x; a.mem_y = h->mem_y; a.mem_aid = h->mem_aid; a.mem_episode = h->mem_episode; a.mem_valid = h->mem_valid;
    a.last_fwd = h->last_fwd; a.entry = h->entry; a.acc = h->acc; a.at = h->at;
    HIP_TRY(launch_gate_record(a, static_cast<hipStream_t>(stream)));
    h->n_records += 1;
    return COPO_OK;
}

extern "C" int64_t copo_gate_words(const copo_gate_cfg* cfg) {
    if (!cfg) return 0;
    return gate_layout(cfg->G, cfg->L, cfg->S, cfg->T, cfg->HB, cfg->TB).words;
}

extern "C" int copo_gate_read(copo_gate* h, int64_t* acc_dev, int32_t* n_records, void* stream) {
    if (!h || (!acc_dev && !n_records)) return fail(COPO_ERR_NULL, "copo_gate_read: NULL argument");
    if (acc_dev) HIP_TRY(h->acc.copy_to(acc_dev, static_cast<hipStream_t>(stream)));
    if (n_records) *n_records = h->n_records;
    return COPO_OK;
}

extern "C" int copo_gate_forget(copo_gate* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_gate_forget: NULL handle");
    HIP_TRY(gate_forget(h, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_gate_reset(copo_gate* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_gate_reset: NULL handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(gate_forget(h, st));
    HIP_TRY(h->acc.fill(0, st));
    h->n_records = 0;
    return COPO_OK;
}

// ---- row pool of the trip log, the conflict log and the encroachment log (rowlog_common.h) --------------------------------------------

// Host side of a log's pool: the record count, the three buffers and the calls that are the same for every log.  `who` is the entry
// point's name for the error string.
struct RowPool {
    int32_t max_rows = 0;
    int32_t n_records = 0;                 // records since create / reset (host side: eager only)
    DevBuf<int32_t> base;                  // [E]
    DevBuf<long long> counters;            // [ROWLOG_COUNTERS]
    DevBuf<uint32_t> pool;                 // [max_rows][ROWLOG_WORDS]

    static int check(int32_t max_rows, const char* who) {
        return max_rows < 1 ? fail(COPO_ERR_DIM, "%s: max_rows=%d (>= 1)", who, max_rows) : COPO_OK;
    }

    void create(DevPool& mem, size_t E, int32_t rows) {
        max_rows = rows;
        base = mem.alloc<int32_t>(E);
        counters = mem.alloc<long long>(ROWLOG_COUNTERS);
        pool = mem.alloc<uint32_t>((size_t)rows * ROWLOG_WORDS);
    }

    RowPoolArgs args() const { return RowPoolArgs{max_rows, base, counters, pool}; }

    // COPO_OK while the next record still has a number
    int can_record(const char* who) const {
        return n_records == INT32_MAX ? fail(COPO_ERR_STATE, "%s: %d records made; reset the handle", who, n_records) : COPO_OK;
    }

    int count(int64_t* out, void* stream) const {
        hipStream_t st = static_cast<hipStream_t>(stream);
        long long c[ROWLOG_COUNTERS];
        HIP_TRY(hipMemcpyAsync(c, counters, sizeof(c), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        out[0] = c[RL_ROWS];
        out[1] = c[RL_DROPPED];
        return COPO_OK;
    }

    int read(int32_t first, int32_t n, int32_t* rows_out, void* stream, const char* who) const {
        if (first < 0 || n < 0 || (int64_t)first + n > max_rows)
            return fail(COPO_ERR_DIM, "%s: rows [%d, %d + %d) of a pool of %d", who, first, first, n, max_rows);
        if (n == 0) return COPO_OK;
        if (!rows_out) return fail(COPO_ERR_NULL, "%s: NULL output", who);
        HIP_TRY(hipMemcpyAsync(rows_out, pool.p + (size_t)first * ROWLOG_WORDS, (size_t)n * ROWLOG_WORDS * 4, hipMemcpyDeviceToDevice,
                               static_cast<hipStream_t>(stream)));
        return COPO_OK;
    }

    // (the rows need no clearing: nothing reads beyond n_rows)
    int clear(void* stream) const {
        HIP_TRY(counters.fill(0, static_cast<hipStream_t>(stream)));
        return COPO_OK;
    }

    int reset(void* stream) {
        HIP_TRY(counters.fill(0, static_cast<hipStream_t>(stream)));
        HIP_TRY(pool.fill(0, static_cast<hipStream_t>(stream)));
        n_records = 0;
        return COPO_OK;
    }
};

static int null_handle(const char* who) { return fail(COPO_ERR_NULL, "%s: NULL handle", who); }

// ---- trip log (trip_kernels.hip) -------------------------------------------------------------------------------

struct copo_trip {
    copo_sim* sim;
    DevPool mem;
    copo_trip_cfg cfg;
    RowPool rows;
    DevBuf<unsigned long long> open;       // [E]
    DevBuf<int32_t> episode;               // [E]
    DevBuf<uint32_t> slots;                // [TRIP_MEM_WORDS][E][N]
    DevBuf<unsigned long long> closing;    // [E]
    DevBuf<uint32_t> endw;                 // [E][N]
};

static TripArgs trip_args(const copo_trip* h) {
    const SimParams& p = h->sim->p;
    TripArgs a;
    a.state = p.state; a.env = p.env; a.E = p.E; a.N = p.N;
    a.r = h->rows.n_records; a.stop_speed = h->cfg.stop_speed;
    a.flags = nullptr; a.rew = nullptr; a.gap = nullptr; a.ttc = nullptr;
    a.open = h->open; a.episode = h->episode; a.mem = h->slots; a.closing = h->closing; a.endw = h->endw; a.rows = h->rows.args();
    return a;
}

extern "C" int copo_trip_create(copo_sim* sim, const copo_trip_cfg* cfg, copo_trip** out) {
    if (!sim || !cfg || !out) return fail(COPO_ERR_NULL, "copo_trip_create: NULL argument");
    *out = nullptr;
    static_assert(COPO_TRIP_WORDS == ROWLOG_WORDS && COPO_TRIP_DONE == TRIP_KIND_DONE && COPO_TRIP_VANISHED == TRIP_KIND_VANISHED &&
                  COPO_TRIP_FLUSHED == TRIP_KIND_FLUSH, "copo_hip.h / trip_common.h");
    if (int rc = RowPool::check(cfg->max_rows, "copo_trip_create")) return rc;
    if (!(cfg->stop_speed >= 0.0f) || !std::isfinite(cfg->stop_speed))
        return fail(COPO_ERR_CONFIG, "copo_trip_create: stop_speed=%g (>= 0, finite)", (double)cfg->stop_speed);
    const size_t E = (size_t)sim->p.E, N = (size_t)sim->p.N;
    HIP_TRY(hipSetDevice(sim->device));
    copo_trip* h = new (std::nothrow) copo_trip();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->sim = sim; h->mem.device = sim->device; h->cfg = *cfg;
    h->open = h->mem.alloc<unsigned long long>(E);
    h->episode = h->mem.alloc<int32_t>(E);
    h->slots = h->mem.alloc<uint32_t>((size_t)TRIP_MEM_WORDS * E * N);
    h->closing = h->mem.alloc<unsigned long long>(E);
    h->endw = h->mem.alloc<uint32_t>(E * N);
    h->rows.create(h->mem, E, cfg->max_rows);
    return finish_create(h, out, "copo_trip_create");
}

extern "C" int copo_trip_destroy(copo_trip* h) { return destroy_handle(h, "copo_trip_destroy"); }

extern "C" int copo_trip_record(copo_trip* h, const uint8_t* flags, const float* rew, const float* gap, const float* ttc, void* stream) {
    if (!h) return null_handle("copo_trip_record");
    if (int rc = h->rows.can_record("copo_trip_record")) return rc;
    TripArgs a = trip_args(h);
    a.flags = flags; a.rew = rew; a.gap = gap; a.ttc = ttc;
    HIP_TRY(launch_trip_record(a, static_cast<hipStream_t>(stream)));
    h->rows.n_records += 1;
    return COPO_OK;
}

extern "C" int copo_trip_flush(copo_trip* h, void* stream) {
    if (!h) return null_handle("copo_trip_flush");
    HIP_TRY(launch_trip_flush(trip_args(h), static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_trip_count(copo_trip* h, int64_t* out, void* stream) {
    return h && out ? h->rows.count(out, stream) : fail(COPO_ERR_NULL, "copo_trip_count: NULL argument");
}

extern "C" int copo_trip_read(copo_trip* h, int32_t first, int32_t n, int32_t* rows_out, void* stream) {
    return h ? h->rows.read(first, n, rows_out, stream, "copo_trip_read") : null_handle("copo_trip_read");
}

extern "C" int copo_trip_clear(copo_trip* h, void* stream) { return h ? h->rows.clear(stream) : null_handle("copo_trip_clear"); }

// (the slot memory needs no clearing: a slot is written when its trip opens)
extern "C" int copo_trip_reset(copo_trip* h, void* stream) {
    if (!h) return null_handle("copo_trip_reset");
    HIP_TRY(h->open.fill(0, static_cast<hipStream_t>(stream)));
    return h->rows.reset(stream);
}

// ---- conflict log (conflict_kernels.hip) -----------------------------------------------------------------------

struct copo_conflict {
    copo_sim* sim;
    DevPool mem;
    copo_conflict_cfg cfg;
    float r2_in, r2_out;                   // radius^2, leave_radius^2, rounded once
    RowPool rows;
    DevBuf<unsigned long long> open;       // [E][N]
    DevBuf<int32_t> aid;                   // [E][N]
    DevBuf<int32_t> episode;               // [E]
    DevBuf<uint32_t> pairs;                // [E][N (N - 1) / 2][CONFLICT_PAIR_WORDS]
    DevBuf<unsigned long long> closing;    // [E][N]
    DevBuf<int32_t> n_closing;             // [E]
};

static ConflictArgs conflict_args(const copo_conflict* h) {
    const SimParams& p = h->sim->p;
    ConflictArgs a;
    a.state = p.state; a.env = p.env; a.E = p.E; a.N = p.N;
    a.r = h->rows.n_records; a.r2_in = h->r2_in; a.r2_out = h->r2_out;
    a.flags = nullptr;
    a.open = h->open; a.aid = h->aid; a.episode = h->episode; a.pairs = h->pairs; a.closing = h->closing; a.n_closing = h->n_closing;
    a.rows = h->rows.args();
    return a;
}

extern "C" int copo_conflict_create(copo_sim* sim, const copo_conflict_cfg* cfg, copo_conflict** out) {
    if (!sim || !cfg || !out) return fail(COPO_ERR_NULL, "copo_conflict_create: NULL argument");
    *out = nullptr;
    static_assert(COPO_CONFLICT_WORDS == ROWLOG_WORDS && COPO_CONFLICT_DONE == CONFLICT_KIND_DONE && COPO_CONFLICT_VANISHED == CONFLICT_KIND_VANISHED &&
                  COPO_CONFLICT_PARTED == CONFLICT_KIND_PARTED && COPO_CONFLICT_FLUSHED == CONFLICT_KIND_FLUSH, "copo_hip.h / conflict_common.h");
    if (int rc = RowPool::check(cfg->max_rows, "copo_conflict_create")) return rc;
    const float r2_in = (float)((double)cfg->radius * (double)cfg->radius), r2_out = (float)((double)cfg->leave_radius * (double)cfg->leave_radius);
    if (!std::isfinite(cfg->radius) || !std::isfinite(cfg->leave_radius) || !(cfg->radius > 0.0f) || !(cfg->leave_radius >= cfg->radius) ||
        !std::isfinite(r2_out))
        return fail(COPO_ERR_CONFIG, "copo_conflict_create: radius=%g (> 0) leave_radius=%g (>= radius), both and their squares finite",
                    (double)cfg->radius, (double)cfg->leave_radius);
    const size_t E = (size_t)sim->p.E, N = (size_t)sim->p.N;
    HIP_TRY(hipSetDevice(sim->device));
    copo_conflict* h = new (std::nothrow) copo_conflict();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->sim = sim; h->mem.device = sim->device; h->cfg = *cfg; h->r2_in = r2_in; h->r2_out = r2_out;
    h->open = h->mem.alloc<unsigned long long>(E * N);
    h->aid = h->mem.alloc<int32_t>(E * N);
    h->episode = h->mem.alloc<int32_t>(E);
    h->pairs = h->mem.alloc<uint32_t>(E * (N * (N - 1) / 2) * CONFLICT_PAIR_WORDS);       // (one slot: never indexed)
    h->closing = h->mem.alloc<unsigned long long>(E * N);
    h->n_closing = h->mem.alloc<int32_t>(E);
    h->rows.create(h->mem, E, cfg->max_rows);
    return finish_create(h, out, "copo_conflict_create");
}

extern "C" int copo_conflict_destroy(copo_conflict* h) { return destroy_handle(h, "copo_conflict_destroy"); }

extern "C" int copo_conflict_record(copo_conflict* h, const uint8_t* flags, void* stream) {
    if (!h) return null_handle("copo_conflict_record");
    if (int rc = h->rows.can_record("copo_conflict_record")) return rc;
    ConflictArgs a = conflict_args(h);
    a.flags = flags;
    HIP_TRY(launch_conflict_record(a, static_cast<hipStream_t>(stream)));
    h->rows.n_records += 1;
    return COPO_OK;
}

extern "C" int copo_conflict_flush(copo_conflict* h, void* stream) {
    if (!h) return null_handle("copo_conflict_flush");
    HIP_TRY(launch_conflict_flush(conflict_args(h), static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_conflict_count(copo_conflict* h, int64_t* out, void* stream) {
    return h && out ? h->rows.count(out, stream) : fail(COPO_ERR_NULL, "copo_conflict_count: NULL argument");
}

extern "C" int copo_conflict_read(copo_conflict* h, int32_t first, int32_t n, int32_t* rows_out, void* stream) {
    return h ? h->rows.read(first, n, rows_out, stream, "copo_conflict_read") : null_handle("copo_conflict_read");
}

extern "C" int copo_conflict_clear(copo_conflict* h, void* stream) { return h ? h->rows.clear(stream) : null_handle("copo_conflict_clear"); }

// (the pair and slot memory needs no clearing: it is read only where an encounter is open, and written when one opens)
extern "C" int copo_conflict_reset(copo_conflict* h, void* stream) {
    if (!h) return null_handle("copo_conflict_reset");
    HIP_TRY(h->open.fill(0, static_cast<hipStream_t>(stream)));
    return h->rows.reset(stream);
}

// ---- encroachment log (encroach_kernels.hip) -------------------------------------------------------------------

struct copo_pet {
    copo_sim* sim;
    DevPool mem;
    copo_pet_cfg cfg;
    GridSpec grid;
    RowPool rows;
    GroupTable groups;
    DevBuf<unsigned long long> stamps;     // [E][H][W]
    DevBuf<int32_t> aid;                   // [E][N]
    DevBuf<unsigned long long> met;        // [E][N]
    DevBuf<int32_t> episode, epoch;        // [E]
    DevBuf<long long> hist;                // [G][PET_TYPES][window]
    DevBuf<long long> critical;            // [G][H][W]
    DevBuf<unsigned long long> fresh;      // [E][N]
    DevBuf<int32_t> n_fresh;               // [E]
};

extern "C" int copo_pet_create(copo_sim* sim, const copo_pet_cfg* cfg, copo_pet** out) {
    if (!sim || !cfg || !out) return fail(COPO_ERR_NULL, "copo_pet_create: NULL argument");
    *out = nullptr;
    static_assert(COPO_PET_WORDS == ROWLOG_WORDS && COPO_PET_MAX_WINDOW == PET_MAX_WINDOW && COPO_PET_TYPES == PET_TYPES, "copo_hip.h / encroach_common.h");
    if (int rc = RowPool::check(cfg->max_rows, "copo_pet_create")) return rc;
    if (cfg->G < 1 || cfg->G > GRID_MAX_GROUPS || cfg->window < 1 || cfg->window > PET_MAX_WINDOW || cfg->critical_records < 0)
        return fail(COPO_ERR_DIM, "copo_pet_create: G=%d (1..%d) window=%d (1..%d) critical_records=%d (>= 0)", cfg->G, GRID_MAX_GROUPS, cfg->window,
                    PET_MAX_WINDOW, cfg->critical_records);
    GridSpec grid;
    if (int rc = make_grid(cfg->x0, cfg->y0, cfg->cell, cfg->W, cfg->H, "copo_pet_create", &grid)) return rc;
    // a wider cell lets a body pass between cell centres
    const double widest = 2.0 * (double)sim->p.hw / std::sqrt(2.0);
    if (!((double)cfg->cell <= widest))
        return fail(COPO_ERR_CONFIG, "copo_pet_create: cell=%g m is wider than 2 hw / sqrt(2) = %g m: a body could pass between cell centres",
                    (double)cfg->cell, widest);
    const size_t E = (size_t)sim->p.E, N = (size_t)sim->p.N, HW = (size_t)cfg->H * cfg->W;
    HIP_TRY(hipSetDevice(sim->device));
    copo_pet* h = new (std::nothrow) copo_pet();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->sim = sim; h->mem.device = sim->device; h->cfg = *cfg; h->grid = grid;
    h->groups.group = h->mem.alloc<int32_t>(E);
    h->stamps = h->mem.alloc<unsigned long long>(E * HW);
    h->aid = h->mem.alloc<int32_t>(E * N);
    h->met = h->mem.alloc<unsigned long long>(E * N);
    h->episode = h->mem.alloc<int32_t>(E);
    h->epoch = h->mem.alloc<int32_t>(E);
    h->hist = h->mem.alloc<long long>((size_t)cfg->G * PET_TYPES * cfg->window);
    h->critical = h->mem.alloc<long long>((size_t)cfg->G * HW);
    h->fresh = h->mem.alloc<unsigned long long>(E * N);
    h->n_fresh = h->mem.alloc<int32_t>(E);
    h->rows.create(h->mem, E, cfg->max_rows);
    return finish_create(h, out, "copo_pet_create");
}

extern "C" int copo_pet_destroy(copo_pet* h) { return destroy_handle(h, "copo_pet_destroy"); }

extern "C" int copo_pet_set_groups(copo_pet* h, const int32_t* group_dev, void* stream) { return GroupTable::set(h, group_dev, stream, "copo_pet_set_groups"); }

extern "C" int copo_pet_record(copo_pet* h, void* stream) {
    if (!h) return null_handle("copo_pet_record");
    if (int rc = h->rows.can_record("copo_pet_record")) return rc;
    const SimParams& p = h->sim->p;
    PetArgs a;
    a.state = p.state; a.env = p.env; a.E = p.E; a.N = p.N; a.r = h->rows.n_records; a.hl = p.hl; a.hw = p.hw;
    a.grid = h->grid; a.window = h->cfg.window; a.critical_records = h->cfg.critical_records;
    a.groups = h->groups.args(h->cfg.G); a.stamps = h->stamps; a.aid = h->aid; a.met = h->met; a.episode = h->episode; a.epoch = h->epoch;
    a.hist = h->hist; a.critical = h->critical; a.fresh = h->fresh; a.n_fresh = h->n_fresh; a.rows = h->rows.args();
    HIP_TRY(launch_pet_record(a, static_cast<hipStream_t>(stream)));
    h->rows.n_records += 1;
    return COPO_OK;
}

extern "C" int copo_pet_forget(copo_pet* h, void* stream) {
    if (!h) return null_handle("copo_pet_forget");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(h->met.fill(0, st));
    HIP_TRY(launch_pet_forget(h->epoch, h->sim->p.E, h->rows.n_records, st));
    return COPO_OK;
}

extern "C" int copo_pet_count(copo_pet* h, int64_t* out, void* stream) {
    return h && out ? h->rows.count(out, stream) : fail(COPO_ERR_NULL, "copo_pet_count: NULL argument");
}

extern "C" int copo_pet_read(copo_pet* h, int32_t first, int32_t n, int32_t* rows_out, void* stream) {
    return h ? h->rows.read(first, n, rows_out, stream, "copo_pet_read") : null_handle("copo_pet_read");
}

extern "C" int copo_pet_aggregates(copo_pet* h, int64_t* hist_dev, int64_t* critical_dev, void* stream) {
    if (!h || (!hist_dev && !critical_dev)) return fail(COPO_ERR_NULL, "copo_pet_aggregates: NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hist_dev) HIP_TRY(h->hist.copy_to(hist_dev, st));
    if (critical_dev) HIP_TRY(h->critical.copy_to(critical_dev, st));
    return COPO_OK;
}

extern "C" int copo_pet_memory(copo_pet* h, uint64_t* grid_dev, uint64_t* met_dev, void* stream) {
    if (!h || (!grid_dev && !met_dev)) return fail(COPO_ERR_NULL, "copo_pet_memory: NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (grid_dev) HIP_TRY(h->stamps.copy_to(grid_dev, st));
    if (met_dev) HIP_TRY(h->met.copy_to(met_dev, st));
    return COPO_OK;
}

extern "C" int copo_pet_clear(copo_pet* h, void* stream) { return h ? h->rows.clear(stream) : null_handle("copo_pet_clear"); }

extern "C" int copo_pet_reset(copo_pet* h, void* stream) {
    if (!h) return null_handle("copo_pet_reset");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(h->stamps.fill(0, st));
    HIP_TRY(h->aid.fill(0, st));
    HIP_TRY(h->met.fill(0, st));
    HIP_TRY(h->episode.fill(0, st));
    HIP_TRY(h->epoch.fill(0, st));
    HIP_TRY(h->hist.fill(0, st));
    HIP_TRY(h->critical.fill(0, st));
    return h->rows.reset(stream);
}
