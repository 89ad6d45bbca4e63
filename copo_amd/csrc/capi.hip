// C ABI of libcopo_hip.so (include/copo_hip.h): argument validation, handle lifetime, error strings.
// No torch types; all launches are asynchronous on the caller's stream.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <algorithm>
#include <vector>

#include <array>
#include <cmath>
#include <set>

#include "sim_common.h"
#include "render_common.h"
#include "interact_common.h"
#include "clip_common.h"
#include "rewind_common.h"
#include "field_common.h"
#include "gate_common.h"

using namespace copo;

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(COPO_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

struct copo_sim {
    SimParams p;
    SimParams* p_dev;          // device copy of p (the kernels' parameter block)
    int device;
    int block;
    bool started;
    double lcf_mean, lcf_std, force_lcf;
    int capacity;              // active agent slots (curriculum), num_agents by default
    float lcf_host[4];         // {mean, std, capacity, 0}: what the kernels read from p.lcf_dist
    bool lcf_dirty;
    std::vector<void*> allocs;
    // host copies of the map tables for copo_render_create: road records [n_routes][seg_rows][COPO_SEG_STRIDE], route_meta,
    // lane lines (on the device only when a detector reads them) and static boxes
    std::vector<float> h_segs, h_meta, h_lines, h_boxes;
    bool boxes_hidden;
};

extern "C" int copo_version(void) { return COPO_ABI_VERSION; }
#define COPO_STR2(x) #x
#define COPO_STR(x) COPO_STR2(x)
extern "C" const char* copo_build_info(void) {
#ifdef COPO_PROFILE_SKIP
    return "libcopo_hip ABI " COPO_STR(COPO_ABI_VERSION) ", gfx950, PROFILING build (COPO_PROFILE_SKIP=" COPO_STR(COPO_PROFILE_SKIP)
           "): phases may be compiled out, results may be wrong; reads COPO_ROWPASS_4X4 COPO_ROWPASS_RT8 COPO_WGRAD_OT COPO_FUSED_WGRAD COPO_FUSED_ROWPASS COPO_RP_DBG";
#else
    return "libcopo_hip ABI " COPO_STR(COPO_ABI_VERSION) ", gfx950, shipped build: all phases compiled in, no environment variable is read";
#endif
}
extern "C" const char* copo_last_error(void) { return g_err; }

template <typename T>
static int upload(copo_sim* s, const T* host, size_t count, const T** dev) {
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, count * sizeof(T) ? count * sizeof(T) : sizeof(T)));
    s->allocs.push_back(d);
    if (count) HIP_TRY(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    *dev = static_cast<const T*>(d);
    return COPO_OK;
}

// measured (scripts/bench_sim.py, 40 slots, populated scenes): up to one scene per CU -> 16 waves per scene; two per CU -> 8;
// then 4; from ~12 scenes per CU on, ONE wave per scene with the small LDS footprint (sim_shape_params, ~20 scenes resident
// per CU) and the register formulation of the neighbour lists (round 3: 4096 scenes 124 -> 110 us, 8192 222 -> 173 us; at
// 2048 four waves per scene still win, 72 vs 96 us)
// (`nbr_fast` = the register formulation of the neighbour lists can run, SimParams::nbr_fast: without it -- K > 8, a mean-field
// range of 0 or beyond the radius -- one wave per scene only pays above 8192 scenes, as before that formulation existed)
// Above that: the PACKED shape (sim_packed.hip: several scenes per workgroup, the per-agent phases dense over the lanes) wherever
// the configuration allows it (`packed` = scenes per workgroup, 0: not available), else one wave per scene.  Returned as -scenes.
static int pick_block(int E, bool nbr_fast = true, int packed = 0) {
    if (E <= 256) return 1024;
    if (E <= 512) return 512;
    if (E <= (nbr_fast ? 3072 : 8192)) return 256;
    return packed > 0 ? -packed : 64;
}
// (measured, 16 384 populated scenes, scripts/bench_sim.py, 4 scenes per workgroup against one wave per scene: 8 slots 62.7 / 66.0 us, 12 78.8 /
// 87.9, 16 90.9 / 99.6, 20 109.1 / 115.8, 10 slots x 240 beams 109 / 124 (fans of 5); with 40 slots the packed shape issues 9 % fewer vector
// instructions but ends behind, 209 vs 193 us: parked waves, barriers.  With detector beams (Bottleneck, 20 slots: 332 / 290 us) one wave
// per scene is ahead; 24 slots 127.9 / 134.2, 30 slots 154.7 / 161.3, 40 slots 207.9 / 204.4: automatic up to 32 slots on maps without
// detector beams)
static int packed_scenes(const SimParams& p) {
    return (p.N <= 32 && p.side_lasers == 0 && p.lane_lasers == 0 && sim_packed_supported(p)) ? sim_packed_default_scenes(p) : 0;
}

extern "C" int copo_sim_create(const copo_sim_cfg* cfg, int device, copo_sim** out) {
    if (!cfg || !out) return fail(COPO_ERR_NULL, "copo_sim_create: cfg/out is NULL");
    *out = nullptr;
    if (cfg->num_envs < 1 || cfg->num_agents < 1 || cfg->num_agents > COPO_MAX_AGENTS)
        return fail(COPO_ERR_DIM, "num_envs=%d num_agents=%d (agents must be 1..%d)", cfg->num_envs, cfg->num_agents,
                    COPO_MAX_AGENTS);
    if (cfg->num_lasers < 1 || cfg->num_lasers > COPO_MAX_LASERS)
        return fail(COPO_ERR_DIM, "num_lasers=%d out of 1..%d", cfg->num_lasers, COPO_MAX_LASERS);
    if (cfg->comm_size < 0 || cfg->comm_size > 64 || (cfg->comm_size > 0 && (cfg->comm_neighbours < 1 || cfg->comm_neighbours > COPO_MAX_AGENTS)))
        return fail(COPO_ERR_CONFIG, "comm_size=%d comm_neighbours=%d", cfg->comm_size, cfg->comm_neighbours);
    if (cfg->add_traffic_light && (cfg->traffic_light_interval < 1 || !(cfg->map_bbox[1] > cfg->map_bbox[0]) || !(cfg->map_bbox[3] > cfg->map_bbox[2])))
        return fail(COPO_ERR_CONFIG, "add_traffic_light needs traffic_light_interval >= 1 and a non-empty map_bbox");
    if (cfg->side_lasers < 0 || cfg->side_lasers > COPO_MAX_LASERS || cfg->lane_line_lasers < 0 || cfg->lane_line_lasers > COPO_MAX_LASERS)
        return fail(COPO_ERR_DIM, "side_lasers=%d lane_line_lasers=%d out of 0..%d", cfg->side_lasers, cfg->lane_line_lasers, COPO_MAX_LASERS);
    if ((cfg->navi_dim != 0 && cfg->navi_dim != COPO_NAVI_DIM) || (cfg->toll_dim != 0 && cfg->toll_dim != 2))
        return fail(COPO_ERR_CONFIG, "navi_dim=%d (0 or %d) toll_dim=%d (0 or 2)", cfg->navi_dim, COPO_NAVI_DIM, cfg->toll_dim);
    const int O = COPO_OBS_DIM(cfg);
    if (cfg->obs_dim != O) return fail(COPO_ERR_DIM, "obs_dim=%d but the configured blocks add up to %d (COPO_OBS_DIM)", cfg->obs_dim, O);
    if (cfg->nbr_k < 1 || cfg->nbr_k > COPO_MAX_AGENTS) return fail(COPO_ERR_DIM, "nbr_k=%d out of 1..64", cfg->nbr_k);
    if (cfg->n_routes < 1 || cfg->n_routes > COPO_MAX_ROUTES || cfg->n_spawns < cfg->num_agents ||
        cfg->n_spawns > COPO_MAX_SPAWNS)
        return fail(COPO_ERR_CONFIG, "n_routes=%d n_spawns=%d (need num_agents <= n_spawns <= %d)", cfg->n_routes,
                    cfg->n_spawns, COPO_MAX_SPAWNS);
    if (!cfg->route_segs || !cfg->route_meta || !cfg->spawn_tab || !cfg->spawn_s || !cfg->ray_cs)
        return fail(COPO_ERR_NULL, "copo_sim_create: a map table pointer is NULL");
    if (cfg->n_boxes < 0 || cfg->n_boxes > COPO_MAX_BOXES || (cfg->n_boxes > 0 && !cfg->boxes))
        return fail(COPO_ERR_CONFIG, "static boxes: n_boxes=%d (max %d) needs the table", cfg->n_boxes, COPO_MAX_BOXES);
    if (cfg->n_lines < 0 || cfg->n_lines > COPO_MAX_LINES ||
        ((cfg->side_lasers || cfg->lane_line_lasers) && (!cfg->lines || (cfg->side_lasers && !cfg->side_cs) || (cfg->lane_line_lasers && !cfg->lane_line_cs))))
        return fail(COPO_ERR_CONFIG, "detectors need the line table and their beam tables (n_lines=%d, max %d)", cfg->n_lines, COPO_MAX_LINES);
    if (cfg->substeps < 1 || cfg->horizon < 1 || cfg->horizon > 65535 || cfg->respawn_cooldown < 0 || cfg->respawn_cooldown > 255 ||
        cfg->delay_done < 0 || cfg->delay_done > 255)
        return fail(COPO_ERR_CONFIG, "substeps >= 1, 1 <= horizon <= 65535, 0 <= respawn_cooldown, delay_done <= 255");
    if (!(cfg->lcf_std > 0.0) || cfg->lcf_mean < -1.0 || cfg->lcf_mean > 1.0)
        return fail(COPO_ERR_CONFIG, "lcf_mean must be in [-1,1] and lcf_std > 0 (env_wrappers.py:195,425-426)");
    for (int r = 0; r < cfg->n_routes; ++r) {
        const int nseg = (int)cfg->route_meta[r * 4 + 1];
        if (nseg < 1 || nseg > COPO_MAX_SEGS) return fail(COPO_ERR_CONFIG, "route %d has %d roads", r, nseg);
        const int space = (int)cfg->route_meta[r * 4 + 3];
        if (space < 0 || space > 32) return fail(COPO_ERR_CONFIG, "route %d: exclusive destination id %d outside 0..32", r, space);
    }
    std::vector<int32_t> safe;
    for (int s = 0; s < cfg->n_spawns; ++s) {
        const int r0 = cfg->spawn_tab[s * 4], nc = cfg->spawn_tab[s * 4 + 1];
        if (r0 < 0 || nc < 1 || r0 + nc > cfg->n_routes) return fail(COPO_ERR_CONFIG, "spawn %d: bad route range", s);
        for (int r = r0; r < r0 + nc; ++r) {
            const float* g = cfg->route_segs + (size_t)r * (COPO_MAX_SEGS + 1) * COPO_SEG_STRIDE;
            if (g[5] != 0.0f || !(cfg->spawn_s[s] < g[4]) || cfg->spawn_tab[s * 4 + 2] < 0 || (float)cfg->spawn_tab[s * 4 + 2] >= floorf(g[COPO_SEG_LANES]))
                return fail(COPO_ERR_CONFIG, "spawn %d must lie on a lane of the straight first road of route %d", s, r);
        }
        if (cfg->spawn_tab[s * 4 + 3]) safe.push_back(s);
    }
    if (safe.empty() || safe.size() > COPO_MAX_SAFE)
        return fail(COPO_ERR_CONFIG, "%zu respawn places (spawn slots marked safe): need 1..%d", safe.size(), COPO_MAX_SAFE);
    copo_sim* s = new (std::nothrow) copo_sim();
    if (!s) return fail(COPO_ERR_DEVICE, "out of host memory");
    s->device = device;
    s->started = false;
    s->lcf_mean = cfg->lcf_mean;
    s->lcf_std = cfg->lcf_std;
    s->force_lcf = -100.0;
    s->capacity = cfg->num_agents;
    s->lcf_dirty = true;
    if (hipSetDevice(device) != hipSuccess) {
        delete s;
        return fail(COPO_ERR_DEVICE, "hipSetDevice(%d) failed", device);
    }
    SimParams& p = s->p;
    memset(&p, 0, sizeof(p));
    p.E = cfg->num_envs; p.N = cfg->num_agents; p.O = cfg->obs_dim; p.K = cfg->nbr_k; p.num_lasers = cfg->num_lasers;
    p.enable_lcf = cfg->enable_lcf; p.horizon = cfg->horizon; p.delay_done = cfg->delay_done;
    p.respawn_cooldown = cfg->respawn_cooldown; p.substeps = cfg->substeps;
    p.n_routes = cfg->n_routes; p.n_spawns = cfg->n_spawns;
    {   // observation row: [side | state | lane | navigation | lasers | toll | traffic light | lcf | messages]
        p.side_lasers = cfg->side_lasers; p.lane_lasers = cfg->lane_line_lasers; p.navi_dim = cfg->navi_dim;
        p.toll_dim = cfg->toll_dim; p.toll_min_steps = cfg->toll_min_steps;
        p.toll_speed_limit = cfg->toll_speed_limit; p.overspeed_penalty = cfg->overspeed_penalty; p.toll_early_exit = cfg->toll_early_exit;
        p.col_state = COPO_SIDE_DIM(cfg);
        p.col_lane = p.col_state + COPO_STATE_DIM;
        p.col_navi = p.col_lane + COPO_LANE_DIM(cfg);
        p.col_lidar = p.col_navi + cfg->navi_dim;
        int col = p.col_lidar + cfg->num_lasers;
        p.col_toll = cfg->toll_dim ? col : -1;
        col += cfg->toll_dim;
        p.col_tl = cfg->add_traffic_light ? col : -1;
        col += cfg->add_traffic_light ? 3 : 0;
        p.col_lcf = cfg->enable_lcf ? col : -1;
        col += cfg->enable_lcf ? 1 : 0;
        p.col_comm = cfg->comm_size > 0 ? col : -1;
        p.act_dim = COPO_ACT_DIM(cfg);
        p.tl_interval = cfg->traffic_light_interval > 0 ? cfg->traffic_light_interval : 1;
        p.comm_size = cfg->comm_size > 0 ? cfg->comm_size : 0;
        p.comm_nb = cfg->comm_size > 0 ? cfg->comm_neighbours : 0;
        p.comm_pos = cfg->add_pos_in_comm ? 1 : 0;
        for (int k = 0; k < 4; ++k) p.bbox[k] = cfg->map_bbox[k];
    }
    p.lidar_range = cfg->lidar_range; p.neighbours_distance = cfg->neighbours_distance; p.mf_distance = cfg->mf_distance;
    {   // neighbours_fast (sim_kernels.hip): conservative fp32 thresholds around the exact fp64 decisions
        const double R2 = (double)cfg->neighbours_distance * (double)cfg->neighbours_distance;
        const double M2 = (double)cfg->mf_distance * (double)cfg->mf_distance;
        p.nbr_r2lo = (float)(R2 * (1.0 - 1e-6));
        p.nbr_r2hi = (float)(R2 * (1.0 + 1e-6));
        const float mlo = (float)(M2 * (1.0 - 1e-5)), mhi = (float)(M2 * (1.0 + 1e-6));
        uint32_t blo, bhi;
        memcpy(&blo, &mlo, 4);
        memcpy(&bhi, &mhi, 4);
        p.mf_key_lo = blo & ~63u;                    // key < lo: inside for certain (keys drop 6 mantissa bits of d^2)
        p.mf_key_hi = (bhi + 63u) & ~63u;            // key >= hi: outside for certain
        // (a mean-field range of exactly 0 stays with the exact formulation: a coincident pair has d = 0 <= 0 there, and the
        // key thresholds of a zero range cannot express it)
        p.nbr_fast = (cfg->nbr_k <= 8 && cfg->neighbours_distance > 0.0f && cfg->mf_distance > 0.0f &&
                      cfg->mf_distance < 0.99f * cfg->neighbours_distance) ? 1 : 0;
    }
    p.dt = cfg->dt; p.hl = cfg->veh_half_len; p.hw = cfg->veh_half_wid; p.wheelbase = cfg->wheelbase;
    p.max_steer = cfg->max_steer; p.max_speed = cfg->max_speed; p.acc_max = cfg->acc_max; p.brake_gain = cfg->brake_gain;
    p.brake_max = cfg->brake_max; p.lat_acc_max = cfg->lat_acc_max; p.reverse_acc = cfg->reverse_acc;
    p.region_hl = 0.5f * cfg->spawn_region_len; p.region_hw = 0.5f * cfg->spawn_region_wid;
    p.driving_reward = cfg->driving_reward; p.speed_reward = cfg->speed_reward; p.success_reward = cfg->success_reward;
    p.crash_penalty = cfg->crash_penalty; p.out_penalty = cfg->out_penalty; p.arrive_margin = cfg->arrive_margin; p.body_margin = cfg->body_margin;
    p.lane_width = cfg->lane_width;
    p.side_range = cfg->side_range; p.lane_range = cfg->lane_line_range;
    // derived constants: single float operations (this file is compiled with -ffp-contract=off), as in the oracle
    p.inv_w = 1.0f / cfg->lane_width;
    p.inv_range = 1.0f / cfg->lidar_range;
    p.inv_vnorm = 1.0f / (cfg->max_speed * 3.6f + 1.0f);
    p.inv_dt = 1.0f / cfg->dt;
    p.inv_side_range = cfg->side_lasers ? 1.0f / cfg->side_range : 0.0f;
    p.inv_lane_range = cfg->lane_line_lasers ? 1.0f / cfg->lane_line_range : 0.0f;
    p.inv_toll = cfg->toll_dim ? 1.0f / (float)(cfg->toll_min_steps > 0 ? cfg->toll_min_steps : 1) : 0.0f;
    p.h_sub = cfg->dt / (float)cfg->substeps;
    p.ray_sign = (cfg->num_lasers > 2 && cfg->ray_cs[3] < 0.0f) ? -1.0f : 1.0f;   // the beam table's sense of rotation
    // detector beams: evenly spaced?  (then a line primitive only meets a WINDOW of them, detector_window in sim_device.h)
    auto even_table = [](const float* cs, int n, float& theta0, float& rpr) {
        theta0 = 0.0f; rpr = 0.0f;
        if (n < 3 || !cs) return;
        const double two_pi = 6.283185307179586;
        const double th0 = std::atan2((double)cs[1], (double)cs[0]);
        double step = std::atan2((double)cs[3], (double)cs[2]) - th0;
        step = step > two_pi / 2 ? step - two_pi : (step < -two_pi / 2 ? step + two_pi : step);
        bool even = std::fabs(std::fabs(step) * n - two_pi) < 1e-3;
        for (int k = 0; k < n && even; ++k) {
            const double want = th0 + k * step;
            even = std::fabs(cs[2 * k] - std::cos(want)) < 1e-4 && std::fabs(cs[2 * k + 1] - std::sin(want)) < 1e-4;
        }
        if (even) { theta0 = (float)th0; rpr = (float)(1.0 / step); }
    };
    even_table(cfg->side_cs, cfg->side_lasers, p.side_theta0, p.side_rpr);
    even_table(cfg->lane_line_cs, cfg->lane_line_lasers, p.lane_theta0, p.lane_rpr);
    p.n_safe = (int32_t)safe.size();
    p.n_spaces = 0;
    for (int r = 0; r < cfg->n_routes; ++r) {
        const int d = (int)cfg->route_meta[r * 4 + 3];
        p.n_spaces = std::max(p.n_spaces, (int32_t)d);
    }
    p.n_lines = (cfg->side_lasers || cfg->lane_line_lasers) ? cfg->n_lines : 0;
    int rc = COPO_OK;
    const size_t EN = (size_t)p.E * p.N;
    void* d = nullptr;
    auto dev_alloc = [&](size_t bytes, void** ptr) -> int {
        hipError_t e = hipMalloc(ptr, bytes);
        if (e != hipSuccess) return fail(COPO_ERR_DEVICE, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
        s->allocs.push_back(*ptr);
        e = hipMemset(*ptr, 0, bytes);
        if (e != hipSuccess) return fail(COPO_ERR_DEVICE, "hipMemset: %s", hipGetErrorString(e));
        return COPO_OK;
    };
    if (rc == COPO_OK && (rc = dev_alloc(COPO_STATE_FIELDS * EN * 4, &d)) == COPO_OK) p.state = (float*)d;
    if (rc == COPO_OK && (rc = dev_alloc((size_t)p.E * 16, &d)) == COPO_OK) p.env = (int32_t*)d;
    if (rc == COPO_OK && (rc = dev_alloc((size_t)p.E * 8, &d)) == COPO_OK) p.seeds = (const uint64_t*)d;
    if (rc == COPO_OK && (rc = dev_alloc(16, &d)) == COPO_OK) p.lcf_dist = (const float*)d;
    if (rc == COPO_OK) {      // device table: only as many road records per route as the longest route needs (+ its terminal record)
        int rows = 2;
        for (int r = 0; r < cfg->n_routes; ++r) rows = std::max(rows, (int)cfg->route_meta[r * 4 + 1] + 1);
        p.seg_rows = rows;
        std::vector<float> compact((size_t)cfg->n_routes * rows * COPO_SEG_STRIDE);
        for (int r = 0; r < cfg->n_routes; ++r)
            memcpy(compact.data() + (size_t)r * rows * COPO_SEG_STRIDE,
                   cfg->route_segs + (size_t)r * (COPO_MAX_SEGS + 1) * COPO_SEG_STRIDE, sizeof(float) * rows * COPO_SEG_STRIDE);
        rc = upload(s, compact.data(), compact.size(), &p.route_segs);
        s->h_segs = std::move(compact);
        s->h_meta.assign(cfg->route_meta, cfg->route_meta + (size_t)cfg->n_routes * 4);
        if (cfg->n_lines > 0 && cfg->lines) s->h_lines.assign(cfg->lines, cfg->lines + (size_t)cfg->n_lines * COPO_LINE_STRIDE);
        if (cfg->n_boxes > 0) s->h_boxes.assign(cfg->boxes, cfg->boxes + (size_t)cfg->n_boxes * COPO_BOX_STRIDE);
        s->boxes_hidden = cfg->boxes_hidden != 0;
    }
    if (rc == COPO_OK) rc = upload(s, cfg->route_meta, (size_t)cfg->n_routes * 4, &p.route_meta);
    if (rc == COPO_OK) rc = upload(s, cfg->spawn_tab, (size_t)cfg->n_spawns * 4, &p.spawn_tab);
    if (rc == COPO_OK) rc = upload(s, cfg->spawn_s, (size_t)cfg->n_spawns, &p.spawn_s);
    if (rc == COPO_OK) rc = upload(s, cfg->ray_cs, (size_t)cfg->num_lasers * 2, &p.ray_cs);
    if (rc == COPO_OK) rc = upload(s, safe.data(), safe.size(), &p.safe_ids);
    if (rc == COPO_OK) {      // pose of every respawn place (sim_kernels.hip spawn_pose, the same float operations in the same order)
        std::vector<float> sp4(4 * std::max<size_t>(safe.size(), 1), 0.0f);
        for (size_t q = 0; q < safe.size(); ++q) {
            const int sp = safe[q];
            const float* g = cfg->route_segs + (size_t)cfg->spawn_tab[sp * 4 + 0] * (COPO_MAX_SEGS + 1) * COPO_SEG_STRIDE;
            const float s0 = cfg->spawn_s[sp];
            const float off = (float)cfg->spawn_tab[sp * 4 + 2] * cfg->lane_width;
            sp4[4 * q + 0] = g[0] + g[2] * s0 + g[3] * off;
            sp4[4 * q + 1] = g[1] + g[3] * s0 - g[2] * off;
            sp4[4 * q + 2] = g[2];
            sp4[4 * q + 3] = g[3];
        }
        rc = upload(s, sp4.data(), sp4.size(), &p.safe_pose);
    }
    if (rc == COPO_OK && p.n_lines) rc = upload(s, cfg->lines, (size_t)cfg->n_lines * COPO_LINE_STRIDE, &p.lines);
    p.n_boxes = cfg->n_boxes;
    p.n_boxes_lidar = cfg->boxes_hidden ? 0 : cfg->n_boxes;
    if (rc == COPO_OK && p.n_boxes) rc = upload(s, cfg->boxes, (size_t)cfg->n_boxes * COPO_BOX_STRIDE, &p.boxes);
    if (rc == COPO_OK && cfg->side_lasers) rc = upload(s, cfg->side_cs, (size_t)cfg->side_lasers * 2, &p.side_cs);
    if (rc == COPO_OK && cfg->lane_line_lasers) rc = upload(s, cfg->lane_line_cs, (size_t)cfg->lane_line_lasers * 2, &p.lane_cs);
    s->block = pick_block(cfg->num_envs, p.nbr_fast != 0, packed_scenes(p));      // (after the observation layout: the packed shape depends on it)
    sim_shape_params(p, s->block);
    if (rc == COPO_OK) {
        const SimParams* pd = nullptr;
        rc = upload(s, &s->p, 1, &pd);
        s->p_dev = const_cast<SimParams*>(pd);
    }
    if (rc != COPO_OK) {
        for (void* a : s->allocs) (void)hipFree(a);
        delete s;
        return rc;
    }
    *out = s;
    return COPO_OK;
}

extern "C" int copo_sim_destroy(copo_sim* s) {
    if (!s) return fail(COPO_ERR_NULL, "copo_sim_destroy: NULL handle");
    (void)hipSetDevice(s->device);
    for (void* a : s->allocs) (void)hipFree(a);
    delete s;
    return COPO_OK;
}

// Push the LCF distribution to device memory on `st` (kernels read it from there, so launches captured
// in a hipGraph keep seeing later updates).  Skipped while the stream is capturing.
static int flush_lcf(copo_sim* s, hipStream_t st) {
    if (!s->lcf_dirty) return COPO_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return COPO_OK;
    s->lcf_host[0] = (float)((s->force_lcf != -100.0) ? s->force_lcf : s->lcf_mean);
    s->lcf_host[1] = (float)s->lcf_std;
    s->lcf_host[2] = (float)s->capacity;
    s->lcf_host[3] = 0.0f;
    HIP_TRY(hipMemcpyAsync(const_cast<float*>(s->p.lcf_dist), s->lcf_host, 16, hipMemcpyHostToDevice, st));
    s->lcf_dirty = false;
    return COPO_OK;
}

extern "C" int copo_sim_flush(copo_sim* s, void* stream) {
    if (!s) return fail(COPO_ERR_NULL, "copo_sim_flush: NULL handle");
    return flush_lcf(s, static_cast<hipStream_t>(stream));
}

extern "C" int copo_sim_set_lcf_dist(copo_sim* s, double mean, double std) {
    if (!s) return fail(COPO_ERR_NULL, "copo_sim_set_lcf_dist: NULL handle");
    if (!(std > 0.0) || mean < -1.0 || mean > 1.0)
        return fail(COPO_ERR_CONFIG, "set_lcf_dist(mean=%g, std=%g): need -1 <= mean <= 1, std > 0", mean, std);
    s->lcf_mean = mean;
    s->lcf_std = std;
    s->lcf_dirty = true;
    return COPO_OK;
}

extern "C" int copo_sim_set_capacity(copo_sim* s, int32_t capacity) {
    if (!s) return fail(COPO_ERR_NULL, "copo_sim_set_capacity: NULL handle");
    if (capacity < 1 || capacity > s->p.N) return fail(COPO_ERR_CONFIG, "capacity=%d not in [1, %d]", capacity, s->p.N);
    s->capacity = capacity;
    s->lcf_dirty = true;
    return COPO_OK;
}

extern "C" int copo_sim_set_force_lcf(copo_sim* s, double v) {
    if (!s) return fail(COPO_ERR_NULL, "copo_sim_set_force_lcf: NULL handle");
    if (v != -100.0 && (v < -1.0 || v > 1.0)) return fail(COPO_ERR_CONFIG, "force_lcf=%g not in [-1,1] (or -100)", v);
    s->force_lcf = v;
    s->lcf_dirty = true;
    return COPO_OK;
}

extern "C" int copo_sim_set_debug(copo_sim* s, int64_t* stamps) {
    if (!s) return fail(COPO_ERR_NULL, "copo_sim_set_debug: NULL handle");
    s->p.dbg = reinterpret_cast<long long*>(stamps);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());         // profiling aid: launches in flight keep the block they started with
    HIP_TRY(hipMemcpy(s->p_dev, &s->p, sizeof(SimParams), hipMemcpyHostToDevice));
    return COPO_OK;
}

extern "C" int copo_sim_set_block(copo_sim* s, int32_t threads) {
    if (!s) return fail(COPO_ERR_NULL, "copo_sim_set_block: NULL handle");
    if (threads == 0) threads = pick_block(s->p.E, s->p.nbr_fast != 0, packed_scenes(s->p));
    if (threads < 0) {        // packed shape: -threads scenes per workgroup (-1: the default count)
        if (!sim_packed_supported(s->p)) return fail(COPO_ERR_CONFIG, "the packed launch shape needs the register formulation of the neighbour lists and no traffic-light / communication block");
        if (threads == -1) threads = -sim_packed_default_scenes(s->p);
        if (threads < -16 || threads > -2 || sim_packed_lds_bytes(s->p, -threads) > 96 * 1024)
            return fail(COPO_ERR_DIM, "block=%d: 2..16 scenes per workgroup within 96 KB of LDS", threads);
    } else if (threads != 64 && threads != 128 && threads != 256 && threads != 512 && threads != 1024)
        return fail(COPO_ERR_DIM, "block=%d must be 64/128/256/512/1024, or -scenes for the packed shape", threads);
    if (threads != s->block) {
        s->block = threads;
        sim_shape_params(s->p, threads);
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipDeviceSynchronize());         // launches in flight keep the shape they started with
        HIP_TRY(hipMemcpy(s->p_dev, &s->p, sizeof(SimParams), hipMemcpyHostToDevice));
    }
    return COPO_OK;
}

extern "C" int copo_sim_set_chunk(copo_sim* s, int32_t fans) {
    if (!s) return fail(COPO_ERR_NULL, "copo_sim_set_chunk: NULL handle");
    if (fans < 0 || fans > COPO_MAX_AGENTS) return fail(COPO_ERR_DIM, "fans=%d must be 0..%d", fans, COPO_MAX_AGENTS);
    if (fans != s->p.chunk_one_wave) {
        const int32_t before = s->p.chunk_one_wave;
        s->p.chunk_one_wave = fans;
        if (s->block < 0 && sim_packed_lds_bytes(s->p, -s->block) > 96 * 1024) {      // packed shape: the workgroup's scenes must still fit
            s->p.chunk_one_wave = before;
            return fail(COPO_ERR_DIM, "fans=%d: %d scenes per workgroup would need more than 96 KB of LDS", fans, -s->block);
        }
        sim_shape_params(s->p, s->block);
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipDeviceSynchronize());         // launches in flight keep the shape they started with
        HIP_TRY(hipMemcpy(s->p_dev, &s->p, sizeof(SimParams), hipMemcpyHostToDevice));
    }
    return COPO_OK;
}

extern "C" int copo_sim_reset(copo_sim* s, const uint64_t* seeds, const copo_step_out* out, void* stream) {
    if (!s || !seeds || !out) return fail(COPO_ERR_NULL, "copo_sim_reset: NULL argument");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(const_cast<uint64_t*>(s->p.seeds), seeds, (size_t)s->p.E * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(s->p.state, 0, COPO_STATE_FIELDS * (size_t)s->p.E * s->p.N * 4, st));
    int rc = flush_lcf(s, st);
    if (rc != COPO_OK) return rc;
    HIP_TRY(launch_sim_reset(s->p, s->p_dev, *out, s->block, st));
    s->started = true;
    return COPO_OK;
}

extern "C" int copo_sim_step(copo_sim* s, const float* act, const copo_step_out* out, void* stream) {
    if (!s || !act || !out) return fail(COPO_ERR_NULL, "copo_sim_step: NULL argument");
    if (!s->started) return fail(COPO_ERR_STATE, "copo_sim_step before copo_sim_reset");
    int rc = flush_lcf(s, static_cast<hipStream_t>(stream));
    if (rc != COPO_OK) return rc;
    HIP_TRY(launch_sim_step(s->p, s->p_dev, act, *out, s->block, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_sim_get_state(copo_sim* s, float* slot_state, int32_t* env_state, void* stream) {
    if (!s || !slot_state || !env_state) return fail(COPO_ERR_NULL, "copo_sim_get_state: NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(slot_state, s->p.state, COPO_STATE_FIELDS * (size_t)s->p.E * s->p.N * 4,
                           hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(env_state, s->p.env, (size_t)s->p.E * 16, hipMemcpyDeviceToDevice, st));
    return COPO_OK;
}

extern "C" int copo_sim_set_state(copo_sim* s, const float* slot_state, const int32_t* env_state, void* stream) {
    if (!s || !slot_state || !env_state) return fail(COPO_ERR_NULL, "copo_sim_set_state: NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(s->p.state, slot_state, COPO_STATE_FIELDS * (size_t)s->p.E * s->p.N * 4,
                           hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->p.env, env_state, (size_t)s->p.E * 16, hipMemcpyDeviceToDevice, st));
    s->started = true;
    return COPO_OK;
}

// ---- stateless ops --------------------------------------------------------------------------------

extern "C" int copo_neighbours_f32(const float* pos, const uint8_t* present, const float* rew, int32_t E, int32_t N,
                                   int32_t K, float radius, float mf_distance, int32_t* nbr_idx, int32_t* nbr_cnt,
                                   int32_t* mf_cnt, float* nbr_dist, float* nei_rew, float* glob_rew, void* stream) {
    if (!pos || !present) return fail(COPO_ERR_NULL, "copo_neighbours_f32: pos/present is NULL");
    if (E < 0 || N < 1 || N > COPO_MAX_AGENTS || K < 1 || K > COPO_MAX_AGENTS)
        return fail(COPO_ERR_DIM, "copo_neighbours_f32: E=%d N=%d K=%d (N,K in 1..64)", E, N, K);
    if (E == 0) return COPO_OK;
    SimParams p;
    memset(&p, 0, sizeof(p));
    p.E = E; p.N = N; p.K = K;
    p.lists_for_absent = 1;
    p.neighbours_distance = radius;
    p.mf_distance = mf_distance;
    StepOut out;
    memset(&out, 0, sizeof(out));
    out.nbr_idx = nbr_idx; out.nbr_cnt = nbr_cnt; out.mf_cnt = mf_cnt; out.nbr_dist = nbr_dist;
    out.nei_rew = rew ? nei_rew : nullptr;
    out.glob_rew = rew ? glob_rew : nullptr;
    HIP_TRY(launch_neighbours(pos, present, rew, p, out, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_gae3_f32(const float* rew, const float* val, const uint8_t* flags, int32_t T, int32_t M,
                             int32_t heads, const double* gamma, double lam, float* adv, float* tgt, void* stream) {
    if (!rew || !val || !flags || !gamma || !adv || !tgt) return fail(COPO_ERR_NULL, "copo_gae3_f32: NULL argument");
    if (T < 0 || M < 0 || heads < 1 || heads > 4) return fail(COPO_ERR_DIM, "copo_gae3_f32: T=%d M=%d heads=%d", T, M, heads);
    if (T == 0 || M == 0) return COPO_OK;
    HIP_TRY(launch_gae3(rew, val, flags, T, M, heads, gamma, lam, adv, tgt, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

static int check_fuse(const char* name, const void* obs, const void* act, const void* flags, const void* idx,
                      const void* cnt, const void* cc, int R, int N, int O, int A, int K) {
    if (!obs || !act || !flags || !idx || !cnt || !cc) return fail(COPO_ERR_NULL, "%s: NULL argument", name);
    if (R < 0 || N < 1 || N > COPO_MAX_AGENTS || O < 1 || A < 0 || K < 1 || K > COPO_MAX_AGENTS)
        return fail(COPO_ERR_DIM, "%s: R=%d N=%d O=%d A=%d K=%d", name, R, N, O, A, K);
    return COPO_OK;
}

extern "C" int copo_cc_fuse_mf_f32(const float* obs, const float* act, const uint8_t* flags, const int32_t* nbr_idx,
                                   const int32_t* cnt, int32_t R, int32_t N, int32_t O, int32_t A, int32_t K,
                                   int32_t counterfactual, float* cc_obs, void* stream) {
    int rc = check_fuse("copo_cc_fuse_mf_f32", obs, act, flags, nbr_idx, cnt, cc_obs, R, N, O, A, K);
    if (rc != COPO_OK || R == 0) return rc;
    HIP_TRY(launch_cc_fuse_mf(obs, act, flags, nbr_idx, cnt, R, N, O, A, K, counterfactual, cc_obs,
                              static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_cc_fuse_concat_f32(const float* obs, const float* act, const uint8_t* flags, const int32_t* nbr_idx,
                                       const int32_t* cnt, int32_t R, int32_t N, int32_t O, int32_t A, int32_t K,
                                       int32_t num_neighbours, int32_t counterfactual, float* cc_obs, void* stream) {
    int rc = check_fuse("copo_cc_fuse_concat_f32", obs, act, flags, nbr_idx, cnt, cc_obs, R, N, O, A, K);
    if (rc != COPO_OK || R == 0) return rc;
    if (num_neighbours < 0 || num_neighbours > COPO_MAX_AGENTS)
        return fail(COPO_ERR_DIM, "copo_cc_fuse_concat_f32: num_neighbours=%d", num_neighbours);
    HIP_TRY(launch_cc_fuse_concat(obs, act, flags, nbr_idx, cnt, R, N, O, A, K, num_neighbours, counterfactual, cc_obs,
                                  static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_lcf_mix_partial_f32(const float* adv, const float* nei_adv, const float* glob_adv, const float* lcf,
                                        const uint8_t* valid, int64_t B, float* mixed, double* stats, void* stream) {
    if (!adv || !nei_adv || !glob_adv || !lcf || !mixed || !stats)
        return fail(COPO_ERR_NULL, "copo_lcf_mix_partial_f32: NULL argument");
    if (B < 0) return fail(COPO_ERR_DIM, "copo_lcf_mix_partial_f32: B=%lld", (long long)B);
    HIP_TRY(launch_lcf_mix_partial(adv, nei_adv, glob_adv, lcf, valid, B, mixed, stats, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_lcf_mix_apply_f32(const float* mixed, const float* glob_adv, const uint8_t* valid, int64_t B,
                                      const double* stats, float* norm_adv, float* glob_adv_std, void* stream) {
    if (!mixed || !glob_adv || !stats || !norm_adv || !glob_adv_std)
        return fail(COPO_ERR_NULL, "copo_lcf_mix_apply_f32: NULL argument");
    if (B < 0) return fail(COPO_ERR_DIM, "copo_lcf_mix_apply_f32: B=%lld", (long long)B);
    if (B == 0) return COPO_OK;
    HIP_TRY(launch_lcf_mix_apply(mixed, glob_adv, valid, B, stats, norm_adv, glob_adv_std, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

// ---- top-down renderer (render_kernels.hip) ----------------------------------------------------------------

struct copo_render {
    copo_sim* sim;
    int W, H, cap, head, count;
    int n_roads, n_lines;
    uint32_t box_rgba;
    const float* roads;        // [n_roads][RENDER_ROAD_STRIDE] deduplicated road records + world boxes
    const float* lines;        // [n_lines][RENDER_LINE_STRIDE]
    const uint32_t* palette;   // [12]
    int32_t* ring;             // [cap][RENDER_RING_FIELDS][E][N]
    int32_t* ring_ep;          // [cap][E]
    std::vector<void*> allocs;
};

static void free_render(copo_render* r) {
    for (void* a : r->allocs) (void)hipFree(a);
    delete r;
}

template <typename T>
static int render_upload(copo_render* r, const T* host, size_t count, const T** dev) {
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, count ? count * sizeof(T) : sizeof(T)));
    r->allocs.push_back(d);
    if (count && host) HIP_TRY(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    else HIP_TRY(hipMemset(d, 0, count ? count * sizeof(T) : sizeof(T)));      // (no host table: zeros)
    *dev = static_cast<const T*>(d);
    return COPO_OK;
}

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
    r->sim = sim; r->W = width; r->H = height; r->cap = trail; r->head = 0; r->count = 0;
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
    const int32_t* ring = nullptr;
    const int32_t* ring_ep = nullptr;
    int rc = render_upload(r, roads.data(), roads.size(), &r->roads);
    if (rc == COPO_OK) rc = render_upload(r, lines.data(), lines.size(), &r->lines);
    if (rc == COPO_OK) rc = render_upload(r, pal, 12, &r->palette);
    if (rc == COPO_OK) rc = render_upload<int32_t>(r, nullptr, (size_t)std::max(trail, 1) * RENDER_RING_FIELDS * EN, &ring);
    if (rc == COPO_OK) rc = render_upload<int32_t>(r, nullptr, (size_t)std::max(trail, 1) * p.E, &ring_ep);
    if (rc != COPO_OK) {
        free_render(r);
        return rc;
    }
    r->ring = const_cast<int32_t*>(ring);
    r->ring_ep = const_cast<int32_t*>(ring_ep);
    *out = r;
    return COPO_OK;
}

extern "C" int copo_render_destroy(copo_render* r) {
    if (!r) return fail(COPO_ERR_NULL, "copo_render_destroy: NULL handle");
    (void)hipSetDevice(r->sim->device);
    free_render(r);
    return COPO_OK;
}

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
    copo_interact_cfg cfg;
    int32_t* acc;              // [INTERACT_ACC_WORDS][E][N]
    double* tit;               // [E][N]
    long long* counts;         // [E][INTERACT_COUNTS]
    double* sums;              // [E][INTERACT_SUMS]
    size_t acc_bytes, tit_bytes, counts_bytes, sums_bytes;
};

static void free_interact(copo_interact* h) {
    for (void* a : {(void*)h->acc, (void*)h->tit, (void*)h->counts, (void*)h->sums})
        if (a) (void)hipFree(a);
    delete h;
}

static InteractArgs interact_args(const copo_interact* h) {
    const SimParams& p = h->sim->p;
    InteractArgs a;
    a.state = p.state; a.env = p.env; a.E = p.E; a.N = p.N;
    a.hl = p.hl; a.hw = p.hw; a.dt = p.dt;
    a.horizon_s = h->cfg.horizon_s; a.ttc_crit_s = h->cfg.ttc_crit_s; a.gap_near_m = h->cfg.gap_near_m; a.brake_mps2 = h->cfg.brake_mps2;
    a.acc = h->acc; a.tit = h->tit; a.counts = h->counts; a.sums = h->sums;
    return a;
}

static int interact_clear(copo_interact* h, hipStream_t stream) {
    HIP_TRY(hipMemsetAsync(h->acc, 0, h->acc_bytes, stream));
    HIP_TRY(hipMemsetAsync(h->tit, 0, h->tit_bytes, stream));
    HIP_TRY(hipMemsetAsync(h->counts, 0, h->counts_bytes, stream));
    HIP_TRY(hipMemsetAsync(h->sums, 0, h->sums_bytes, stream));
    return COPO_OK;
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
    h->sim = sim; h->cfg = *cfg;
    const size_t E = (size_t)sim->p.E, EN = E * sim->p.N;
    h->acc_bytes = (size_t)INTERACT_ACC_WORDS * EN * sizeof(int32_t); h->tit_bytes = EN * sizeof(double);
    h->counts_bytes = E * INTERACT_COUNTS * sizeof(long long); h->sums_bytes = E * INTERACT_SUMS * sizeof(double);
    hipError_t err = hipMalloc((void**)&h->acc, h->acc_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->tit, h->tit_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->counts, h->counts_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->sums, h->sums_bytes);
    if (err == hipSuccess) err = hipMemset(h->acc, 0, h->acc_bytes);
    if (err == hipSuccess) err = hipMemset(h->tit, 0, h->tit_bytes);
    if (err == hipSuccess) err = hipMemset(h->counts, 0, h->counts_bytes);
    if (err == hipSuccess) err = hipMemset(h->sums, 0, h->sums_bytes);
    if (err != hipSuccess) {
        free_interact(h);
        return fail(COPO_ERR_DEVICE, "copo_interact_create: %s", hipGetErrorString(err));
    }
    *out = h;
    return COPO_OK;
}

extern "C" int copo_interact_destroy(copo_interact* h) {
    if (!h) return fail(COPO_ERR_NULL, "copo_interact_destroy: NULL handle");
    (void)hipSetDevice(h->sim->device);
    free_interact(h);
    return COPO_OK;
}

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
    return interact_clear(h, static_cast<hipStream_t>(stream));
}

// ---- event clips (clip_kernels.hip) ----------------------------------------------------------------------------

struct copo_clip {
    copo_sim* sim;
    copo_clip_cfg cfg;
    int32_t cap;
    uint32_t *ring, *pool;
    int32_t *ring_env, *scene, *ready, *cid, *counters, *pool_env, *header;
    size_t ring_bytes, ring_env_bytes, scene_bytes, ready_bytes, pool_bytes, pool_env_bytes, header_bytes;
};

static void free_clip(copo_clip* h) {
    for (void* a : {(void*)h->ring, (void*)h->pool, (void*)h->ring_env, (void*)h->scene, (void*)h->ready, (void*)h->cid, (void*)h->counters,
                    (void*)h->pool_env, (void*)h->header})
        if (a) (void)hipFree(a);
    delete h;
}

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

// idle state machines, no clip, record 0; the pool is zeroed so that frames beyond a clip's length read 0 (the ring needs no clearing:
// a clip never reaches back beyond the records made since)
static int clip_clear(copo_clip* h, hipStream_t stream) {
    HIP_TRY(hipMemsetAsync(h->scene, 0, h->scene_bytes, stream));
    HIP_TRY(hipMemsetAsync(h->ready, 0, h->ready_bytes, stream));
    HIP_TRY(hipMemsetAsync(h->cid, 0, h->ready_bytes, stream));
    HIP_TRY(hipMemsetAsync(h->counters, 0, CLIP_COUNTERS * sizeof(int32_t), stream));
    HIP_TRY(hipMemsetAsync(h->pool, 0, h->pool_bytes, stream));
    HIP_TRY(hipMemsetAsync(h->pool_env, 0, h->pool_env_bytes, stream));
    HIP_TRY(hipMemsetAsync(h->header, 0, h->header_bytes, stream));
    return COPO_OK;
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
    h->sim = sim; h->cfg = *cfg; h->cap = cfg->pre + cfg->post + 1;
    const size_t E = (size_t)sim->p.E, N = (size_t)sim->p.N, cap = (size_t)h->cap, C = (size_t)cfg->max_clips;
    h->ring_bytes = E * cap * CLIP_WORDS * N * 4; h->ring_env_bytes = E * cap * CLIP_ENV_WORDS * 4;
    h->scene_bytes = E * CLIP_SCENE_WORDS * 4; h->ready_bytes = E * 4;
    h->pool_bytes = C * cap * CLIP_WORDS * N * 4; h->pool_env_bytes = C * cap * CLIP_ENV_WORDS * 4; h->header_bytes = C * CLIP_HEADER * 4;
    hipError_t err = hipMalloc((void**)&h->ring, h->ring_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->ring_env, h->ring_env_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->scene, h->scene_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->ready, h->ready_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->cid, h->ready_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->counters, CLIP_COUNTERS * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc((void**)&h->pool, h->pool_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->pool_env, h->pool_env_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->header, h->header_bytes);
    if (err == hipSuccess) err = hipMemset(h->ring, 0, h->ring_bytes);
    if (err == hipSuccess) err = hipMemset(h->ring_env, 0, h->ring_env_bytes);
    if (err != hipSuccess) {
        (void)hipGetLastError();               // (a refused request must not show up as the next launch's error)
        free_clip(h);
        return fail(COPO_ERR_DEVICE, "copo_clip_create: %s (ring %zu bytes, pool %zu bytes)", hipGetErrorString(err), E * cap * CLIP_WORDS * N * 4,
                    C * cap * CLIP_WORDS * N * 4);
    }
    int rc = clip_clear(h, nullptr);
    if (rc == COPO_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(COPO_ERR_DEVICE, "copo_clip_create: clearing failed");
    if (rc != COPO_OK) {
        free_clip(h);
        return rc;
    }
    *out = h;
    return COPO_OK;
}

extern "C" int copo_clip_destroy(copo_clip* h) {
    if (!h) return fail(COPO_ERR_NULL, "copo_clip_destroy: NULL handle");
    (void)hipSetDevice(h->sim->device);
    free_clip(h);
    return COPO_OK;
}

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
    HIP_TRY(hipMemcpyAsync(header_out, h->header + (size_t)first * CLIP_HEADER, (size_t)n * CLIP_HEADER * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(snaps_out, h->pool + (size_t)first * per, (size_t)n * per * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(env_out, h->pool_env + (size_t)first * per_env, (size_t)n * per_env * 4, hipMemcpyDeviceToDevice, st));
    return COPO_OK;
}

extern "C" int copo_clip_reset(copo_clip* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_clip_reset: NULL handle");
    return clip_clear(h, static_cast<hipStream_t>(stream));
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
    int32_t depth, stride;
    int64_t n_records;             // records made since create / reset (host side: the feature is eager only)
    uint32_t* ring;
    int32_t* ring_env;
};

static void free_rewind(copo_rewind* h) {
    for (void* a : {(void*)h->ring, (void*)h->ring_env})
        if (a) (void)hipFree(a);
    delete h;
}

extern "C" int copo_rewind_create(copo_sim* sim, const copo_rewind_cfg* cfg, copo_rewind** out) {
    if (!sim || !cfg || !out) return fail(COPO_ERR_NULL, "copo_rewind_create: NULL argument");
    *out = nullptr;
    if (cfg->depth < 1 || cfg->depth > COPO_REWIND_MAX_DEPTH || cfg->stride < 1)
        return fail(COPO_ERR_DIM, "copo_rewind_create: depth=%d (1..%d) stride=%d (>= 1)", cfg->depth, COPO_REWIND_MAX_DEPTH, cfg->stride);
    static_assert(COPO_REWIND_MAX_DEPTH == REWIND_MAX_DEPTH && COPO_REWIND_TALLY == REWIND_TALLY, "copo_hip.h / rewind_common.h");
    HIP_TRY(hipSetDevice(sim->device));
    copo_rewind* h = new (std::nothrow) copo_rewind();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->sim = sim; h->depth = cfg->depth; h->stride = cfg->stride; h->n_records = 0;
    const size_t E = (size_t)sim->p.E, N = (size_t)sim->p.N, D = (size_t)cfg->depth;
    const size_t ring_bytes = E * D * COPO_STATE_FIELDS * N * 4, env_bytes = E * D * REWIND_ENV_WORDS * 4;
    hipError_t err = hipMalloc((void**)&h->ring, ring_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->ring_env, env_bytes);
    if (err == hipSuccess) err = hipMemset(h->ring, 0, ring_bytes);
    if (err == hipSuccess) err = hipMemset(h->ring_env, 0, env_bytes);
    if (err != hipSuccess) {
        (void)hipGetLastError();               // (a refused request must not show up as the next launch's error)
        free_rewind(h);
        return fail(COPO_ERR_DEVICE, "copo_rewind_create: %s (ring %zu bytes)", hipGetErrorString(err), ring_bytes + env_bytes);
    }
    *out = h;
    return COPO_OK;
}

extern "C" int copo_rewind_destroy(copo_rewind* h) {
    if (!h) return fail(COPO_ERR_NULL, "copo_rewind_destroy: NULL handle");
    (void)hipSetDevice(h->sim->device);
    free_rewind(h);
    return COPO_OK;
}

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

// ---- traffic field maps (field_kernels.hip) --------------------------------------------------------------------

struct copo_field {
    copo_sim* sim;
    copo_field_cfg cfg;
    float inv_cell;
    int32_t block, n_blocks;       // scenes per workgroup of the tile pass, and how many such blocks
    int32_t* group;                // [E]
    int32_t* last;                 // [E][N]
    uint32_t* mask;                // [n_blocks][FIELD_MASK_WORDS]
    long long* maps;               // [G][FIELD_LAYERS][H][W]
    long long* scene_records;      // [G]
    size_t last_bytes, mask_bytes, maps_bytes, rec_bytes;
};

static void free_field(copo_field* h) {
    for (void* a : {(void*)h->group, (void*)h->last, (void*)h->mask, (void*)h->maps, (void*)h->scene_records})
        if (a) (void)hipFree(a);
    delete h;
}

static FieldArgs field_args(const copo_field* h, const uint8_t* flags, const float* ttc) {
    const SimParams& p = h->sim->p;
    FieldArgs a;
    a.state = p.state; a.E = p.E; a.N = p.N; a.hl = p.hl; a.hw = p.hw;
    a.x0 = h->cfg.x0; a.y0 = h->cfg.y0; a.cell = h->cfg.cell; a.inv_cell = h->inv_cell;
    a.W = h->cfg.W; a.H = h->cfg.H; a.G = h->cfg.G; a.block = h->block; a.ttc_below = h->cfg.ttc_below;
    a.group = h->group; a.flags = flags; a.ttc = ttc; a.last = h->last; a.mask = h->mask; a.maps = h->maps; a.scene_records = h->scene_records;
    return a;
}

extern "C" int copo_field_create(copo_sim* sim, const copo_field_cfg* cfg, copo_field** out) {
    if (!sim || !cfg || !out) return fail(COPO_ERR_NULL, "copo_field_create: NULL argument");
    *out = nullptr;
    static_assert(COPO_FIELD_LAYERS == FIELD_LAYERS && COPO_FIELD_MAX_SIDE == FIELD_MAX_SIDE && COPO_FIELD_MAX_GROUPS == FIELD_MAX_GROUPS,
                  "copo_hip.h / field_common.h");
    if (cfg->W < 1 || cfg->W > FIELD_MAX_SIDE || cfg->H < 1 || cfg->H > FIELD_MAX_SIDE || cfg->G < 1 || cfg->G > FIELD_MAX_GROUPS ||
        !(cfg->cell > 0.0f) || !std::isfinite(cfg->cell))
        return fail(COPO_ERR_DIM, "copo_field_create: W=%d H=%d (1..%d) G=%d (1..%d) cell=%g (> 0, finite)", cfg->W, cfg->H, FIELD_MAX_SIDE,
                    cfg->G, FIELD_MAX_GROUPS, (double)cfg->cell);
    const float inv_cell = (float)(1.0 / (double)cfg->cell);
    if (!std::isfinite(cfg->x0) || !std::isfinite(cfg->y0) || !(cfg->ttc_below >= 0.0f) || !std::isfinite(cfg->ttc_below) ||
        !std::isfinite(inv_cell))
        return fail(COPO_ERR_CONFIG, "copo_field_create: x0=%g y0=%g 1/cell=%g (finite), ttc_below=%g (>= 0, finite)", (double)cfg->x0,
                    (double)cfg->y0, (double)inv_cell, (double)cfg->ttc_below);
    const size_t E = (size_t)sim->p.E, N = (size_t)sim->p.N;
    // scenes per workgroup of the tile pass: 4 (one per wave) while the scenes are few, up to 64 -- every workgroup ends with one
    // pass over its tile, which more scenes share
    const int32_t block = 4 * (int32_t)std::min<size_t>(std::max<size_t>(E / 1024, 1), 16);
    const size_t n_blocks = (E + block - 1) / block;
    if (n_blocks > 65535) return fail(COPO_ERR_DIM, "copo_field_create: %zu scenes (at most %d)", E, 65535 * 64);
    HIP_TRY(hipSetDevice(sim->device));
    copo_field* h = new (std::nothrow) copo_field();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->sim = sim; h->cfg = *cfg; h->inv_cell = inv_cell; h->block = block; h->n_blocks = (int32_t)n_blocks;
    h->last_bytes = E * N * sizeof(int32_t); h->mask_bytes = n_blocks * FIELD_MASK_WORDS * sizeof(uint32_t);
    h->maps_bytes = (size_t)cfg->G * FIELD_LAYERS * cfg->H * cfg->W * sizeof(long long); h->rec_bytes = (size_t)cfg->G * sizeof(long long);
    hipError_t err = hipMalloc((void**)&h->group, E * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc((void**)&h->last, h->last_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->mask, h->mask_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->maps, h->maps_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->scene_records, h->rec_bytes);
    if (err == hipSuccess) err = hipMemset(h->group, 0, E * sizeof(int32_t));
    if (err == hipSuccess) err = hipMemset(h->last, 0xff, h->last_bytes);
    if (err == hipSuccess) err = hipMemset(h->mask, 0, h->mask_bytes);
    if (err == hipSuccess) err = hipMemset(h->maps, 0, h->maps_bytes);
    if (err == hipSuccess) err = hipMemset(h->scene_records, 0, h->rec_bytes);
    if (err != hipSuccess) {
        (void)hipGetLastError();               // (a refused request must not show up as the next launch's error)
        free_field(h);
        return fail(COPO_ERR_DEVICE, "copo_field_create: %s (maps %zu bytes)", hipGetErrorString(err), (size_t)cfg->G * FIELD_LAYERS * cfg->H * cfg->W * 8);
    }
    *out = h;
    return COPO_OK;
}

extern "C" int copo_field_destroy(copo_field* h) {
    if (!h) return fail(COPO_ERR_NULL, "copo_field_destroy: NULL handle");
    (void)hipSetDevice(h->sim->device);
    free_field(h);
    return COPO_OK;
}

extern "C" int copo_field_set_groups(copo_field* h, const int32_t* group_dev, void* stream) {
    if (!h || !group_dev) return fail(COPO_ERR_NULL, "copo_field_set_groups: NULL argument");
    HIP_TRY(hipMemcpyAsync(h->group, group_dev, (size_t)h->sim->p.E * sizeof(int32_t), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_field_record(copo_field* h, const uint8_t* flags, const float* ttc, int32_t accumulate, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_field_record: NULL handle");
    if (accumulate != 0 && accumulate != 1) return fail(COPO_ERR_DIM, "copo_field_record: accumulate=%d (0 or 1)", accumulate);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const FieldArgs a = field_args(h, flags, ttc);
    if (accumulate) HIP_TRY(hipMemsetAsync(h->mask, 0, h->mask_bytes, st));
    HIP_TRY(launch_field_events(a, accumulate, st));
    if (accumulate) HIP_TRY(launch_field_tiles(a, st));
    return COPO_OK;
}

extern "C" int copo_field_read(copo_field* h, int64_t* maps_dev, int64_t* scene_records_dev, void* stream) {
    if (!h || (!maps_dev && !scene_records_dev)) return fail(COPO_ERR_NULL, "copo_field_read: NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (maps_dev) HIP_TRY(hipMemcpyAsync(maps_dev, h->maps, h->maps_bytes, hipMemcpyDeviceToDevice, st));
    if (scene_records_dev) HIP_TRY(hipMemcpyAsync(scene_records_dev, h->scene_records, h->rec_bytes, hipMemcpyDeviceToDevice, st));
    return COPO_OK;
}

extern "C" int copo_field_forget(copo_field* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_field_forget: NULL handle");
    HIP_TRY(hipMemsetAsync(h->last, 0xff, h->last_bytes, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_field_reset(copo_field* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_field_reset: NULL handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(h->maps, 0, h->maps_bytes, st));
    HIP_TRY(hipMemsetAsync(h->scene_records, 0, h->rec_bytes, st));
    HIP_TRY(hipMemsetAsync(h->last, 0xff, h->last_bytes, st));
    return COPO_OK;
}

// ---- traffic gates (gate_kernels.hip) --------------------------------------------------------------------------

struct copo_gate {
    copo_sim* sim;
    copo_gate_cfg cfg;
    GateLayout at;
    int32_t n_records;             // records since create / reset (host side: eager only)
    float4* gates;                 // [L]
    int2* sections;                // [max(S, 1)]
    int32_t* group;                // [E]
    uint32_t *mem_x, *mem_y;       // [E][N]
    int32_t* mem_aid;              // [E][N]
    int32_t* mem_episode;          // [E]
    unsigned long long* mem_valid; // [E]
    int32_t* last_fwd;             // [E][L]
    int32_t* entry;                // [E][max(S, 1)][N]
    long long* acc;                // [at.words]
    size_t slot_bytes, valid_bytes, fwd_bytes, entry_bytes, acc_bytes;
};

static void free_gate(copo_gate* h) {
    for (void* a : {(void*)h->gates, (void*)h->sections, (void*)h->group, (void*)h->mem_x, (void*)h->mem_y, (void*)h->mem_aid,
                    (void*)h->mem_episode, (void*)h->mem_valid, (void*)h->last_fwd, (void*)h->entry, (void*)h->acc})
        if (a) (void)hipFree(a);
    delete h;
}

// the slot memory, last_fwd and entry: nothing is followed, nothing crossed
static hipError_t gate_forget(copo_gate* h, hipStream_t st) {
    hipError_t err = hipMemsetAsync(h->mem_valid, 0, h->valid_bytes, st);
    if (err == hipSuccess) err = hipMemsetAsync(h->last_fwd, 0xff, h->fwd_bytes, st);
    if (err == hipSuccess) err = hipMemsetAsync(h->entry, 0xff, h->entry_bytes, st);
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
    const size_t E = (size_t)sim->p.E, N = (size_t)sim->p.N, L = (size_t)cfg->L, S1 = (size_t)std::max(cfg->S, 1);
    HIP_TRY(hipSetDevice(sim->device));
    copo_gate* h = new (std::nothrow) copo_gate();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->sim = sim; h->cfg = *cfg; h->n_records = 0;
    h->at = gate_layout(cfg->G, cfg->L, cfg->S, cfg->T, cfg->HB, cfg->TB);
    h->slot_bytes = E * N * 4; h->valid_bytes = E * sizeof(unsigned long long); h->fwd_bytes = E * L * sizeof(int32_t);
    h->entry_bytes = E * S1 * N * sizeof(int32_t); h->acc_bytes = (size_t)h->at.words * sizeof(long long);
    hipError_t err = hipMalloc((void**)&h->gates, L * sizeof(float4));
    if (err == hipSuccess) err = hipMalloc((void**)&h->sections, S1 * sizeof(int2));
    if (err == hipSuccess) err = hipMalloc((void**)&h->group, E * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc((void**)&h->mem_x, h->slot_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->mem_y, h->slot_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->mem_aid, h->slot_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->mem_episode, E * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc((void**)&h->mem_valid, h->valid_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->last_fwd, h->fwd_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->entry, h->entry_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&h->acc, h->acc_bytes);
    if (err == hipSuccess) err = hipMemcpy(h->gates, gates, L * sizeof(float4), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemset(h->sections, 0, S1 * sizeof(int2));
    if (err == hipSuccess && cfg->S > 0) err = hipMemcpy(h->sections, sections, (size_t)cfg->S * sizeof(int2), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemset(h->group, 0, E * sizeof(int32_t));
    if (err == hipSuccess) err = hipMemset(h->mem_x, 0, h->slot_bytes);
    if (err == hipSuccess) err = hipMemset(h->mem_y, 0, h->slot_bytes);
    if (err == hipSuccess) err = hipMemset(h->mem_aid, 0, h->slot_bytes);
    if (err == hipSuccess) err = hipMemset(h->mem_episode, 0, E * sizeof(int32_t));
    if (err == hipSuccess) err = hipMemset(h->acc, 0, h->acc_bytes);
    if (err == hipSuccess) err = gate_forget(h, nullptr);
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) {
        (void)hipGetLastError();               // (a refused request must not show up as the next launch's error)
        free_gate(h);
        return fail(COPO_ERR_DEVICE, "copo_gate_create: %s (slot memory %zu bytes)", hipGetErrorString(err), E * N * 12 + E * S1 * N * 4);
    }
    *out = h;
    return COPO_OK;
}

extern "C" int copo_gate_destroy(copo_gate* h) {
    if (!h) return fail(COPO_ERR_NULL, "copo_gate_destroy: NULL handle");
    (void)hipSetDevice(h->sim->device);
    free_gate(h);
    return COPO_OK;
}

extern "C" int copo_gate_set_groups(copo_gate* h, const int32_t* group_dev, void* stream) {
    if (!h || !group_dev) return fail(COPO_ERR_NULL, "copo_gate_set_groups: NULL argument");
    HIP_TRY(hipMemcpyAsync(h->group, group_dev, (size_t)h->sim->p.E * sizeof(int32_t), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_gate_record(copo_gate* h, void* stream) {
    if (!h) return fail(COPO_ERR_NULL, "copo_gate_record: NULL handle");
    if (h->n_records == INT32_MAX) return fail(COPO_ERR_STATE, "copo_gate_record: %d records made; reset the handle", h->n_records);
    const SimParams& p = h->sim->p;
    GateArgs a;
    a.state = p.state; a.env = p.env; a.E = p.E; a.N = p.N;
    a.L = h->cfg.L; a.S = h->cfg.S; a.G = h->cfg.G; a.T = h->cfg.T; a.HB = h->cfg.HB; a.TB = h->cfg.TB; a.tt_bin = h->cfg.tt_bin;
    a.r = h->n_records; a.tbin = std::min(h->n_records / h->cfg.bin_records, h->cfg.T - 1);
    a.gates = h->gates; a.sections = h->sections; a.group = h->group;
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
    if (acc_dev) HIP_TRY(hipMemcpyAsync(acc_dev, h->acc, h->acc_bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
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
    HIP_TRY(hipMemsetAsync(h->acc, 0, h->acc_bytes, st));
    h->n_records = 0;
    return COPO_OK;
}
