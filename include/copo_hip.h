/*
 * copo_hip.h -- C ABI of libcopo_hip.so, the MI355X (gfx950) hot path of the CoPO rollout-and-update engine.
 *
 * Every entry point replaces one Python interface of the reference (decisionforce/CoPO,
 * paths relative to copo_code/copo/torch_copo/); see INTEGRATION.md for the ctypes binding a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch types.  All data pointers are DEVICE pointers owned by the
 *     caller (kept alive by the caller until the stream has consumed them) unless marked HOST.
 *   - every call returns COPO_OK (0) or a negative error code; nothing throws.  copo_last_error()
 *     returns a thread-local, library-owned message for the last failing call on this thread.
 *   - asynchronous on the hipStream_t passed as `void* stream` (NULL = default stream); no implicit
 *     device synchronisation inside any op.
 *   - one opaque handle per GPU process; a handle is not thread-safe (the reference runs one env per
 *     process, README.md:179-180).
 *   - deterministic: counter-based RNG keyed by (seed, env, slot, spawn counter).
 */
#ifndef COPO_HIP_H
#define COPO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COPO_ABI_VERSION 8

#define COPO_OK 0
#define COPO_ERR_NULL (-1)      /* required pointer is NULL */
#define COPO_ERR_DIM (-2)       /* size/shape out of the supported range */
#define COPO_ERR_DEVICE (-3)    /* HIP runtime error (message in copo_last_error) */
#define COPO_ERR_STATE (-4)     /* call order violated (e.g. step before reset) */
#define COPO_ERR_CONFIG (-5)    /* inconsistent configuration / map tables */

#define COPO_MAX_AGENTS 64      /* slots per env (one wave64 owns an env's agents) */
#define COPO_MAX_SEGS 16        /* roads per route (a full turn of the roundabout is 11) */
#define COPO_SEG_STRIDE 16      /* floats per road record */
#define COPO_MAX_LASERS 256
#define COPO_MAX_BOXES 16       /* static boxes (buildings) of a map */
#define COPO_BOX_STRIDE 6       /* {x, y, cos, sin, half_len, half_wid} */
#define COPO_MAX_SPAWNS 256     /* spawn slots per map */
#define COPO_MAX_SAFE 32        /* respawn places (spawn slots with the `safe` mark) per map */
#define COPO_MAX_ROUTES 128
#define COPO_MAX_LINES 128      /* lane-line primitives per map (side / lane-line detectors) */
#define COPO_LINE_STRIDE 12
#define COPO_STATE_DIM 6        /* heading, speed, steering, last action x2, yaw rate */
#define COPO_NAVI_DIM 10
#define COPO_INFO_DIM 8
#define COPO_STATE_FIELDS 16
#define COPO_LCF_STATS_DOUBLES (8 + 6 * 2048) /* size of the `stats` workspace of copo_lcf_mix_* */

/* per-slot step flags (uint8 bitfield), the device-side equivalent of the info dict keys consumed by
 * utils/callbacks.py:63-91 (arrive_dest / crash / out_of_road / max_step) plus row bookkeeping. */
#define COPO_F_ACTED 0x01u      /* slot held an agent that acted this step -> a (obs, act, rew, done) row exists */
#define COPO_F_DONE 0x02u       /* that agent terminated this step */
#define COPO_F_ARRIVE 0x04u
#define COPO_F_CRASH 0x08u
#define COPO_F_OUT 0x10u
#define COPO_F_MAXSTEP 0x20u    /* the AGENT drove `horizon` steps without terminating (episode_lengths[id] >= horizon) */
#define COPO_F_SPAWNED 0x40u    /* a new agent occupies the slot after this step (obs valid, reward 0, no row) */
#define COPO_F_ENV_RESET 0x80u  /* the episode of this scene ended this step and the scene was reset (done["__all__"]) */

/* columns of the optional per-slot info output [E][N][COPO_INFO_DIM] (utils/callbacks.py:35-46) */
#define COPO_I_VELOCITY 0       /* km/h */
#define COPO_I_STEERING 1
#define COPO_I_ACCELERATION 2
#define COPO_I_STEP_REWARD 3
#define COPO_I_COST 4           /* 1 on a crash (MetaDrive's multi-agent default: out_of_road_cost = 0) */
#define COPO_I_EPISODE_LENGTH 5
#define COPO_I_EPISODE_REWARD 6
#define COPO_I_ROUTE_COMPLETION 7

/* Road record, COPO_SEG_STRIDE floats.  A road is one primitive (straight or arc) carrying `lanes` lanes; the record
 * describes the centre line of lane 0, the LEFTMOST lane -- lane i lies i * lane_width to its right:
 *   0 x0, 1 y0, 2 cos0, 3 sin0   start pose            4 length      5 kappa (signed: + = counter-clockwise)
 *   6 s_start (route arc length at the start)           7 theta0
 *   8 ckx, 9 cky   navigation check point: the end of the road at its lateral middle
 *  10 lanes + 0.25 (left edge line continuous) + 0.5 (right edge line continuous): the edges a body must not touch (body_margin)
 *            + 0.125 (left edge line BROKEN and crossable: the reference point may be up to one lane width left of lane 0 --
 *                     MetaDrive's on_lane of the opposite road across a broken centre line, as in the parking-lot block)
 *                  11 radius feature of the navigation block, 12 radius (0 for a plain straight), 13 angle feature
 *  14 umx, 15 umy unit vector from an arc's centre to its mid point (projection without a wrap inside the arc)
 * STRAIGHT records (kappa == 0) overload 12 / 14 / 15 for MetaDrive's Merge / Split blocks (maps.Net.add_funnel; read by
 * funnel_extra in the step kernel and the oracle): extra drivable width to the RIGHT of the record's lanes, bounded by the
 * outer edge of the outermost wave lane -- two arcs of opposite sense:
 *   12 wave radius R (> 0 switches the funnel on; 0 = plain straight, 14 / 15 are then ignored)
 *   14 extra width D at the wide end, signed: + the road narrows along its direction, - it widens
 *   15 arc length u1 from the wide end at which the edge line's first arc (radius R + w/2) hands over to the second (R - w/2)
 * A map builder that leaves field 12 of a straight non-zero therefore changes its out-of-road decisions.
 * A route has nseg roads followed by one terminal record (length 0) holding the end pose. */
#define COPO_SEG_CKX 8
#define COPO_SEG_LANES 10
#define COPO_SEG_FEAT 11
#define COPO_SEG_UMX 14

/* Lane-line primitive, COPO_LINE_STRIDE floats (side detector: continuous lines; lane-line detector: all lines):
 *   0 kind (1 broken, 2 continuous), 1 x0, 2 y0, 3 cos0, 4 sin0, 5 length, 6 kappa, 7 cx, 8 cy (arc centre),
 *   9 umx, 10 umy (centre -> arc mid point), 11 cos(half the arc angle) */

typedef struct copo_sim_cfg {
    /* population */
    int32_t num_envs;          /* E */
    int32_t num_agents;        /* N slots per env, <= COPO_MAX_AGENTS */
    int32_t num_lasers;        /* LiDAR beams (72; 240 for config C5) */
    int32_t obs_dim;           /* COPO_OBS_DIM() */
    int32_t nbr_k;             /* neighbour ids stored per slot (<= N-1) */
    int32_t enable_lcf;        /* 1: LCFEnv (append (lcf+1)/2 to obs, sample LCF at spawn); 0: CCEnv only */
    int32_t horizon;           /* MetaDrive `horizon` (1000), MultiAgentMetaDrive.step: (i) an agent that acted `horizon` steps is
                                  done with max_step; (ii) once `horizon` env steps have run the scene stops respawning and
                                  drains; (iii) the scene is reset when no agent is left driving (or after 5 x horizon steps) */
    int32_t delay_done;        /* steps a vehicle that terminated without arriving lingers as an obstacle (MetaDrive `delay_done`) */
    int32_t respawn_cooldown;  /* steps a slot stays empty before re-use (0: MetaDrive respawns in the same step) */
    int32_t substeps;          /* physics sub-steps per env step (5) */
    /* radii */
    float lidar_range;         /* m */
    float neighbours_distance; /* env_wrappers.py:40,168 (strict <) */
    float mf_distance;         /* algo_ccppo.py:43,283 (prefix of the sorted list with d <= mf) */
    /* vehicle + kinematic bicycle model (centre-referenced, slip angle from the steering angle) */
    float dt;                  /* env step seconds (0.1) */
    float veh_half_len, veh_half_wid, wheelbase;
    float max_steer;           /* rad */
    float max_speed;           /* m/s */
    float acc_max;             /* m/s^2 at full throttle (engine force cut above max_speed) */
    float brake_gain, brake_max; /* deceleration = min(brake_gain * |a1|, brake_max) for a1 < 0 */
    float lat_acc_max;         /* tyre friction limit on the lateral acceleration v x yaw rate (m/s^2); 0 = none (the bicycle turns on rails) */
    float reverse_acc;         /* m/s^2 at full NEGATIVE throttle when the vehicle has a reverse gear (MetaDrive `enable_reverse`, the
                                  ParkingLot's vehicle config: a negative throttle is engine force backwards, there is no brake); 0 = no
                                  reverse gear: a negative throttle brakes and the speed stops at 0 */
    float spawn_region_len, spawn_region_wid; /* the box that must hold no vehicle for a respawn (8 x 3 m) */
    /* reward (MetaDrive multi-agent scheme) */
    float driving_reward, speed_reward, success_reward, crash_penalty, out_penalty;
    float arrive_margin;       /* arrival: within +- this of the end of the final road */
    float body_margin;         /* out of road when the BODY touches the road's edge lines (MetaDrive: on_yellow / on_white_continuous_line,
                                  crash_sidewalk): the centre must keep body_margin x (half_wid |cos| + half_len |sin| of the heading
                                  error) from both edges.  0: the centre rule (vehicle.out_of_route alone) */
    float lane_width;
    /* LCF distribution at creation (LCFEnv.current_lcf_mean/std, env_wrappers.py:200-201) */
    double lcf_mean, lcf_std;
    /* map tables (HOST pointers, copied at create) */
    int32_t n_routes;
    int32_t n_spawns;
    const float* route_segs;   /* [n_routes][COPO_MAX_SEGS + 1][COPO_SEG_STRIDE] */
    const float* route_meta;   /* [n_routes][4] = {total_len, nseg, index of the toll-booth road or -1, exclusive destination id + 1 or 0}.
                                * Exclusive destinations (at most 32 per map; MetaDrive's ParkingSpaceManager): a spawn draws its route among
                                * those of its spawn place whose destination no LIVING agent of the scene is heading for (all of them if
                                * none is free); the space is free again when that agent is done. */
    const int32_t* spawn_tab;  /* [n_spawns][4] = {first_route, n_destinations, lane, safe} */
    const float* spawn_s;      /* [n_spawns] longitudinal position of the slot on its spawn road */
    const float* ray_cs;       /* [num_lasers][2] = beam directions in the vehicle frame (forward, left) */
    /* optional observation / action extensions of CCEnv / LCFEnv (env_wrappers.py:44-46, 89-118, 258-272, 331-337,
     * 362-371); all zero = off. */
    int32_t add_traffic_light;      /* append clip([message(t), x', y'], 0, 1): env_wrappers.py:258-272 */
    int32_t traffic_light_interval; /* steps per phase (30) */
    int32_t comm_size;              /* > 0: communication on -- actions are [2 + comm_size] floats per slot */
    int32_t comm_neighbours;        /* nearest neighbours whose message is appended (4) */
    int32_t add_pos_in_comm;        /* 1: each message is followed by [d/20, (lon/d+1)/2, (lat/d+1)/2] clipped to [0,1] */
    float map_bbox[4];              /* {x_min, x_max, y_min, y_max} of the road network (traffic-light position columns) */
    /* MetaDrive's optional detectors (Bottleneck: 4 + 4 beams -> O = 96; Tollgate: 72 + 4 beams, no navigation block,
     * two toll columns -> O = 156).  0 beams = the two / one lateral-distance columns of the default observation. */
    int32_t side_lasers;            /* side detector beams (continuous lines), first beam 90 deg clockwise of the heading */
    int32_t lane_line_lasers;       /* lane-line detector beams (all lines) */
    float side_range, lane_line_range;
    int32_t navi_dim;               /* 10, or 0 (Tollgate) */
    int32_t toll_dim;               /* 0, or 2 (Tollgate: on the booth road; stayed there longer than toll_min_steps -- zeros off it) */
    int32_t toll_min_steps;         /* steps a vehicle has to spend in a booth (30) */
    int32_t n_lines;
    const float* lines;             /* [n_lines][COPO_LINE_STRIDE] (HOST) */
    const float* side_cs;           /* [side_lasers][2] beam directions in the vehicle frame (forward, left) (HOST) */
    const float* lane_line_cs;      /* [lane_line_lasers][2] (HOST) */
    /* ABI 8 -- MetaDrive 0.2.5's MultiAgentTollgateEnv rules (restated from the release's published source, which is not in the
     * reference tree; all zero = the rules of ABI 7):
     *   toll_speed_limit  > 0: on the booth road (TollGate.SPEED_LIMIT = 3 km/h, here in m/s) the step reward is the driving
     *                          reward alone while |v| <= limit and -overspeed_penalty * |v| / max_speed above it
     *                          (`reward_function`: `if vehicle.overspeed: reward = -overspeed_penalty * speed / max_speed`);
     *                          off the booth road the speed term is added as everywhere (the env's own speed_reward is 0.0);
     *   toll_early_exit   1: a vehicle that leaves the booth road before toll_min_steps is DONE with the out_of_road flag and
     *                          keeps the step's ordinary reward (`done_function`: `done_info["out_of_road"] = True`, the reward
     *                          function does not see it); 0: it is a crash with -crash_penalty (rounds 2-5). */
    float toll_speed_limit;
    float overspeed_penalty;
    int32_t toll_early_exit;
    /*   static boxes      buildings of the map as oriented boxes {centre x, y, cos, sin of the long axis, half length, half width}
     *                          (`TollGate._add_building_and_speed_limit`: `if idx % 2 == 1` a TollGateBuilding of the lane's width and
     *                          the road's length at the centre of every SECOND lane of the booth road).  A vehicle whose box overlaps
     *                          one (the separating-axis test of the vehicle collisions) is done with the crash flag (MetaDrive:
     *                          crash_building); the LiDAR sees them like vehicles (ray / box test in the box frame, minimum of the hit
     *                          distances).  n_boxes <= COPO_MAX_BOXES; 0 = none. */
    int32_t n_boxes;
    const float* boxes;             /* [n_boxes][COPO_BOX_STRIDE] (HOST) */
    int32_t boxes_hidden;           /* 1: the LiDAR does NOT see the static boxes (they still end an agent on touch): the experiment of
                                       profiles/r06_fidelity.txt -- whether MetaDrive 0.2.5's LiDAR mask holds the buildings' walls is not
                                       something this tree can settle; 0 (default): seen */
} copo_sim_cfg;

/* Observation row: [side block | heading, speed, steering, last action x2, yaw rate | lane-line block | navigation |
 * lasers | toll | 3 traffic light | 1 lcf | comm_neighbours x (comm_size + 3 if add_pos_in_comm)], where the side block
 * is side_lasers beams or the 2 lateral-distance columns and the lane-line block lane_line_lasers beams or 1 column. */
#define COPO_SIDE_DIM(c) ((c)->side_lasers > 0 ? (c)->side_lasers : 2)
#define COPO_LANE_DIM(c) ((c)->lane_line_lasers > 0 ? (c)->lane_line_lasers : 1)
#define COPO_EGO_DIM(c) (COPO_SIDE_DIM(c) + COPO_STATE_DIM + COPO_LANE_DIM(c))
#define COPO_OBS_DIM(c)                                                                                       \
    (COPO_EGO_DIM(c) + (c)->navi_dim + (c)->num_lasers + (c)->toll_dim + ((c)->add_traffic_light ? 3 : 0) +     \
     ((c)->enable_lcf ? 1 : 0) +                                                                              \
     ((c)->comm_size > 0 ? (c)->comm_neighbours * ((c)->comm_size + ((c)->add_pos_in_comm ? 3 : 0)) : 0))
/* floats per slot of the action array: steering, throttle, then the message */
#define COPO_ACT_DIM(c) (2 + ((c)->comm_size > 0 ? (c)->comm_size : 0))

typedef struct copo_sim copo_sim;

/* outputs of one vectorised env step; any pointer except obs may be NULL to skip that output */
typedef struct copo_step_out {
    float* obs;          /* [E][N][O]   obs AFTER the step (the next policy input); rows of slots that hold no
                                         agent (neither ACTED nor SPAWNED) are NOT written -- the reference has no
                                         dict entry for them, and not streaming ~half of the rows halves the traffic */
    float* rew;          /* [E][N]      native reward of the acting agent (return_native_reward=True)     */
    float* nei_rew;      /* [E][N]      env_wrappers.py:321-325                                           */
    float* glob_rew;     /* [E]         env_wrappers.py:313                                               */
    uint8_t* flags;      /* [E][N]      COPO_F_* bitfield                                                 */
    int32_t* nbr_idx;    /* [E][N][K]   slot ids sorted by (distance, slot), -1 padded  (:125-139); like obs, rows of
                                         slots that held no agent when the lists were made (the scene BEFORE an
                                         end-of-episode reset) are not written -- nbr_cnt / mf_cnt / nei_rew are 0 there            */
    int32_t* nbr_cnt;    /* [E][N]      neighbours within neighbours_distance (may exceed K)              */
    int32_t* mf_cnt;     /* [E][N]      length of the list prefix with distance <= mf_distance            */
    float* nbr_dist;     /* [E][N][K]   distances (float64 compare, stored fp32)                          */
    float* lcf;          /* [E][N]      LCF in [-1,1] of the acting agent (info["lcf"]) / new occupant    */
    float* info;         /* [E][N][COPO_INFO_DIM]                                                          */
    int32_t* agent_id;   /* [E][N]      per-env running id of the acting agent ("agent%d"), -1 if none    */
} copo_step_out;

/* ---- library ---- */
int copo_version(void);
/* how this library was built, for bench lines and bug reports: ABI, target, profiling mask ("none" in the shipped build) and the
 * environment variables it reads (none: every tuning knob is an argument of this ABI).  Owned by the library. */
const char* copo_build_info(void);
const char* copo_last_error(void);

/* ---- vectorised multi-agent env: replaces MultiAgent*Env.step/reset (MetaDrive, call site
 *      utils/env_wrappers.py:95), CCEnv.step (:89-123) and LCFEnv.step/_get_reset_return (:274-391) ---- */
int copo_sim_create(const copo_sim_cfg* cfg, int device, copo_sim** out);
int copo_sim_destroy(copo_sim* sim);
/* seeds: HOST [E]; writes the reset observation + flags(SPAWNED) + lcf.  env_wrappers.py:274-305 */
int copo_sim_reset(copo_sim* sim, const uint64_t* seeds, const copo_step_out* out, void* stream);
/* LCFEnv.set_lcf_dist (env_wrappers.py:420-426): affects agents spawned from now on */
int copo_sim_set_lcf_dist(copo_sim* sim, double mean, double std);
/* One distribution per scene: mean_std is HOST [E][2] = {mean, std} of scene e for agents spawned from now on, each row validated as
 * set_lcf_dist validates (COPO_ERR_CONFIG names the first bad scene, nothing is changed then); NULL returns to the single
 * distribution of set_lcf_dist.  The reference gives every env of a worker one distribution (env_wrappers.py:420-426) and evaluates
 * checkpoints one at a time; a table lets the scenes of one batch belong to different checkpoints.  set_force_lcf still overrides
 * every scene (mean = the forced value, std = set_lcf_dist's).  The kernels always draw scene e from row e of [E][2] device words
 * behind the four words of the single distribution -- without a table every row holds the single pair, so there is one kernel path --
 * and the rows are pushed like it: by the next reset / step / flush after a change, not while the stream is capturing. */
int copo_sim_set_lcf_table(copo_sim* sim, const float* mean_std);
/* The LCF distribution lives in device memory (launches captured in a hipGraph keep seeing updates).
 * set_lcf_dist/set_force_lcf mark it dirty; the next reset/step pushes it on its stream, except while that
 * stream is capturing -- replay-only callers push explicitly with copo_sim_flush before the replay. */
int copo_sim_flush(copo_sim* sim, void* stream);
/* LCFEnv.set_force_lcf (env_wrappers.py:428-430): v == -100 disables */
int copo_sim_set_force_lcf(copo_sim* sim, double v);
/* Population capacity, 1 <= capacity <= num_agents (default): slots >= capacity are left empty by a reset and never
 * respawn; vehicles already driving in them finish their episode.  With a following copo_sim_reset this is
 * `ChangeNEnv.close_and_reset_num_agents` of the curriculum baseline (env_wrappers.py:444-460) without re-creating
 * the simulator.  Device-resident like the LCF distribution (pushed by the next reset / step / flush). */
int copo_sim_set_capacity(copo_sim* sim, int32_t capacity);
/* act: [E][N][COPO_ACT_DIM] device fp32: steering, throttle (clipped to [-1,1] inside, as RLlib's clip_actions does),
 * then the comm_size message floats when the communication channel is on (passed through unclipped, like the reference) */
int copo_sim_step(copo_sim* sim, const float* act, const copo_step_out* out, void* stream);
/* raw state access for tests / checkpointing: [COPO_STATE_FIELDS][E][N] fp32 words + [E][4] int32 env words */
int copo_sim_get_state(copo_sim* sim, float* slot_state, int32_t* env_state, void* stream);
int copo_sim_set_state(copo_sim* sim, const float* slot_state, const int32_t* env_state, void* stream);
/* launch shape of the step kernel; tuning knob, results do not depend on it.  threads > 0: one scene per workgroup of 64 / 128 / 256 /
 * 512 / 1024 threads; threads < 0: the PACKED shape for large scene counts, -threads (2..16) scenes per workgroup with the per-agent phases
 * dense over the lanes (-1 = the default count; needs nbr_k <= 8, 0 < mf_distance < neighbours_distance, no traffic-light /
 * communication block: COPO_ERR_CONFIG otherwise); 0 = pick from E (packed above 3072 scenes where available) */
int copo_sim_set_block(copo_sim* sim, int32_t threads);
/* LiDAR fans whose ray minima are held in LDS at a time when ONE wave owns a scene (workgroup size 64): 1..64, 0 = default;
 * trades resident scenes per compute unit against fuller work batches; tuning knob, results do not depend on it */
int copo_sim_set_chunk(copo_sim* sim, int32_t fans);
/* profiling aid: device buffer [E][8] int64 receiving clock64() stamps at the phase boundaries of the step kernel
 * (NULL switches it off; results of the step do not depend on it); row [7]: which formulation of the neighbour lists ran */
int copo_sim_set_debug(copo_sim* sim, int64_t* stamps);

/* ---- top-down renderer: the reference's env.render(mode="top_down", num_stack=25) (copo/vis.py), drawn from the simulator's own
 *      device state.  A handle reads its simulator's state and map tables and must be destroyed before it.
 * Pixel (row i from the top = north, column j) of a view {cx, cy, m metres per pixel} is the world point
 * (cx + (j + 0.5 - W/2) m, cy - (i + 0.5 - H/2) m); layers in paint order: background, road surface (the step kernel's lateral road
 * rule), lane lines, static boxes, the trail of the last `trail` snapshots, vehicles.  Pixels are packed RGBA8
 * words (R in the low byte). ---- */
typedef struct copo_render copo_render;
/* width, height 1..4096; trail = snapshot capacity 0..32; palette_rgb: HOST [12][3], the vehicle colours by agent id % 12 */
int copo_render_create(copo_sim* sim, int32_t width, int32_t height, int32_t trail, const uint8_t* palette_rgb, copo_render** out);
/* push every slot's current pose, status and agent id and each scene's episode counter into the trail ring */
int copo_render_record(copo_render* r, void* stream);
/* empty the trail ring (after a manual reset or set_state) */
int copo_render_clear(copo_render* r, void* stream);
/* scenes: device [S] indices into 0..E-1 (not checked on the device), 1 <= S <= E; views: device [S][3]; trail 0..capacity; rgba:
 * device [S][H][W] */
int copo_render_frames(copo_render* r, const int32_t* scenes, int32_t S, const float* views, int32_t trail, uint32_t* rgba, void* stream);
int copo_render_destroy(copo_render* r);

/* ---- interaction meter: surrogate safety measures of the driving agents, computed from the simulator's own device state (DESIGN.md
 *      section 8b).  A handle reads its simulator's state and must be destroyed before it.
 * Bodies are the rectangles veh_half_len x veh_half_wid of the ALIVE (velocity speed x heading) and WRECK (velocity 0) slots of a scene;
 * static boxes take no part.  Per ALIVE slot and record, over the other bodies of its scene: gap = 0 when the rectangles overlap, else
 * the smallest of the eight vertex-to-rectangle distances; TTC = first time of overlap under constant velocities and fixed headings
 * (swept separating axes), +inf beyond horizon_s or when the pair never meets.  Per agent (slot + agent id + episode counter) the
 * meter accumulates steps, minimum gap, minimum TTC, steps with TTC < ttc_crit_s (tet), sum of (ttc_crit_s - TTC) dt over them (tit),
 * entries into the near state (TTC < ttc_crit_s or gap < gap_near_m) and steps that follow a record of the same agent with
 * (previous speed - speed) / dt > brake_mps2; an agent that left its slot is folded into the scene totals by the next record. ---- */
typedef struct copo_interact_cfg {
    float horizon_s, ttc_crit_s, gap_near_m, brake_mps2;
} copo_interact_cfg;
typedef struct copo_interact copo_interact;
/* horizon_s, brake_mps2 > 0 and ttc_crit_s, gap_near_m >= 0, all finite (COPO_ERR_CONFIG otherwise); every accumulator starts empty */
int copo_interact_create(copo_sim* sim, const copo_interact_cfg* cfg, copo_interact** out);
/* measure the current state: gap, ttc device [E][N] fp32 (+inf for a slot that is not ALIVE or has no partner), either may be NULL;
 * updates the accumulators and totals.  One launch, no allocation, no host synchronisation. */
int copo_interact_record(copo_interact* h, float* gap, float* ttc, void* stream);
/* counts_i64: device [E][6] = {agents, steps, tet steps, near events, brake events, agents with a finite minimum TTC}; sums_f64: device
 * [E][3] = {sum of minimum gaps (+inf once an agent never had a partner), sum of the finite minimum TTCs, sum of tit}, over the agents
 * folded so far, added up in slot order (reproducible bit for bit).  flush_open = 1: as if every agent still driving ended now
 * (the accumulators themselves are left as they are). */
int copo_interact_totals(copo_interact* h, int64_t* counts_i64, double* sums_f64, int32_t flush_open, void* stream);
/* empty every accumulator and the totals (after a manual reset or set_state) */
int copo_interact_reset(copo_interact* h, void* stream);
int copo_interact_destroy(copo_interact* h);

/* ---- event clips: a flight recorder on the device.  A handle reads its simulator's state and must be destroyed
 *      before it.  A snapshot of a scene holds, per slot, COPO_CLIP_WORDS 32-bit words -- the raw bits of state fields 0..3 (x, y,
 *      heading, speed), the low byte of field 13 (status) and field 14 (agent id): what the renderer and the interaction meter read --
 *      and the scene's env words 0 and 1 (t_env, episode).  Every scene keeps its last cap = pre + post + 1 snapshots in a ring.
 * Trigger of a record: a slot fires when (flags & flag_mask) != 0, ttc < ttc_below or gap < gap_below (plain fp32 <: NaN and +inf never
 * fire; a threshold or mask of 0 is off).  An idle scene that fires at record r is armed: trig_rec = r, trig_slot = its lowest firing
 * slot, trig_aid = that slot's agent id, kind = OR over the scene of {1 flag, 2 ttc, 4 gap}, n_events = 1; an armed scene that fires
 * counts it in n_events.  `post` records later (in the same record with post = 0) the scene commits the records
 * [max(trig_rec - pre, lo), trig_rec + post] in chronological order as one clip and is idle again, with lo = trig_rec + post + 1 (two
 * clips of a scene share no record; a scene reset does not end a clip: the snapshots carry the episode word).  The scenes that commit in one
 * record take the clip ids n_clips, n_clips + 1, ... in ascending scene order; an id >= max_clips is not stored and counts as dropped.
 * Header of a clip: COPO_CLIP_HEADER int32 = {scene, first_rec, length, trig_rec, trig_slot, kind, trig_aid, n_events}; records count
 * from 0 since create / reset.  Frames of a clip beyond its length are 0. ---- */
#define COPO_CLIP_MAX_CAP 256
#define COPO_CLIP_WORDS 6
#define COPO_CLIP_HEADER 8
typedef struct copo_clip_cfg {
    int32_t pre, post;         /* records kept before / after the trigger record: >= 0, pre + post + 1 <= COPO_CLIP_MAX_CAP (COPO_ERR_DIM) */
    int32_t max_clips;         /* pool size, >= 1 (COPO_ERR_DIM) */
    uint32_t flag_mask;        /* COPO_F_* bits */
    float ttc_below, gap_below;   /* >= 0 and finite (COPO_ERR_CONFIG) */
} copo_clip_cfg;
typedef struct copo_clip copo_clip;
/* allocates the rings (24 E N cap bytes) and the pool (24 max_clips N cap bytes): COPO_ERR_DEVICE when the device refuses */
int copo_clip_create(copo_sim* sim, const copo_clip_cfg* cfg, copo_clip** out);
/* snapshot of the current state of every scene, triggers from this record's arrays -- flags device [E][N] uint8 (the step's output), ttc /
 * gap device [E][N] fp32 (the meter's outputs); NULL: that trigger is off for the call -- and the commit of the scenes that are due.
 * Three launches on `stream`, no allocation, no host synchronisation; simulator memory is only read. */
int copo_clip_record(copo_clip* h, const uint8_t* flags, const float* ttc, const float* gap, void* stream);
/* commit every armed scene with the records it has so far (a shorter length; lo = the next record), same order and overflow rule */
int copo_clip_flush(copo_clip* h, void* stream);
/* HOST outputs: clips stored so far (<= max_clips) and clips dropped; waits for `stream` */
int copo_clip_count(copo_clip* h, int32_t* n_clips, int32_t* dropped, void* stream);
/* clips [first, first + n) of the pool, device to device: header_out [n][COPO_CLIP_HEADER], snaps_out [n][cap][COPO_CLIP_WORDS][N],
 * env_out [n][cap][2]; first + n <= max_clips (COPO_ERR_DIM) */
int copo_clip_read(copo_clip* h, int32_t first, int32_t n, int32_t* header_out, uint32_t* snaps_out, int32_t* env_out, void* stream);
/* forget every clip, counter and armed scene; records count from 0 again */
int copo_clip_reset(copo_clip* h, void* stream);
int copo_clip_destroy(copo_clip* h);
/* playback, no handle: for j < S, frame frame_idx[j] of clip clip_idx[j] of device pool arrays snaps [C][cap][COPO_CLIP_WORDS][N] / envw
 * [C][cap][2] becomes scene j of `target`: fields 0..3 the raw bits, field 13 the status byte, field 14 the agent id, every other field 0,
 * env words {t_env, episode, 0, 1}; frame_idx[j] == -1: an all-EMPTY scene.  N must be the target's, 1 <= S <= its E (COPO_ERR_DIM);
 * scenes >= S are left alone; clip_idx is not checked against C.  The target is for the renderer and the meter, not for stepping. */
int copo_clip_scatter(copo_sim* target, const uint32_t* snaps, const int32_t* envw, int32_t cap, int32_t N, const int32_t* clip_idx,
                      const int32_t* frame_idx, int32_t S, void* stream);

/* ---- scene rewind: a ring of FULL snapshots per scene on the device, forks of one scene at one past record into scenes of another
 *      simulator, and a tally of how the forked branches end.  A handle reads its (source) simulator's state and
 *      must be destroyed before it.  Eager only: the record count lives on the host, nothing here belongs inside a captured graph.
 * A snapshot of a scene is everything the scene resumes from except its seed: all COPO_STATE_FIELDS 32-bit words of every slot, as raw
 * bits, and the scene's four env words.  Every scene keeps its last `depth` snapshots: [E][depth][COPO_STATE_FIELDS][N] words plus
 * [E][depth][4] env words, 64 N E depth + 16 E depth bytes.
 * Records count from 0 since create / reset -- the counting of the clip recorder's records, so a clip header's first_rec / trig_rec name
 * rewind records when the caller makes both records every time.  Record r is STORED iff r % stride == 0, in ring place
 * (r / stride) % depth; the other records launch nothing.
 * Fork, request j < S: scene first + j of `target` becomes scene scene[j] of the source at the newest stored record <= rec[j], that is
 * record q * stride with q = min(rec[j], last record) / stride, and status[j] = q * stride.  All COPO_STATE_FIELDS fields are written as
 * raw bits and the four env words are copied; the target's device seed of that scene becomes the source scene's CURRENT seed, or
 * seeds[j] when `seeds` is given.  A request is invalid when nothing has been recorded, rec[j] < 0, the snapshot has left the ring (q <=
 * last stored q - depth) or scene[j] is outside 0..E-1 (checked on the device): status[j] = -1 and the target scene is written all-EMPTY
 * with env words {0, 0, 0, 1} (its seed is left alone unless `seeds` is given).
 *   lcf[j]         NaN keeps the snapshot's LCF; any other value v sets field 10 of every slot of that scene whose status byte is ALIVE
 *                  to min(max(v, -1), 1).  Slots that are not ALIVE keep their bits, and agents spawned after the fork draw their LCF
 *                  from the TARGET's own distribution (the set_lcf_dist / set_force_lcf values of the target handle; with a
 *                  copo_sim_set_lcf_table on the target, the row of the target scene first + j).
 *   watch_slot[j]  watch_aid[j] = field 14 (agent id) of slot watch_slot[j] in the snapshot when that slot is ALIVE there, else -1 (also
 *                  for a slot outside 0..N-1, an invalid request, or watch_slot == NULL).
 * Tally, stateless: one step's flags [B][N] are added to the rows tally[B][COPO_REWIND_TALLY], which the caller initialises to
 * {0, 0, 0, 0, 0, 0, 0, -1}: [0] += 1; [1] += slots with ACTED; [2] / [3] / [4] / [5] += slots with DONE and ARRIVE / CRASH / OUT /
 * MAXSTEP; and when [6] == 0, watch_slot[b] is in 0..N-1 and that slot has DONE: [6] = its flags byte, [7] = [0] before the increment
 * (the watched slot's first end only: a later occupant of the slot does not overwrite it). ---- */
#define COPO_REWIND_MAX_DEPTH 64
#define COPO_REWIND_TALLY 8
typedef struct copo_rewind_cfg {
    int32_t depth;             /* snapshots per scene, 1..COPO_REWIND_MAX_DEPTH (COPO_ERR_DIM) */
    int32_t stride;            /* every stride-th record is stored, >= 1 (COPO_ERR_DIM) */
} copo_rewind_cfg;
typedef struct copo_rewind copo_rewind;
/* allocates the rings (64 N E depth + 16 E depth bytes): COPO_ERR_DEVICE when the device refuses */
int copo_rewind_create(copo_sim* sim, const copo_rewind_cfg* cfg, copo_rewind** out);
/* one record of the current state of every scene.  A stored record is ONE launch on `stream`, no allocation, no host synchronisation;
 * simulator memory is only read */
int copo_rewind_record(copo_rewind* h, void* stream);
/* forget everything; records count from 0 again (host side only: the ring needs no clearing) */
int copo_rewind_reset(copo_rewind* h);
/* HOST output: records made since create / reset */
int copo_rewind_count(copo_rewind* h, int32_t* n_records);
/* scene, rec, status: device [S] int32; lcf device [S] fp32 or NULL; seeds device [S] uint64 or NULL; watch_slot, watch_aid device [S]
 * int32 or NULL.  `target` must not be the source and must live on its GPU (COPO_ERR_CONFIG); its slots, n_routes, n_spawns and
 * observation width must equal the source's, 1 <= S, 0 <= first and first + S <= its E (COPO_ERR_DIM); a refused call launches nothing.
 * One launch; scenes of the target outside [first, first + S) are untouched; afterwards the target counts as started and may be stepped */
int copo_rewind_fork(copo_rewind* h, copo_sim* target, int32_t first, int32_t S, const int32_t* scene, const int32_t* rec, const float* lcf,
                     const uint64_t* seeds, const int32_t* watch_slot, int32_t* status, int32_t* watch_aid, void* stream);
/* flags device [B][N] uint8 (a step's output), watch_slot device [B] int32 or NULL, tally device [B][COPO_REWIND_TALLY] int32; B >= 0,
 * N in 1..COPO_MAX_AGENTS (COPO_ERR_DIM).  One launch, no atomics */
int copo_rewind_tally(const uint8_t* flags, const int32_t* watch_slot, int32_t* tally, int32_t B, int32_t N, void* stream);
int copo_rewind_destroy(copo_rewind* h);

/* ---- seat tally (cross-play): one step's outcomes folded per (scene group, bank member).  Stateless.
 * flags device [E][N] uint8 (a step's output), rew device [E][N] fp32 or NULL, seat device [E][N] int32 (the member that drives the
 * slot), group device [E] int32, out device [G][K][COPO_SEAT_WORDS] int64.  A slot counts only where 0 <= seat < K, 0 <= group[e] < G
 * and its flags carry COPO_F_ACTED.  Words: ACTED slot-steps; DONE; ARRIVE / CRASH / OUT / MAXSTEP among the rows with DONE (one
 * count per set bit); REWARD_Q16 = the sum of rint(min(max(rew, -1024), 1024) * 65536) as int64 (NaN counts as 0; the product is
 * exact in fp32 and rounded once, half to even; NULL rew adds nothing); SPAWNED = rows with COPO_F_SPAWNED and a valid seat and
 * group, whether or not they acted.  `out` ACCUMULATES (the caller clears it): 64-bit integer atomic adds, so the result does not
 * depend on the order.  One launch on the caller's stream, no allocation, no host synchronisation; may be captured in a graph.
 * E >= 0, N in 1..COPO_SEAT_MAX_SLOTS, K in 1..65535, G >= 1 (COPO_ERR_DIM); a refused call launches nothing. */
#define COPO_SEAT_WORDS 8
#define COPO_SEAT_MAX_SLOTS 256
#define COPO_SEAT_ACTED 0
#define COPO_SEAT_DONE 1
#define COPO_SEAT_ARRIVE 2
#define COPO_SEAT_CRASH 3
#define COPO_SEAT_OUT 4
#define COPO_SEAT_MAXSTEP 5
#define COPO_SEAT_REWARD_Q16 6
#define COPO_SEAT_SPAWNED 7
int copo_seat_tally(const uint8_t* flags, const float* rew, const int32_t* seat, const int32_t* group, int32_t E, int32_t N, int32_t K,
                    int32_t G, int64_t* out, void* stream);

/* ---- certify tally: one step's certified bounds (copo_cert_obs_seats_f32) folded per (scene group, bank
 * member) against the level's deltas.  Stateless.  flags device [E][N] uint8 (the step's output), bounds device [E][N][COPO_CERT_WORDS]
 * fp32, seat / group as copo_seat_tally, level_of device [G][K] int32, levels device [L][4] fp32 (eps, delta_steer, delta_throttle, 0),
 * out device [G][K][COPO_CERT_TALLY_WORDS] int64.  A slot counts where 0 <= seat < K, 0 <= group[e] < G, 0 <= level_of[group][seat] < L,
 * its flags carry COPO_F_ACTED and bounds[..][6] == 1.  With dev_a = max(hi_a - mu_a, mu_a - lo_a), width_a = hi_a - lo_a (fp32, each
 * difference rounded once) and q(x) = rint(min(max(x, 0), 1024) * 65536) as int64 (one rounding, half to even), the words are:
 * [0] rows counted; [1] rows with dev_0 <= delta_steer and dev_1 <= delta_throttle; [2] / [3] either condition alone; [4] / [5] the
 * sums of q(width_0) / q(width_1); [6] the largest q(max(dev_0, dev_1)) (a 64-bit atomic max); [7] rows one of whose six numbers is
 * NaN or infinite (they stay out of the words 1 .. 6).  `out` ACCUMULATES (the caller clears it); integers only, so the result does not
 * depend on the order.  One launch on the caller's stream, no allocation, no host synchronisation; may be captured in a graph.
 * NULL flags / bounds / seat / group / level_of / levels / out: COPO_ERR_NULL; E >= 0, N in 1..COPO_SEAT_MAX_SLOTS, K in 1..65535,
 * G >= 1, L >= 1 (COPO_ERR_DIM); a refused call launches nothing. */
#define COPO_CERT_TALLY_WORDS 8
int copo_certify_tally(const uint8_t* flags, const float* bounds, const int32_t* seat, const int32_t* group, const int32_t* level_of,
                       const float* levels, int32_t E, int32_t N, int32_t K, int32_t G, int32_t L, int64_t* out, void* stream);

/* ---- attribution tally: one step's integrated gradients (copo_ig_obs_seats_f32) folded per (scene group, bank
 * member).  Stateless.  flags device [E][N] uint8 (the step's output), attr device [E N][2][in_dim] fp32, heads device [E N][COPO_IG_HEAD_WORDS]
 * fp32, seat / group as copo_seat_tally, words device [G][K][COPO_ATTRIB_TALLY_WORDS] int64, cols device [G][K][2][in_dim] int64.  A slot
 * counts exactly where copo_seat_tally counts it as acted (0 <= seat < K, 0 <= group[e] < G, flags carry COPO_F_ACTED); it is attributed
 * where heads[..][6] == 1.  q(v) = llrint(min(|v|, 2^20) * 2^32) as int64, taken in float64 from the fp32 value, NaN as 0 (one rounding).
 * cols[g][k][a][j] += q(attr[row][a][j]) over the attributed rows; words: [0] rows attributed; [1] / [2] the sums of q(mu_a(o) - mu_a(b))
 * (the fp32 difference of heads[a] and heads[2 + a], rounded once); [3] / [4] the sums of q(gap_a); [5] the largest q(gap) of either head (a
 * 64-bit atomic max); [6] rows counted but not attributed; [7] 0.  Both outputs ACCUMULATE (the caller clears them); integers only, so the
 * result does not depend on the order.  Sums are formed inside the wave that owns the scene first: one atomic per (scene, member seated
 * in it, head, column) at the most.  One launch on the caller's stream, no allocation, no host synchronisation; may be captured in a
 * graph.  NULL flags / attr / heads / seat / group / words / cols: COPO_ERR_NULL; E >= 0, N in 1..COPO_SEAT_MAX_SLOTS, K in 1..65535,
 * G >= 1, in_dim >= 1 (COPO_ERR_DIM); a refused call launches nothing. */
#define COPO_ATTRIB_TALLY_WORDS 8
#define COPO_IG_HEAD_WORDS 8
int copo_attrib_tally(const uint8_t* flags, const float* attr, const float* heads, const int32_t* seat, const int32_t* group, int32_t E,
                      int32_t N, int32_t K, int32_t G, int32_t in_dim, int64_t* words, int64_t* cols, void* stream);

/* ---- jury tally: one step's verdicts (copo_jury_obs_seats_f32) against the driver's own distribution inputs,
 * folded per (scene group, driving member, judging member).  Stateless.  flags device [E][N] uint8 (the step's output), dist device
 * [E][N][4] fp32 (mu_steer, mu_throttle, logstd_steer, logstd_throttle of the member that drives the slot: the forward's dist_inputs),
 * verdict device [E N][K][4] fp32 (the same four numbers by judge j at [row][j]), seat / group as copo_seat_tally, judges device [G][K]
 * int32 (nonzero: member j judges the rows of group g), out device [G][K][K][COPO_JURY_WORDS] int64.  A (slot, judge j) pair counts
 * where 0 <= seat < K, 0 <= group[e] < G, the slot's flags carry COPO_F_ACTED and judges[group[e]][j] != 0; it is added at
 * out[group[e]][k = seat][j].  With d_a = |mu_a(judge) - mu_a(driver)| in fp32 (the difference rounded once) and q(x) =
 * rint(min(max(x, 0), 1024) * 65536) as int64 (one rounding, half to even; NaN counts as 0) the words are: [0] pairs counted; [1] pairs
 * with d_0 > delta_steer or d_1 > delta_throttle (a NaN exceeds nothing); [2] / [3] the sums of q(d_0) / q(d_1); [4] the sum of
 * q(|dlogstd_0| + |dlogstd_1|), either difference and then their sum rounded once in fp32; [5] the sum of q(KL(driver || judge)); [6] the
 * sum of q(KL(judge || driver)); [7] the largest q(max(d_0, d_1)) (fmaxf: a NaN yields to the other axis; a 64-bit atomic max).
 * KL of the two diagonal Gaussians, in float64 from the fp32 inputs (m: mean, s: log-std), added over a = 0, 1 in this order and form:
 *     KL(p || q) = sum_a (s_q - s_p) + (0.5 (exp(2 (s_p - s_q)) + (m_p - m_q)^2 exp(-2 s_q)) - 0.5)
 * and quantised in float64 by the same q.  Equal bits on both sides give zero in the words 1 .. 7.  `out` ACCUMULATES (the caller clears
 * it; word 7 keeps the largest); integers only, so the result does not depend on the order.  One launch on the caller's stream, no
 * allocation, no host synchronisation; may be captured in a graph.  NULL flags / dist / verdict / seat / group / judges / out:
 * COPO_ERR_NULL; E >= 0, N in 1..COPO_SEAT_MAX_SLOTS, K in 1..65535, G >= 1, dist and verdict 16-byte aligned (COPO_ERR_DIM); a refused
 * call launches nothing. */
#define COPO_JURY_WORDS 8
int copo_jury_tally(const uint8_t* flags, const float* dist, const float* verdict, const int32_t* seat, const int32_t* group,
                    const int32_t* judges, int32_t E, int32_t N, int32_t K, int32_t G, float delta_steer, float delta_throttle,
                    int64_t* out, void* stream);

/* ---- influence graph (eval/influence.py): which neighbour a driver reacts to, and how strongly.  A policy learns
 *      of other vehicles through the LiDAR block of its observation row alone, so the effect of vehicle j on ego i has an exact
 *      counterfactual: i's row with j taken out of the scene.  Stateless entry points, one launch each on the caller's stream, no
 *      allocation, no host synchronisation; all may be captured in a graph.  Each replaces nothing in the reference.
 * The scene is the simulator's at the moment the policy reads `obs`: after the step or reset that wrote the row, before the next step.
 * An EGO is a row r = e N + n with seat[r] >= 0 whose slot is ALIVE.  Per beam b of an ego: d_j(b) = the entering distance of the ray
 * against the box of slot j != n (alive or lingering wreck) by the step's own pair record and ray / box test, `range` for a miss or a hit
 * not below the range; s(b) = the same minimum over the static boxes the LiDAR sees; min1 = min(s, min_j d_j).  Slot j OWNS b when d_j(b)
 * == min1(b) < range, s(b) > min1(b) and no lower slot attains the value; min2(b) = the minimum over everything but the owner.  The
 * CANDIDATES of an ego are the owners of at least one beam, ordered by (smallest owned distance as fp32 bits, slot); the first M are kept,
 * the rest only counted.  Variant c of row r is row r M + c of obs_cf: every column of obs[r], the LiDAR block replaced by
 * (owner(b) == who[r][c] ? min2(b) : min1(b)) * inv_range.
 *
 * copo_influence_heading (BEFORE a step, with the action the step will read, act device [E][N][act_dim]): heading device [E N][2] fp32 :=
 * the heading unit vector the step gives every slot (its own dynamics code).  The step's LiDAR reads that vector and the state does not
 * keep it; without it copo_influence_obs is exact only for vehicles that stood still in the last step.
 * copo_influence_obs: seat device [E][N] int32, heading device [E N][2] or NULL (a pair of zeros = nothing kept: sin / cos of the stored
 * heading; a vehicle the last step spawned has its road's vector either way), obs device [E N][O] -> who device [E N][M] int32 (-1 =
 * none), ncand device [E N] int32 (kept candidates | truncated << 16), ego device [E N] uint8 (COPO_F_ACTED on an ego, else 0: the `flags`
 * of copo_influence_tally), obs_cf device [E N M][O] (the variant rows that exist; the others are left alone), hit device [E N][M] or
 * NULL (the candidate's smallest owned distance over the range), clean device [E N][num_lasers] or NULL (min1 * inv_range: the bits of
 * the simulator's own LiDAR block).  Rows that are not egos get who = -1, ncand = 0, ego = 0.  One wave per row, lanes over beams.
 * copo_influence_lists: member k's seat list rows[k][0 .. counts[k]) (the seat forward's tables) -> vrows device [K][cap M] int64, the
 * variant rows r M + c of its egos, ascending, and vcounts device [K] int32: the lists copo_jury_obs_seats_f32 takes on (obs_cf, vrows,
 * vcounts, cap M, n_out M).  A prefix over lanes and waves decides every position.
 * copo_influence_tally: with p = dist[r] (the driver's own distribution inputs on obs[r]) and q = verdict_cf[r M + c][seat[r]], d_a =
 * |q.mu_a - p.mu_a| in fp32, KL(p || q) and q16 as copo_jury_tally defines them, a pair counts for every who[r][c] >= 0 of a row whose
 * flags carry COPO_F_ACTED with 0 <= seat < K, 0 <= group[e] < G.  out device [G][K][COPO_INFL_WORDS] int64 ACCUMULATES: [0] egos; [1]
 * pairs; [2] pairs with d_0 > delta_steer or d_1 > delta_throttle; [3] / [4] the sums of q16(d_0) / q16(d_1); [5] the sum of q16(KL);
 * [6] the largest q16(max(d_0, d_1)) (atomic max); [7] truncated candidates.  edges device [E N][M][4] fp32 or NULL: d_0, d_1, KL and
 * hit[r][c] of every pair (hit NULL: 0).  Integer atomics only, so the result does not depend on the order.
 * Refusals: NULL required pointer COPO_ERR_NULL; a simulator never reset COPO_ERR_STATE; M outside 1..COPO_INFL_MAX, K outside 1..65535,
 * N outside 1..COPO_SEAT_MAX_SLOTS, G < 1, cap < 1, n_out < 1, obs_cf == obs, dist / verdict_cf / edges not 16-byte aligned
 * COPO_ERR_DIM; a refused call launches nothing. */
#define COPO_INFL_MAX 8
#define COPO_INFL_WORDS 8
int copo_influence_heading(copo_sim* sim, const float* act, float* heading, void* stream);
int copo_influence_obs(copo_sim* sim, const int32_t* seat, const float* heading, const float* obs, int32_t M, int32_t* who, float* obs_cf,
                       int32_t* ncand, uint8_t* ego, float* hit, float* clean, void* stream);
int copo_influence_lists(const int64_t* rows, const int32_t* counts, int32_t K, int64_t cap, int64_t n_out, const int32_t* ncand, int32_t M,
                         int64_t* vrows, int32_t* vcounts, void* stream);
int copo_influence_tally(const uint8_t* flags, const float* dist, const float* verdict_cf, const int32_t* who, const int32_t* ncand,
                         const float* hit, const int32_t* seat, const int32_t* group, int32_t E, int32_t N, int32_t K, int32_t G, int32_t M,
                         float delta_steer, float delta_throttle, int64_t* out, float* edges, void* stream);

/* ---- fault injection: noisy sensors between the simulator's observation and the policy, noisy and sticky
 *      actuators between the policy's action and the simulator.  Two stateless entry points; each is one launch on the caller's stream,
 *      allocates nothing and reads nothing on the host, so both may be captured in a graph.  The simulator knows nothing of them.
 * Keys: seat device [E][N] int32 and group device [E] int32 are the tables of the seat tally; level_of device [G][K] int32; levels device
 * [L][COPO_FAULT_LEVEL_WORDS] 32-bit words: [0] f32 lidar_sigma, [1] u32 dropout_thr, [2] f32 dropout_value, [3] f32 act_sigma, [4] u32
 * sticky_thr, [5..7] zero; a threshold is rint(p * 2^24) for a probability p.  Row r = e N + n has level level_of[group[e]][seat[e][n]];
 * where the seat is outside [0, K), the group outside [0, G) or the level outside [0, L) the row passes through unchanged, bit for bit.
 * Draws: every one is hash_rng(fault_seed, r, tick[r], c, stream) of the simulator's counter-based generator on streams it does not use
 * (32..37, csrc/fault_common.h); tick device [E N] int32 is the caller's.  A Bernoulli draw is (h >> 8) < thr.  The standard-normal
 * stand-in z of two hashes: S = the sum of their four 16-bit halves, z = ((float)S - 131070.0f) * (float)(sqrt(3) / 65536): conversion
 * and subtraction exact, the product rounded once; mean 0, variance 1 - 2^-32, |z| <= 3.4641 (the tails END there).  A clamp to [lo, hi]
 * is v < lo ? lo : (v > hi ? hi : v); every product and sum is rounded on its own.
 * Both refuse with -1 and their name in copo_last_error(): a NULL pointer (flags_prev may be NULL), obs == obs_seen, E < 0, N < 1, O < 1,
 * E N > 2^30, not 0 <= col_lo <= col_hi <= O, K outside 1..65535, G < 1, L < 1.  A refused call launches nothing; E == 0 is COPO_OK.
 *
 * copo_fault_obs: obs device [E N][O] fp32 -> obs_seen (another buffer of that shape; every column is written).  Column c of
 * [col_lo, col_hi) is beam b = c - col_lo: if the dropout draw (r, tick, b) fires the value is dropout_value; else, if lidar_sigma != 0,
 * clamp(x + lidar_sigma * z(r, tick, b), 0, 1); else x.  Every other column is copied.  tick is read only.
 * copo_fault_act: act device [E N][2] fp32, the clipped action the step will read, in place.  If flags_prev (device [E N] uint8, the
 * PREVIOUS step's flags) is given and the row's previous flags carry COPO_F_ACTED and none of COPO_F_DONE, COPO_F_SPAWNED,
 * COPO_F_ENV_RESET -- the slot holds the agent it held a step ago -- and the sticky draw (r, tick) fires, act = prev[r].  Then, if
 * act_sigma != 0, component j becomes clamp(a + act_sigma * z(r, tick, j), -1, 1).  Then, for EVERY row, pass-through rows included,
 * prev[r] = act (device [E N][2] fp32) and tick[r] += 1: the tick is the number of steps since the caller cleared it. */
#define COPO_FAULT_LEVEL_WORDS 8
int copo_fault_obs(const float* obs, float* obs_seen, int32_t E, int32_t N, int32_t O, int32_t col_lo, int32_t col_hi,
                   const int32_t* seat, const int32_t* group, int32_t K, int32_t G, const int32_t* level_of, const uint32_t* levels,
                   int32_t L, const int32_t* tick, uint64_t fault_seed, void* stream);
int copo_fault_act(float* act, float* prev, const uint8_t* flags_prev, int32_t E, int32_t N, const int32_t* seat, const int32_t* group,
                   int32_t K, int32_t G, const int32_t* level_of, const uint32_t* levels, int32_t L, int32_t* tick, uint64_t fault_seed,
                   void* stream);

/* ---- traffic field maps: where the scenes of a simulator drive, queue, crash and come close, summed on the device over scenes and
 *      records into integer grids.  A handle reads its simulator's state and must be destroyed before it.  Eager
 *      only.  Every accumulator is an integer, so the maps do not depend on the order the device adds in.
 * Grid: cell (ix, iy) of W x H has the centre (x0 + (ix + 0.5) cell, y0 + (iy + 0.5) cell).  Scene e adds to the maps of group
 * group[e] (all 0 after create); a value outside 0..G-1 (checked on the device) contributes nothing.  Bodies are read as the interaction
 * meter reads them: state fields 0..3 (x, y, heading, speed), the status byte of field 13, veh_half_len x veh_half_wid.  Centre cell of a
 * body: (floor((x - x0) inv), floor((y - y0) inv)) in fp32, every operation rounded by itself, inv = 1 / cell rounded once to fp32; outside
 * the grid: no centre-cell layer.  Footprint: the cells whose centre p has |u . (p - c)| <= half_len and |n . (p - c)| <= half_wid.
 * Layers, int64 [G][COPO_FIELD_LAYERS][H][W], what one accumulating record adds:
 *   0 occupancy  +1 in every footprint cell of every ALIVE body        1 wreck   the same for every WRECK body
 *   2 visits     +1 in the centre cell of every ALIVE body             3 speed_q rint(min(max(v, 0), 255) * 256) there (half to even)
 *   4 vx_q, 5 vy_q   rint(min(max(v, -255), 255) * cos(heading) * 256), the same with sin, signed, there
 *   6 crash, 7 out, 8 arrive   +1 at the LAST-SEEN cell of every slot whose flags carry DONE and CRASH / OUT / ARRIVE (one per set bit)
 *   9 critical   +1 in the centre cell of every ALIVE slot with ttc < ttc_below (plain fp32 <; NULL array or threshold 0: off)
 * scene_records int64 [G]: the scenes of each group over the accumulating records.  Last seen: per slot, the centre cell of the previous
 * record of this handle if the slot was ALIVE inside the grid then (else none: no event counts); events are counted first, then the
 * memory is overwritten from the current state.  Events count in EVERY record, also with accumulate = 0. ---- */
#define COPO_FIELD_LAYERS 10
#define COPO_FIELD_MAX_SIDE 1024
#define COPO_FIELD_MAX_GROUPS 64
typedef struct copo_field_cfg {
    float x0, y0, cell;        /* finite; cell > 0 (COPO_ERR_DIM) */
    int32_t W, H;              /* 1..COPO_FIELD_MAX_SIDE (COPO_ERR_DIM) */
    int32_t G;                 /* 1..COPO_FIELD_MAX_GROUPS (COPO_ERR_DIM) */
    float ttc_below;           /* >= 0 and finite (COPO_ERR_CONFIG); 0: the critical layer is off */
} copo_field_cfg;
typedef struct copo_field copo_field;
/* allocates the maps (80 G H W bytes) and 4 E N bytes of last-seen memory: COPO_ERR_DEVICE when the device refuses */
int copo_field_create(copo_sim* sim, const copo_field_cfg* cfg, copo_field** out);
/* group_dev: device [E] int32, copied on `stream` */
int copo_field_set_groups(copo_field* h, const int32_t* group_dev, void* stream);
/* one record of the current state.  flags: device [E][N] uint8 (the step's output) or NULL (after a reset: no event); ttc: device [E][N]
 * fp32 (the meter's output) or NULL; accumulate: 1, or 0 = events and the last-seen memory only (COPO_ERR_DIM otherwise).  At most three
 * stream operations, no allocation, no host synchronisation; simulator memory is only read. */
int copo_field_record(copo_field* h, const uint8_t* flags, const float* ttc, int32_t accumulate, void* stream);
/* device to device: maps_dev [G][COPO_FIELD_LAYERS][H][W] int64, scene_records_dev [G] int64; either may be NULL, not both */
int copo_field_read(copo_field* h, int64_t* maps_dev, int64_t* scene_records_dev, void* stream);
/* forget the last-seen memory only (after a manual reset or set_state: the next record fires no event) */
int copo_field_forget(copo_field* h, void* stream);
/* zero the maps and scene_records and forget the last-seen memory; the groups stay */
int copo_field_reset(copo_field* h, void* stream);
int copo_field_destroy(copo_field* h);

/* ---- traffic gates: line-crossing counts, speeds, headways and travel times between gates, summed on the device over scenes and records
 *      into int64 accumulators per scene group.  A handle reads its simulator's state and must be destroyed before
 *      it.  Eager only: the record count lives on the host.  Every accumulator is an integer, so nothing depends on the order the device
 *      adds in.
 * Limits and inputs.  Gates: L in 1..COPO_GATE_MAX_GATES (COPO_ERR_DIM), each {ax, ay, bx, by} fp32, a directed segment A -> B in world
 * coordinates, finite with A != B (COPO_ERR_CONFIG).  Sections: S in 0..COPO_GATE_MAX_SECTIONS pairs {gate_in, gate_out} of gate indices
 * (they may be equal; an index outside 0..L-1: COPO_ERR_DIM).  Groups: G in 1..COPO_GATE_MAX_GROUPS; scene e adds to group[e] (all 0 after
 * create); a value outside 0..G-1 (checked on the device) contributes nothing, but the scene's slot memory, last_fwd and entry records
 * are still kept.  Bodies are read as the field maps read them: state fields 0, 1 (x, y) and 3 (speed), the status byte of field 13, field
 * 14 (agent id), and env word 1 (episode).
 * Continuity.  The handle keeps per slot, from its previous record: x and y as raw bits, the agent id, the scene's episode word and a
 * valid bit.  A slot is FOLLOWED in this record iff it is ALIVE now, the memory is valid (the slot was ALIVE in the previous record of this
 * handle), the agent id is equal and the episode is equal.  Otherwise the slot has no crossing in this record and its section entries
 * are cleared.  Crossings are evaluated first, then the memory is overwritten from the current state: a respawn, a scene reset or a
 * set_state never counts as a movement.  An agent's final step, after which its slot is no longer ALIVE, is not seen: a crossing made in
 * that step is missed, at most one step per agent.
 * Side of a gate.  All arithmetic is fp32, every operation rounded by itself (no contraction).  d = B - A;
 * side(P) = d.x * (P.y - A.y) - d.y * (P.x - A.x).  FORWARD: side(prev) < 0 and side(cur) >= 0.  BACKWARD: side(prev) >= 0 and
 * side(cur) < 0.  The crossing must also lie within the gate's extent: with m = cur - prev, a = m.x * (A.y - prev.y) - m.y * (A.x - prev.x)
 * and b the same with B, (a <= 0 and b >= 0) or (a >= 0 and b <= 0).  Comparisons are plain fp32, so a NaN never crosses.
 * Accumulators, int64, record r counting from 0 since create / reset:
 *   count[G][L][2]       forward / backward crossings
 *   speed_q[G][L][2]     sum of rint(min(max(v, 0), 255) * 256) over the crossings (half to even: the field maps' quantisation)
 *   series[G][L][2][T]   the crossings again, in time bin min(r / bin_records, T - 1)
 *   headway[G][L][HB]    forward crossings only.  The handle keeps last_fwd[E][L] (int32, -1 = none).  The forward crossings of one
 *                        scene at one gate in one record are ordered by slot: the first has h = r - last_fwd and is counted only if
 *                        last_fwd >= 0, every further one has h = 0; the bin is min(h, HB - 1); then last_fwd = r
 *   sec_count[G][S], sec_sum[G][S], sec_hist[G][S][TB]
 *                        the handle keeps entry[E][N][S] (int32, -1 = none).  A forward crossing of gate_in sets entry = r; after all
 *                        entries of this record are written, a forward crossing of gate_out with entry >= 0 gives tt = r - entry:
 *                        sec_count += 1, sec_sum += tt, sec_hist += 1 in bin min(tt / tt_bin, TB - 1); then entry = -1
 *   scene_records[G]     += 1 per scene of the group and record
 *   alive[G]             += the number of ALIVE slots (the density)
 * They lie in ONE block of copo_gate_words() int64 words in this order, which copo_gate_read copies. ---- */
#define COPO_GATE_MAX_GATES 32
#define COPO_GATE_MAX_SECTIONS 64
#define COPO_GATE_MAX_GROUPS 64
#define COPO_GATE_MAX_BINS 256
#define COPO_GATE_MAX_HIST 64
typedef struct copo_gate_cfg {
    int32_t L, S, G;           /* gates, sections, groups */
    int32_t T, bin_records;    /* time bins of the series 1..COPO_GATE_MAX_BINS, records per bin >= 1 (COPO_ERR_DIM) */
    int32_t HB;                /* headway bins (records), 1..COPO_GATE_MAX_HIST (COPO_ERR_DIM) */
    int32_t TB, tt_bin;        /* travel-time bins 1..COPO_GATE_MAX_HIST of tt_bin >= 1 records each (COPO_ERR_DIM) */
} copo_gate_cfg;
typedef struct copo_gate copo_gate;
/* gates: HOST [L][4] fp32; sections: HOST [S][2] int32 (NULL when S == 0).  Allocates 12 E N + 4 E N max(S, 1) + 4 E L + 12 E bytes of
 * memory and the accumulators: COPO_ERR_DEVICE when the device refuses */
int copo_gate_create(copo_sim* sim, const copo_gate_cfg* cfg, const float* gates, const int32_t* sections, copo_gate** out);
/* group_dev: device [E] int32, copied on `stream` */
int copo_gate_set_groups(copo_gate* h, const int32_t* group_dev, void* stream);
/* one record of the current state: ONE launch on `stream`, no allocation, no host synchronisation; simulator memory is only read */
int copo_gate_record(copo_gate* h, void* stream);
/* int64 words of the accumulator block of a configuration (0 for NULL) */
int64_t copo_gate_words(const copo_gate_cfg* cfg);
/* device to device: acc_dev [copo_gate_words()] int64; n_records: HOST output, records since create / reset; either may be NULL, not both */
int copo_gate_read(copo_gate* h, int64_t* acc_dev, int32_t* n_records, void* stream);
/* forget the slot memory, last_fwd and entry only (after a manual reset or set_state: the next record fires nothing) */
int copo_gate_forget(copo_gate* h, void* stream);
/* the same, and zero the accumulators and the record count; the groups stay */
int copo_gate_reset(copo_gate* h, void* stream);
int copo_gate_destroy(copo_gate* h);

/* ---- trip log: ONE row per finished agent, written on the device into a bounded pool.  A handle reads its
 *      simulator's state and must be destroyed before it.  Eager only: the record count lives on the host.  Everything the device computes
 *      is integer logic, one fp32 add per record (the reward), the field maps' speed quantisation and plain fp32 `<`, so the rows are
 *      reproducible bit for bit.
 * Records count from 0 since create / reset.  State fields by number: 3 speed, 9 route progress, 10 LCF, 12 route | road << 16, 13
 * status | timer << 8 | age << 16, 14 agent id; env word 1 is the scene's episode.  A slot's IDENTITY is (agent id, episode word).  The
 * handle keeps per scene an open mask of 64 bits and the episode word, per slot the agent id and the accumulators below.
 * Record r, with the optional device arrays flags u8 [E][N] (the step's output), rew, gap, ttc fp32 [E][N] (NULL = absent), for every slot:
 *   1 CLOSE, when a trip is open in the slot.  With flags & COPO_F_ACTED and rew given: reward = reward + rew (a plain fp32 add).  With
 *     flags & COPO_F_DONE: the trip closes with kind COPO_TRIP_DONE and end = the flags byte.  Otherwise, if the slot is not ALIVE now
 *     with the same identity: it closes with kind COPO_TRIP_VANISHED (a scene reset, a set_state, or records that were skipped) and
 *     end = 0.  flags = NULL (the record after a reset) can close only that way.
 *   2 OPEN, when the slot is ALIVE and no trip is open in it, also after a close in this same record: first_rec = r, route = the low 16
 *     bits of field 12, lcf = the raw bits of field 10, prog0 = the raw bits of field 9, steps = speed_sum = speed_max = stops = 0,
 *     reward = +0.0f, min_gap = min_ttc = +inf.
 *   3 ACCUMULATE, when a trip is open after 1 and 2: steps += 1; prog1 = the raw bits of field 9; q = rint(min(max(v, 0), 255) * 256)
 *     (fp32, half to even: the field maps' quantisation; a NaN gives 0); speed_sum += q (uint32); speed_max = max(speed_max, q);
 *     stops += (v < stop_speed); min_gap = gap if gap < min_gap, min_ttc likewise (plain `<`: a NaN never enters).
 * Row, COPO_TRIP_WORDS 32-bit words: {scene, slot | route << 16, agent id, episode, first_rec, steps, end flags | kind << 8, lcf bits,
 * prog0 bits, prog1 bits, speed_sum, speed_max, stops, reward bits, min_gap bits, min_ttc bits}.
 * Order.  The rows closed in one record take the ids n_rows, n_rows + 1, ... in ascending (scene, slot) order; an id >= max_rows is not
 * stored and counts as dropped, the trip is closed all the same.  No atomic decides an id: which rows exist and their order do not
 * depend on scheduling. ---- */
#define COPO_TRIP_WORDS 16
#define COPO_TRIP_DONE 1
#define COPO_TRIP_VANISHED 2
#define COPO_TRIP_FLUSHED 3
typedef struct copo_trip_cfg {
    int32_t max_rows;          /* pool size, >= 1 (COPO_ERR_DIM) */
    float stop_speed;          /* m/s, finite and >= 0 (COPO_ERR_CONFIG): a record with v < stop_speed counts as a stop */
} copo_trip_cfg;
typedef struct copo_trip copo_trip;
/* allocates the pool (64 max_rows bytes) and 56 E N + 24 E bytes of memory: COPO_ERR_DEVICE when the device refuses */
int copo_trip_create(copo_sim* sim, const copo_trip_cfg* cfg, copo_trip** out);
/* one record of the current state.  Three launches on `stream`, no allocation, no host synchronisation; simulator memory is only read */
int copo_trip_record(copo_trip* h, const uint8_t* flags, const float* rew, const float* gap, const float* ttc, void* stream);
/* every open trip closes with kind COPO_TRIP_FLUSHED and end = 0 under the same order and overflow rule; nothing stays open (a slot that
 * is still ALIVE opens a new trip in the next record).  Not a record: the count does not move */
int copo_trip_flush(copo_trip* h, void* stream);
/* HOST output: out[0] = rows stored so far (<= max_rows), out[1] = rows dropped; the one call that waits for `stream` */
int copo_trip_count(copo_trip* h, int64_t* out, void* stream);
/* rows [first, first + n) of the pool, device to device: rows_out [n][COPO_TRIP_WORDS] int32; first + n <= max_rows (COPO_ERR_DIM) */
int copo_trip_read(copo_trip* h, int32_t first, int32_t n, int32_t* rows_out, void* stream);
/* n_rows = dropped = 0; the open trips and the record count stay (drains a bounded pool during a long run) */
int copo_trip_clear(copo_trip* h, void* stream);
/* forget everything: rows, counters, open trips; records count from 0 again */
int copo_trip_reset(copo_trip* h, void* stream);
int copo_trip_destroy(copo_trip* h);

/* ---- conflict log: ONE row per pairwise encounter, written on the device into a bounded pool; no counterpart in
 *      the reference.  A handle reads its simulator's state and must be destroyed before it.  Eager only: the record count lives on the
 *      host.  Everything the device computes is integer logic and, per pair, two fp32 subtractions, two products and one add, each rounded by
 *      itself, and plain fp32 `<`: no fused multiply-add, square root or division, so the rows are reproducible bit for bit.
 * Records count from 0 since create / reset.  State fields 0..3 (x, y, heading, speed) are read as raw bits, the status byte of field 13,
 * field 14 (agent id) and env word 1 (episode).  A party's IDENTITY is (agent id, episode word).  ALIVE-WRECK pairs are out of scope.
 * Closeness of slots a < b, both ALIVE now: dx = x_b - x_a, dy = y_b - y_a, d2 = dx dx + dy dy; r2_in = radius^2 and r2_out =
 * leave_radius^2 are rounded once to fp32 on the host; a NaN is never close.
 * Memory of the handle: per slot the agent id of the previous record and a 64-bit open mask (bit b > a: pair (a, b) has an open
 * encounter), per scene the episode word, per pair 12 words {first_rec, steps, d2min bits, min_off, pose of a, pose of b at the minimum},
 * indexed densely: 48 B x N (N - 1) / 2 per scene (37 KB at 40 slots, 9.6 MB at 256 scenes, 0.6 GB at 16 384 scenes).
 * Record r, with the optional device array flags u8 [E][N] (the step's output, NULL = absent), per scene in this order:
 *   1 CLOSE, every open pair: with flags given and COPO_F_DONE on slot a or b: kind COPO_CONFLICT_DONE, end_a = the flags byte of a if it
 *     carries DONE, else 0, end_b likewise; otherwise, if either slot is not ALIVE now with its remembered identity: kind
 *     COPO_CONFLICT_VANISHED, ends 0; otherwise, if !(d2 < r2_out): kind COPO_CONFLICT_PARTED, ends 0.
 *   2 OPEN, every pair a < b, both ALIVE now, without an open encounter after 1 (also one that closed in this record) and d2 < r2_in:
 *     first_rec = r, steps = 0, d2min = +inf, min_off = 0.
 *   3 ACCUMULATE, every pair open after 1 and 2: steps = min(steps + 1, 65535); if d2 < d2min: d2min = d2, min_off = min(r - first_rec,
 *     65535) and the eight pose words {x, y, heading, speed} of a and of b are copied as raw bits.
 *   4 the slot and scene memory is overwritten from the current state.
 * Row, COPO_CONFLICT_WORDS 32-bit words: {scene, slot_a | slot_b << 6 | kind << 12 | end_a << 16 | end_b << 24, aid_a, aid_b, episode,
 * first_rec, steps | min_off << 16, d2min bits, pose_a[4], pose_b[4]}.
 * Order.  The rows closed in one record take the ids n_rows, n_rows + 1, ... in ascending (scene, slot_a, slot_b) order; an id >= max_rows
 * is not stored and counts as dropped, the encounter is closed all the same.  No atomic decides an id. ---- */
#define COPO_CONFLICT_WORDS 16
#define COPO_CONFLICT_DONE 1
#define COPO_CONFLICT_VANISHED 2
#define COPO_CONFLICT_PARTED 3
#define COPO_CONFLICT_FLUSHED 4
typedef struct copo_conflict_cfg {
    int32_t max_rows;          /* pool size, >= 1 (COPO_ERR_DIM) */
    float radius;              /* m, finite and > 0 (COPO_ERR_CONFIG): an encounter opens below it */
    float leave_radius;        /* m, finite and >= radius (COPO_ERR_CONFIG): an encounter parts at or beyond it */
} copo_conflict_cfg;
typedef struct copo_conflict copo_conflict;
/* allocates the pool (64 max_rows bytes) and 24 E N (N - 1) + 20 E N + 12 E bytes of memory: COPO_ERR_DEVICE when the device refuses */
int copo_conflict_create(copo_sim* sim, const copo_conflict_cfg* cfg, copo_conflict** out);
/* one record of the current state.  Three launches on `stream`, no allocation, no host synchronisation; simulator memory is only read */
int copo_conflict_record(copo_conflict* h, const uint8_t* flags, void* stream);
/* every open encounter closes with kind COPO_CONFLICT_FLUSHED and ends 0 under the same order and overflow rule.  Not a record */
int copo_conflict_flush(copo_conflict* h, void* stream);
/* HOST output: out[0] = rows stored so far (<= max_rows), out[1] = rows dropped; the one call that waits for `stream` */
int copo_conflict_count(copo_conflict* h, int64_t* out, void* stream);
/* rows [first, first + n) of the pool, device to device: rows_out [n][COPO_CONFLICT_WORDS] int32; first + n <= max_rows (COPO_ERR_DIM) */
int copo_conflict_read(copo_conflict* h, int32_t first, int32_t n, int32_t* rows_out, void* stream);
/* n_rows = dropped = 0; the open encounters and the record count stay */
int copo_conflict_clear(copo_conflict* h, void* stream);
/* forget everything: rows, counters, open encounters; records count from 0 again */
int copo_conflict_reset(copo_conflict* h, void* stream);
int copo_conflict_destroy(copo_conflict* h);

/* ---- encroachment log: post-encroachment times (PET) from a grid of stamps per scene, ONE row per encounter written on the device into a
 *      bounded pool, and integer aggregates per scene group; no counterpart in the reference.  A handle reads its
 *      simulator's state and must be destroyed before it.  Eager only: the record count lives on the host.  The footprint is the field
 *      maps' rule operation for operation; everything else is integer logic and one fp32 product, so rows, grid and aggregates are
 *      reproducible bit for bit and do not depend on how workgroups are scheduled.
 * Grid: W x H cells of `cell` metres from (x0, y0) per scene, 8 bytes each.  C(n), the footprint of slot n: the cells whose centre
 *   (x0 + (ix + 0.5) cell, y0 + (iy + 0.5) cell) lies in the body: sincos_det of the heading, u = fm(dx, c, dy s), w = fm(dy, c, -(dx s)),
 *   |u| <= hl && |w| <= hw.  Cells outside the grid do not exist.
 * Stamp: (q + 1) << 32 | (aid & 0xffff) << 16 | hq << 8 | slot for a stamp written in record q, hq = __float2int_rn(heading * (float)(128 /
 *   pi)) & 255; 0 = empty.
 * Record r, per scene, in this order:
 *   1 TURNOVER: slot n turns over when it is not ALIVE, when its agent id (state field 14) differs from the remembered one, or when the
 *     episode word (env word 1) differs from the remembered one.  It clears its `met` mask and every slot of the scene clears bit n of
 *     its own.  An episode change sets the scene's epoch = r.  Ids and the episode word are remembered.
 *   2 VALID: a stamp {q + 1, a16, hq, s} under C(n) is valid for ALIVE slot n iff s != n, slot s is ALIVE now with (aid & 0xffff) == a16,
 *     q + 1 > epoch, and 1 <= r - q <= window.  P(n): the slots with a valid stamp under C(n).
 *   3 ENCOUNTER: for every s of P(n) & ~met[n], ascending, one row: pet = the smallest r - q over the valid stamps of s under C(n), cell =
 *     the lowest iy * W + ix that attains it, hq_a = that stamp's hq, n_cells = the cells under C(n) with valid stamps of s.  Then
 *     met[n] |= P(n).  With g = group[e] in 0..G-1: hist[g][type][pet - 1] += 1, type from d = min(rel, 256 - rel), rel = (hq_b - hq_a) &
 *     255: 0 following d <= 21, 2 opposing d >= 107, else 1 crossing; critical[g][cell] += 1 when pet <= critical_records.  A dropped row
 *     counts in both all the same.
 *   4 STAMP, after every read of the record: every ALIVE slot n writes max(old, stamp) into each cell of C(n), a 64-bit atomic max.
 * Row, COPO_PET_WORDS 32-bit words: {scene, slot_b | slot_a << 6, aid_b, aid_a, episode, r, pet, cell, n_cells, speed_a bits, x_b, y_b,
 * heading_b, speed_b bits, hq_a, hq_b}: b = n entered, a = s had left; poses and speeds of record r.
 * Order.  The rows of one record take the ids n_rows, n_rows + 1, ... in ascending (scene, slot_b, slot_a) order; an id >= max_rows is not
 * stored and counts as dropped.  No atomic decides an id. ---- */
#define COPO_PET_WORDS 16
#define COPO_PET_MAX_WINDOW 4096
#define COPO_PET_TYPES 3
typedef struct copo_pet_cfg {
    float x0, y0;              /* m, finite (COPO_ERR_CONFIG) */
    float cell;                /* m, > 0 and finite (COPO_ERR_DIM), 1 / cell finite and cell <= 2 hw / sqrt(2) (COPO_ERR_CONFIG) */
    int32_t W, H;              /* cells, 1..COPO_FIELD_MAX_SIDE each (COPO_ERR_DIM) */
    int32_t G;                 /* scene groups, 1..COPO_FIELD_MAX_GROUPS (COPO_ERR_DIM) */
    int32_t window;            /* records a stamp stays valid for = bins of the histogram, 1..COPO_PET_MAX_WINDOW (COPO_ERR_DIM) */
    int32_t critical_records;  /* >= 0 (COPO_ERR_DIM): encounters with pet <= this count in the critical map */
    int32_t max_rows;          /* pool size, >= 1 (COPO_ERR_DIM) */
} copo_pet_cfg;
typedef struct copo_pet copo_pet;
/* allocates 8 E H W bytes of grid, 20 E N + 16 E bytes of memory, the aggregates (8 G (3 window + H W)) and the pool (64 max_rows):
 * COPO_ERR_DEVICE when the device refuses.  Every scene is in group 0 */
int copo_pet_create(copo_sim* sim, const copo_pet_cfg* cfg, copo_pet** out);
/* group_dev: device int32 [E]; scene e adds to the aggregates of group_dev[e], a value outside 0..G-1 to none (its rows are written) */
int copo_pet_set_groups(copo_pet* h, const int32_t* group_dev, void* stream);
/* one record of the current state.  Four launches on `stream`, no allocation, no host synchronisation; simulator memory is only read */
int copo_pet_record(copo_pet* h, void* stream);
/* epoch = the next record's number in every scene and every `met` mask cleared: no stamp written so far is valid any more (after a
 * reset or set_state by hand) */
int copo_pet_forget(copo_pet* h, void* stream);
/* HOST output: out[0] = rows stored so far (<= max_rows), out[1] = rows dropped; the one call that waits for `stream` */
int copo_pet_count(copo_pet* h, int64_t* out, void* stream);
/* rows [first, first + n) of the pool, device to device: rows_out [n][COPO_PET_WORDS] int32; first + n <= max_rows (COPO_ERR_DIM) */
int copo_pet_read(copo_pet* h, int32_t first, int32_t n, int32_t* rows_out, void* stream);
/* copies of hist int64 [G][COPO_PET_TYPES][window] and critical int64 [G][H][W], device to device; either may be NULL, not both */
int copo_pet_aggregates(copo_pet* h, int64_t* hist_dev, int64_t* critical_dev, void* stream);
/* copies of the stamps uint64 [E][H][W] and the met masks uint64 [E][N], device to device; either may be NULL, not both */
int copo_pet_memory(copo_pet* h, uint64_t* grid_dev, uint64_t* met_dev, void* stream);
/* n_rows = dropped = 0; stamps, masks, aggregates and the record count stay */
int copo_pet_clear(copo_pet* h, void* stream);
/* forget everything but the groups: rows, counters, stamps, masks, aggregates; records count from 0 again */
int copo_pet_reset(copo_pet* h, void* stream);
int copo_pet_destroy(copo_pet* h);

/* ---- evaluation recorder: ONE row per finished WHOLE scene episode, the reference's evaluation table (RecorderEnv.get_episode_result,
 *      copo/eval/recoder.py:188-349, what eval/evaluate_population.py writes out) for E scenes, folded on the device from the sampler's
 *      fragments.  A handle observes no simulator: it lives on the device that is current at create and reads
 *      the five tensors of a fragment in place.  Replaces, per step and scene: on_episode_step (recoder.py:107-127: step means of
 *      velocity and neighbour count, own / neighbourhood reward per agent :49-70), on_episode_end (:129-152: outcome counts) and
 *      get_episode_result (:188-299 rates, reward / cost / length statistics; :326-347 the SVO estimate).  Energy columns: left out.
 * State, all fp64, carried across fragments: per scene the accumulators of a row and an int64 count of finished episodes, per slot the
 * current occupant's cost, own-reward and neighbour-reward sums.
 * Step t of scene e, ignored once the scene has finished `limit` episodes (limit 0: never).  resetting = any slot carries
 * COPO_F_ENV_RESET; acted = COPO_F_ACTED; present = acted | (COPO_F_SPAWNED & ~resetting); done = acted & COPO_F_DONE.
 *   steps += 1; with an acting slot: v = mean velocity over them, vsteps += 1, vsum += v, vmin / vmax; with a present slot: m = mean
 *   nbr_cnt over them, nsteps += 1, nsum += m, nmax.  Slot: acted: cost += info cost; present: own += rew, nei += (nbr_cnt > 0 ?
 *   nei_rew : rew).  done: agents, success / crash / out counts by the flags, sum / min / max of info episode_reward and of the slot's
 *   cost, sum of info episode_length (and over the successful); alpha = degrees(atan2(nei, own)), svo = clamp(alpha, 0, 90): count,
 *   sum, min, max of svo, svo_reward += hypot(nei, own) * cos(radians(svo - alpha)); then cost = own = nei = 0.  A row with
 *   COPO_F_DONE | COPO_F_SPAWNED is the acting agent's: the new occupant starts at zero sums.
 *   resetting: with agents > 0 ONE row; then episodes += 1 and the accumulators start over (the slots' sums stay).
 * Row, COPO_RECORDER_NCOL fp64 values: the 25 columns of copo_amd/eval/vec_recorder.py COLUMNS in their order, svo_estimate_deg_mean /
 * _min / _max, svo_reward (sum / agents), scene, episode index of the scene (episodes finished before this one).
 * Order.  Every sum over slots has ONE fixed order (csrc/recorder_common.h), so rows do not depend on how the steps are cut into
 * fragments.  The rows of one call take the ids n_rows, n_rows + 1, ... in (scene, step) order; an id >= max_rows is not stored and
 * counts as dropped.  No atomic decides an id or adds to a sum. ---- */
#define COPO_RECORDER_NCOL 31
#define COPO_RECORDER_MAX_SLOTS 256
typedef struct copo_recorder copo_recorder;
/* E >= 1, N in 1..COPO_RECORDER_MAX_SLOTS, max_rows >= 1, limit >= 0 (COPO_ERR_DIM, checked before the device is touched).  Allocates
 * 248 max_rows + 24 E N + 216 E bytes: COPO_ERR_DEVICE when the device refuses */
int copo_recorder_create(int32_t E, int32_t N, int32_t max_rows, int32_t limit, copo_recorder** out);
/* one fragment of T >= 1 steps, device arrays: flags u8 [T][E][N], infos fp32 [T][E][N][COPO_INFO_DIM] (16-byte aligned,
 * COPO_ERR_CONFIG), rewards, nei_rewards fp32 [T][E][N], nbr_cnt int32 [T][E][N].  Three launches on `stream` whatever T is, no
 * allocation, no host synchronisation; the inputs are only read */
int copo_recorder_add(copo_recorder* h, const uint8_t* flags, const float* infos, const float* rewards, const float* nei_rewards,
                      const int32_t* nbr_cnt, int32_t T, void* stream);
/* HOST output: out[0] = rows stored so far (<= max_rows), out[1] = rows dropped; waits for `stream` */
int copo_recorder_count(copo_recorder* h, int64_t* out, void* stream);
/* rows [first, first + n) of the pool, device to device: rows_out [n][COPO_RECORDER_NCOL] fp64; first + n <= max_rows (COPO_ERR_DIM) */
int copo_recorder_read(copo_recorder* h, int32_t first, int32_t n, double* rows_out, void* stream);
/* a copy of the finished-episode counts, device to device: episodes_dev int64 [E] */
int copo_recorder_episodes(copo_recorder* h, int64_t* episodes_dev, void* stream);
/* n_rows = dropped = 0; the open episodes, the slots' sums and the episode counts stay */
int copo_recorder_clear(copo_recorder* h, void* stream);
/* forget everything: rows, counters, accumulators, slot sums, episode counts */
int copo_recorder_reset(copo_recorder* h, void* stream);
int copo_recorder_destroy(copo_recorder* h);

/* ---- stateless ops ---- */

/* CCEnv._update_distance_map + _find_in_range (env_wrappers.py:125-158) + LCFEnv reward block (:313-326).
 * pos [E][N][2] fp32, present [E][N] u8, rew [E][N] (may be NULL -> no reward outputs). */
int copo_neighbours_f32(const float* pos, const uint8_t* present, const float* rew, int32_t E, int32_t N, int32_t K,
                        float radius, float mf_distance, int32_t* nbr_idx, int32_t* nbr_cnt, int32_t* mf_cnt,
                        float* nbr_dist, float* nei_rew, float* glob_rew, void* stream);

/* Three GAE heads in one segmented reverse scan over [T][M] (M = E*N columns):
 * compute_advantages (algo_ccppo.py:362-373), compute_nei_advantage / compute_global_advantage
 * (algo_copo.py:189-204, 492-500).  rew/val/adv/tgt: [3][T][M]; flags [T][M] (ACTED/DONE bits);
 * gamma[heads] (HOST doubles); bootstrap = value of the segment's LAST row unless DONE.  Rows without ACTED get 0. */
int copo_gae3_f32(const float* rew, const float* val, const uint8_t* flags, int32_t T, int32_t M, int32_t heads,
                  const double* gamma, double lam, float* adv, float* tgt, void* stream);

/* mean_field_ccppo_process / concat_ccppo_process (algo_ccppo.py:225-311) over [T][E][N] rows.
 * obs [R][N][O], act [R][N][A], flags [R][N], nbr_idx [R][N][K], cnt [R][N] (mf: mf_cnt, concat: nbr_cnt),
 * with R = T*E.  cc_obs [R][N][C]: C = 2O+A (mf, counterfactual), 2O (mf), O+k(O+A) / O+kO (concat). */
int copo_cc_fuse_mf_f32(const float* obs, const float* act, const uint8_t* flags, const int32_t* nbr_idx,
                        const int32_t* cnt, int32_t R, int32_t N, int32_t O, int32_t A, int32_t K,
                        int32_t counterfactual, float* cc_obs, void* stream);
int copo_cc_fuse_concat_f32(const float* obs, const float* act, const uint8_t* flags, const int32_t* nbr_idx,
                            const int32_t* cnt, int32_t R, int32_t N, int32_t O, int32_t A, int32_t K,
                            int32_t num_neighbours, int32_t counterfactual, float* cc_obs, void* stream);

/* CoPOTrainer.training_step coordinated-advantage block (algo_copo.py:539-551):
 *   A_c = cos(lcf*pi/2)*adv + sin(lcf*pi/2)*nei_adv ; stats of A_c and glob_adv over valid rows;
 *   norm_adv = (A_c-mean)/max(1e-4,std) ; glob_adv_std likewise (population std).
 * Two-phase for data-parallel runs: `_partial` writes {count, sum, sumsq} x2 as doubles stats[0..5]
 * (caller all-reduces those six), `_apply` consumes the (reduced) stats.  `stats` is a device workspace of
 * COPO_LCF_STATS_DOUBLES doubles (per-block partials live behind the six results; the reduction order is
 * fixed, so results are run-to-run deterministic).  valid [B] u8 may be NULL. */
int copo_lcf_mix_partial_f32(const float* adv, const float* nei_adv, const float* glob_adv, const float* lcf,
                             const uint8_t* valid, int64_t B, float* mixed, double* stats, void* stream);
int copo_lcf_mix_apply_f32(const float* mixed, const float* glob_adv, const uint8_t* valid, int64_t B,
                           const double* stats, float* norm_adv, float* glob_adv_std, void* stream);

/* Sums behind `MultiAgentDrivingCallbacks.on_episode_end / on_train_result` (utils/callbacks.py:48-110) over the
 * n_rows rows of one iteration (flags u8, info [n_rows][COPO_INFO_DIM], nbr_cnt i32): out15[0..7] over rows that acted
 * and terminated = {count, arrive, crash, out_of_road, max_step, sum info[5], info[6], info[7]}, out15[8..14] over rows
 * that acted = {count, sum info[0..4], sum nbr_cnt}. */
int copo_episode_metrics(const uint8_t* flags, const float* info, const int32_t* nbr_cnt, int64_t n_rows, double* out15,
                         void* stream);

/* Row movers around the SGD loop.  copo_gather_rows_f32: dsts[s][r][:] = srcs[s][rows[r]][:] for n_src <= COPO_GATHER_MAX_SRC
 * sources of widths[s] floats per row in ONE launch (host arrays of device pointers) -- the epoch's planned rows into minibatch
 * order, after which copo_ppo_fused_step_f32 takes rows = NULL.  copo_pack_columns_f32: pack[r] = [cols[0][r] | cols[1][r] | ...]
 * (widths[c] floats each, <= COPO_PACK_MAX_COLS columns): the per-row pack the step kernels read, from the iteration's separate
 * column tensors.  (Replace RLlib's SampleBatch column handling inside `train_one_step`, algo_copo.py:555-558.) */
#define COPO_GATHER_MAX_SRC 4
#define COPO_PACK_MAX_COLS 24
int copo_gather_rows_f32(const float* const* srcs, float* const* dsts, const int32_t* widths, int32_t n_src, const int64_t* rows,
                         int64_t n_rows, void* stream);
int copo_pack_columns_f32(const float* const* cols, const int32_t* widths, int32_t n_cols, int64_t n_rows, float* pack,
                          void* stream);

/* Minibatch plan of one SGD epoch (the static-shape replacement of RLlib's shuffled minibatch iterator used by
 * `train_one_step`, algo_copo.py:555-558): from a permutation `perm` of this rank's B_local valid rows `valid_idx`,
 * minibatch k takes q + (k < r) consecutive entries of the shuffled list (q, r = divmod(B_local, n_mb)); rows / w are
 * [n_mb][mb] (padding: row 0, weight 0), denom[k] = number of rows of minibatch k over ALL ranks (B_all: HOST array of
 * `world` counts), *mb_index (may be NULL) is reset to 0.  perm NULL: the shuffle is a keyed pseudo-random permutation
 * computed in the kernel (4-round Feistel network with cycle walking, key4_host = four 32-bit words on the HOST). */
int copo_plan_epoch(const int64_t* valid_idx, const int64_t* perm, const uint32_t* key4_host, int64_t B_local, int32_t n_mb,
                    int32_t mb, const int64_t* B_all_host, int32_t world, int64_t* rows, float* w, float* denom,
                    int64_t* mb_index, void* stream);

/* ---- fused minibatch learner --------------------------------------------------------------------------------
 * Replaces, for one static-shape minibatch, `Policy.loss` + autograd + Adam of the reference
 * (algo_ippo.py:78-172, algo_ccppo.py:376-472, algo_copo.py:311-424; RLlib train_one_step, algo_copo.py:555-558)
 * and the two policy-gradient evaluations of `CoPOPolicy.meta_update` (algo_copo.py:250-278).
 * All fp32 parameters of the model live in ONE flat buffer `theta`; a net is obs -> H -> H -> out (tanh). */
typedef struct copo_net_layout {
    int64_t w1, b1, w2, b2, w3, b3;   /* offsets (floats) into theta; weights are [out][in] row-major */
    int32_t in_dim, out_dim;
} copo_net_layout;

#define COPO_HEAD_PPO 0        /* full PPO loss: policy net + value heads */
#define COPO_HEAD_META_NEW 1   /* policy net only, loss = mean(-clipped surrogate) with the global advantage */
#define COPO_HEAD_META_OLD 2   /* policy net only, loss = mean(logp(action))  (target network)           */
#define COPO_PPO_MAX_MB 1024   /* rows per minibatch supported by the fused learner */
#define COPO_META_BATCH_MAX 256        /* minibatches per copo_meta_batch_grads_f32 call */
#define COPO_META_DOT_PARTIALS 8192 /* doubles in the `dot_partials` workspace of the meta update */
#define COPO_PPO_MAX_KSPLIT 4  /* row splits of the weight-gradient GEMMs (fixed order -> deterministic sums) */
#define COPO_OPERAND_F32 0
#define COPO_OPERAND_BF16 1
#define COPO_PPO_STATS 8       /* sums of: total, policy, vf_ego, kl, entropy, vf_nei, vf_glob, advantage  */

typedef struct copo_ppo_cfg {
    int32_t mb;                /* rows per minibatch (static shape; padded rows carry weight 0) */
    int32_t hidden;            /* H: width of both hidden layers */
    int32_t act_dim;           /* 2 */
    int32_t n_value_heads;     /* 1 (IPPO / CCPPO) or 3 (CoPO: ego, neighbourhood, global) */
    int32_t pack_width;        /* floats per row of pack_src */
    int32_t col_actions, col_logp, col_dist, col_adv, col_meta_adv;  /* pack columns */
    int32_t col_vpred[3], col_vtarget[3];
    int32_t use_kl, old_value_loss;
    int32_t operand_dtype;     /* COPO_OPERAND_F32, or COPO_OPERAND_BF16: the `policy_dtype = bfloat16` configuration -- inputs,
                                  weights, activations and activation gradients are rounded to bfloat16 wherever torch.autocast
                                  rounds them, products accumulate in fp32 (the arithmetic of v_mfma_f32_*_bf16); parameters,
                                  Adam and the losses stay fp32.  Row-pass shapes, PPO head mode and copo_mlp_forward_f32 only. */
    int32_t reserved0;
    float clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff;
    float lr, beta1, beta2, eps;   /* Adam (torch.optim.Adam semantics, no weight decay) */
    copo_net_layout pol, val[3];
    int64_t n_params;          /* length of theta (floats) */
} copo_ppo_cfg;

/* floats of `workspace` needed for this configuration */
int64_t copo_ppo_workspace_floats(const copo_ppo_cfg* cfg);
/* One minibatch step.  rows [mb] index the dense sources (obs_src [R][pol.in_dim], cc_src [R][val.in_dim] or NULL
 * = obs_src, pack_src [R][pack_width]); w [mb] row weights; denom [1] = global number of valid rows (device);
 * apply_adam = 1: parameters and Adam moments are updated in the epilogues and *step is incremented;
 * apply_adam = 0: only `grad` (flat, same layout as theta) is written.  stats (may be NULL) accumulates.
 * mb_index (device int64, may be NULL = 0) selects the minibatch k: rows / w are then [n_mb][mb] tables and denom
 * is [n_mb]; bump_index = 1 increments *mb_index at the end, so that a captured hipGraph of this call walks the
 * epoch plan by itself.
 * theta_t (may be NULL): a mirror of theta, same length and offsets, in which W1 and W2 of every net are stored
 * transposed ([in][out]).  When given, the forward passes read it (coalesced B operands) and the Adam epilogue
 * keeps it current; create / refresh it with copo_transpose_weights_f32 whenever theta was changed from outside. */
int copo_ppo_fused_step_f32(const copo_ppo_cfg* cfg, float* theta, float* adam_m, float* adam_v, float* grad,
                            const float* obs_src, const float* cc_src, const float* pack_src, const int64_t* rows,
                            const float* w, const float* denom, const float* kl_coeff, int64_t* step,
                            float* workspace, float* stats, int32_t apply_adam, int32_t head_mode,
                            int64_t* mb_index, int32_t bump_index, float* theta_t, void* stream);
int copo_transpose_weights_f32(const copo_ppo_cfg* cfg, const float* theta, float* theta_t, void* stream);
/* Forward-only pass of nets [first_net, first_net + n_nets) of the layout (0 = policy, 1.. = value nets) over n_rows
 * DENSE rows: `model.forward` / `central_value_function` / `get_nei_value` / `get_global_value` of the reference's
 * models (algo_ccppo.py:74-219, algo_copo.py:96-182) for rollouts and the dense postprocess.  values [n_nets][n_rows]
 * (row of a policy net unused); for the policy net optionally dist_inputs [n_rows][4], and with eps [n_rows][2]
 * (standard normal draws) the sampled action, its log-probability and the action clipped to [-1, 1].  Needs the
 * transposed mirror theta_t and hidden in {64, 128, 256, 512}. */
int copo_mlp_forward_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, const float* obs_src,
                         const float* cc_src, int64_t n_rows, int32_t first_net, int32_t n_nets, float* values,
                         float* dist_inputs, const float* eps, float* action, float* logp, float* clipped, void* stream);
/* The policy net of a BANK of n_members parameter sets over n_members * rows_per_member dense rows in one launch: the rollout of a
 * checkpoint sweep (the reference's copo/eval.py:93-241 evaluates its checkpoints one after the other).  Member k's parameters are
 * theta + k * member_stride and its mirror theta_t + k * member_stride (member_stride >= n_params, a multiple of 4; build the mirror
 * with copo_transpose_weights_f32 once per member on its slice); row m of obs_src and of every output belongs to member
 * m / rows_per_member.  No tile of rows spans two members -- tiles are counted per member, the member is a grid dimension and a
 * member's last tile is masked -- so member k's rows hold the bits copo_mlp_forward_f32 writes for that member's parameters on that
 * slice alone; for that the kernel variant is the one copo_mlp_forward_f32 takes for rows_per_member rows.  Outputs as above
 * (dist_inputs, clipped may be NULL; eps NULL = no sampling); no value nets, no row list.  n_members in 1..65535. */
int copo_mlp_forward_bank_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                              int32_t n_members, int64_t rows_per_member, const float* obs_src, float* dist_inputs,
                              const float* eps, float* action, float* logp, float* clipped, void* stream);
/* SEAT mode of the bank (cross-play): every row ("seat") of the shared [n_out] sources and outputs may belong to any member.  Member k
 * owns the row list rows[k * cap .. k * cap + counts[k]) (rows: device int64 [n_members][cap]; counts: device int32 [n_members], each in
 * 0..cap, 0 is legal); it reads obs_src / eps at those rows, writes dist_inputs / action / logp / clipped at those rows and uses the
 * parameters theta + k * member_stride.  Rows in no list are not written.  Row indices (0 <= row < n_out, no row twice) are the
 * caller's contract, as in copo_mlp_forward_rows_f32.  Grid ceil(cap / 16) x n_members; a workgroup past its member's count leaves at
 * once, a member's last tile is masked as the last tile of a launch of its rows alone.
 * Variant: how many rows a member holds is known on the device only, so seat mode ALWAYS takes the one-tile kernel, also at hidden 256
 * and whatever cap is.  A member's rows therefore hold the bits of the one-tile single-member kernel: what copo_mlp_forward_f32 writes
 * for that member's parameters on its gathered rows at every hidden width -- at hidden 256 as long as that launch has fewer than
 * 2 * 32 * 256 rows (from there on copo_mlp_forward_f32 takes the two-tile variant, which rounds a few rows in ten thousand
 * differently).  NULL rows / counts: COPO_ERR_NULL; cap < 1, n_out < 1, n_members outside 1..65535 or a member_stride the bank entry
 * refuses: COPO_ERR_DIM; a refused call launches nothing. */
int copo_mlp_forward_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                               int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                               const float* obs_src, float* dist_inputs, const float* eps, float* action, float* logp, float* clipped,
                               void* stream);
/* Adversarial observation of a seated bank (eval/adversary.py): one gradient-sign step on the columns
 * [col_lo, col_hi) of every listed row, against the policy that drives the row.  Member k owns the row list of seat mode (rows, counts,
 * cap, n_out as in copo_mlp_forward_seats_f32; rows in no list are not written).  A row's level is
 * levels[level_of[group[row / n_slots]][k]] = (eps, steer, throttle, 0): with mu = the first two outputs of member k's policy net on the
 * TRUE row o of obs_src and J = steer mu_0 + throttle mu_1, g = dJ/do and
 *     obs_seen[row][j] = clamp(o[j] + eps sign(g[j]), 0, 1) for col_lo <= j < col_hi (sign(0) = 0), o[j] bit for bit elsewhere.
 * A row passes through bit for bit, with no arithmetic on it, when its level index or its group is out of range, when eps == 0 or when
 * steer == throttle == 0.  grad (device [n_out][in_dim] or NULL): g of every listed row, zeros for rows whose level is out of range or
 * has steer == throttle == 0; with grad given, rows at eps == 0 still get their gradient (a per-beam saliency) and pass through.
 * One launch, grid ceil(cap / 16) x n_members, always the 16-row tile; forward and backward run in the same workgroup, W1 / W2 of the
 * forward from the mirror theta_t, those of the backward from theta as stored.  No atomics, fixed summation order: two launches give
 * the same bits.  fp32 operands and hidden in {64, 128, 256, 512} only (else COPO_ERR_DIM, as for n_out % n_slots != 0, columns
 * outside [0, in_dim], cap < 1, n_members outside 1..65535, a member_stride the bank entry refuses); NULL theta / theta_t / rows / counts / obs_src /
 * obs_seen / group / level_of / levels: COPO_ERR_NULL.  A refused call launches nothing. */
int copo_adv_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                           int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                           const float* obs_src, float* obs_seen, float* grad, int32_t col_lo, int32_t col_hi, int32_t n_slots,
                           const int32_t* group, int32_t n_groups, const int32_t* level_of, const float* levels,
                           int32_t n_levels, void* stream);
/* Iterated adversarial observation of a seated bank (eval/pgd.py): projected gradient descent on the columns
 * [col_lo, col_hi) of every listed row, against the policy that drives the row, all iterations in one launch.  The seat-mode arguments,
 * obs_src, obs_seen, the columns, n_slots, group and level_of are those of copo_adv_obs_seats_f32.  A level is eight 32-bit words:
 * eps >= 0, steer, throttle, alpha >= 0 (f32), iters, flags (i32; bit 0 RANDOM_START, bit 1 UNTARGETED), two zeros.  With
 * it = min(iters, max_iters) and o the TRUE row:
 *     x_0 = o; under RANDOM_START x_0[j] = clamp(o[j] + eps u, 0, 1) on the columns, u = 2 uniform01(h) - 1,
 *           h = hash_rng(seed, row, tick[row], j - col_lo, 40) of sim_math.h
 *     i < it: g = dJ/dx at x_i; J = steer mu_0 + throttle mu_1, or under UNTARGETED J = |mu(x) - mu(o)|^2 / 2;
 *           y = x_i[j] + alpha sign(g[j]) (sign(0) = 0); y = min(max(y, o[j] - eps), o[j] + eps); x_{i+1}[j] = min(max(y, 0), 1)
 *     obs_seen[row] = x_it on the columns, o[j] bit for bit elsewhere; every sum and product is rounded once.
 * A row passes through bit for bit, with no arithmetic on it, when its level index or its group is out of range, when eps == 0, when
 * it <= 0, or when the level is targeted with steer == throttle == 0; rows in no list are not written.  iters = 1, alpha = eps,
 * flags = 0 is copo_adv_obs_seats_f32's step.  tick (device int32 [n_out] or NULL, which reads as 0) counts the calls: every listed
 * valid row reads tick[row] and gets tick[row] + 1 back, at every level, so a captured graph draws fresh starts at every replay (a row
 * sits in one member's list at the most).  trace (device float [max_iters][n_out][in_dim] or NULL): g of iteration i of every
 * attacked row for i < it, zeros for later iterations and for listed rows that pass through.  One launch, grid ceil(cap / 16) x
 * n_members, the 16-row tile with the iterate resident in LDS; no atomics: two launches from equal ticks give the same bits.
 * Refusals as copo_adv_obs_seats_f32 (NULL theta / theta_t / rows / counts / obs_src / obs_seen / group / level_of / levels:
 * COPO_ERR_NULL; bad dimensions, bfloat16 operands, a hidden width outside {64, 128, 256, 512}: COPO_ERR_DIM), and max_iters outside
 * [1, 16]: COPO_ERR_DIM.  A refused call launches nothing. */
int copo_pgd_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                           int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                           const float* obs_src, float* obs_seen, int32_t col_lo, int32_t col_hi, int32_t n_slots,
                           const int32_t* group, int32_t n_groups, const int32_t* level_of, const uint32_t* levels,
                           int32_t n_levels, uint64_t seed, int32_t* tick, int32_t max_iters, float* trace, void* stream);
/* Certified bounds of a seated bank (eval/certify.py): interval bound propagation through the policy net, the
 * other side of the two attacks above -- for every listed row a box that holds the two action MEANS (before sampling and clipping)
 * under every perturbation of the columns [col_lo, col_hi) inside an L-infinity budget.  The seat-mode arguments, obs_src, the columns,
 * n_slots, group and level_of are those of copo_adv_obs_seats_f32.  A level is four f32 words: eps >= 0, delta_steer >= 0,
 * delta_throttle >= 0, 0 (the deltas are read by copo_certify_tally only).  With o the TRUE row:
 *     lo[j] = max(o[j] - eps, 0), hi[j] = min(o[j] + eps, 1) on the columns, lo = hi = o[j] elsewhere; c0 = (lo + hi) / 2, r0 = (hi - lo) / 2
 *     layers i = 1, 2: zc = W_i c + b_i, zr = |W_i| r; l = tanh(zc - zr), u = max(tanh(zc + zr), l); c = (l + u) / 2, r = (u - l) / 2
 *     heads a = 0, 1:  mc = W3[a] . c + b3[a], mr = |W3[a]| . r; lo_a = (mc - mr) - pad, hi_a = (mc + mr) + pad, each sum rounded once
 *     bounds[row] = lo_0, hi_0, lo_1, hi_1, mu_0(o), mu_1(o), valid = 1.0, eps   (mu(o): the clean pass of the same launch)
 * fp32 sums are not rounded outward: the bounds are sound up to fp32 rounding, and pad >= 0 widens every bound by exactly pad.  A listed
 * row whose level index or group is out of range gets eight zeros (valid = 0); rows in no list are not written.  At eps == 0 and
 * pad == 0, lo_a == hi_a == mu_a(o) bit for bit.  One launch, grid ceil(cap / 16) x n_members, the 16-row tile three times (clean,
 * centre, radius) against one weight stream from the mirror theta_t; no atomics, fixed summation order: two launches give the same bits.
 * Refusals as copo_adv_obs_seats_f32 (NULL theta / theta_t / rows / counts / obs_src / bounds / group / level_of / levels:
 * COPO_ERR_NULL; bad dimensions, bfloat16 operands, a hidden width outside {64, 128, 256, 512}: COPO_ERR_DIM), and a negative or
 * non-finite pad: COPO_ERR_DIM.  A refused call launches nothing. */
#define COPO_CERT_WORDS 8
int copo_cert_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                            int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                            const float* obs_src, float* bounds, int32_t col_lo, int32_t col_hi, int32_t n_slots,
                            const int32_t* group, int32_t n_groups, const int32_t* level_of, const float* levels,
                            int32_t n_levels, float pad, void* stream);
/* Linear bounds of a seated bank (eval/certify.py method="linear"): copo_cert_obs_seats_f32's box, tightened by
 * one linear relaxation per tanh unit that is carried backward from each action mean to the input box.  Arguments, levels, the input
 * box and the forward pass are copo_cert_obs_seats_f32's; with l = zc - zr, u = zc + zr, tl = tanh(l), tu = max(tanh(u), tl) of a unit:
 *     lam = max(min(1 - tl^2, 1 - tu^2), 0), betaL = tl - lam l, betaU = tu - lam u   (lam z + betaL <= tanh z <= lam z + betaU on [l, u])
 *     head a: v2 = W3[a], g2 = v2 lam2; v1 = W2^T g2, g1 = v1 lam1; v0 = W1^T g1; base = b3[a] + g2 . b2 + g1 . b1 + v0 . c0, rad = |v0| . r0
 *     hiL = base + v2+ . betaU2 + v2- . betaL2 + v1+ . betaU1 + v1- . betaL1 + rad;  loL = the same with betaL / betaU exchanged, - rad
 *     (loI, hiI) = copo_cert_obs_seats_f32's box before its pad;  lo = max(loL, loI), hi = min(hiL, hiI); lo > hi (rounding): (loI, hiI)
 *     bounds[row] = lo_0 - pad, hi_0 + pad, lo_1 - pad, hi_1 + pad, mu_0(o), mu_1(o), valid = 1.0, eps   (the layout copo_certify_tally reads)
 *     parts[row]  = loL_0, hiL_0, loL_1, hiL_1, loI_0, hiI_0, loI_1, hiI_1 before the pad; parts may be NULL
 * Sound up to fp32 rounding, as the interval pass.  An invalid listed row gets eight zeros in both outputs; rows in no list are not
 * written.  One launch of copo_cert_obs_seats_f32's shape and LDS at every hidden width (layer 1's intervals are recomputed behind
 * the W2 pass, not kept); no atomics, fixed summation order: two launches give the same bits.  Refusals are
 * copo_cert_obs_seats_f32's; a refused call launches nothing. */
int copo_lin_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                           int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                           const float* obs_src, float* bounds, float* parts, int32_t col_lo, int32_t col_hi, int32_t n_slots,
                           const int32_t* group, int32_t n_groups, const int32_t* level_of, const float* levels,
                           int32_t n_levels, float pad, void* stream);
/* Input attribution of a seated bank (eval/attribution.py): integrated gradients of the two action MEANS of every
 * listed row with respect to its whole observation row, against the policy that drives the row, all quadrature points in one launch.
 * The seat-mode arguments, obs_src, n_slots, group and level_of are those of copo_adv_obs_seats_f32; col_lo / col_hi are checked as
 * there and not read (every column is attributed).  A level is four 32-bit words: m (i32, the quadrature points), flags (i32, reserved,
 * 0), two zeros; base (device fp32 [n_levels][in_dim]) holds a baseline row per level, a NaN entry meaning "this column keeps the row's
 * own value".  With mm = min(m, max_points), o the TRUE row, b[j] = isnan(base[j]) ? o[j] : base[j] and d = o - b:
 *     x_s = b + ((s - 1/2) / mm) d, s = 1 .. mm (midpoint rule);  G_a = sum_s d mu_a / d x at x_s, s ascending (a = 0 steer, 1 throttle)
 *     attr[row][a][j] = (d[j] G_a[j]) / mm, exactly 0.0 where d[j] == 0;  gap_a = (mu_a(o) - mu_a(b)) - sum_j attr[row][a][j], j ascending
 *     heads[row] = mu_0(o), mu_1(o), mu_0(b), mu_1(b), gap_0, gap_1, valid = 1.0, mm as bits
 * every difference, quotient, product and sum above rounded once in fp32.  The attributions of a row sum to mu_a(o) - mu_a(b) up to the
 * quadrature residual gap_a, which the launch reports.  A listed row whose level index or group is out of range, or whose mm <= 0, gets
 * zeros in attr and eight zeros in heads (valid = 0); rows in no list are not written.  One launch, grid ceil(cap / 16) x n_members, the
 * 16-row tile resident in LDS with the running sums; forward from the mirror theta_t, backward on theta as stored, the two heads one
 * after the other behind one forward per point.  No atomics, fixed summation order: two launches give the same bits.  Refusals as
 * copo_adv_obs_seats_f32 (NULL theta / theta_t / rows / counts / obs_src / attr / heads / base / group / level_of / levels:
 * COPO_ERR_NULL; bad dimensions, bfloat16 operands, a hidden width outside {64, 128, 256, 512}, tiles beyond the workgroup's LDS -- hidden
 * 512 with more than 128 input columns --: COPO_ERR_DIM), and max_points outside [1, 32]: COPO_ERR_DIM.  A refused call launches nothing. */
int copo_ig_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                          int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                          const float* obs_src, float* attr, float* heads, int32_t col_lo, int32_t col_hi, int32_t n_slots,
                          const int32_t* group, int32_t n_groups, const int32_t* level_of, const int32_t* levels,
                          int32_t n_levels, const float* base, int32_t max_points, void* stream);
/* The jury pass of a seated bank (eval/jury.py): the third mode of the bank's forward.  The dense bank gives every
 * member its own rows and seat mode gives a row to ONE member; here a row may be judged by many, and each judge's distribution inputs
 * land in a plane of their own.  Member j is a judge and owns the list rows[j cap .. j cap + counts[j]) of [0, n_out) (rows device
 * [n_members][cap] int64, counts device [n_members] int32; a row may stand in the lists of several judges, at most once per list; an
 * index outside [0, n_out) is skipped).  Judge j reads the true row obs_src[r] ([n_out][pol.in_dim]), runs its own policy net on it
 * (theta + j member_stride, the mirror theta_t alike) and writes mu_steer, mu_throttle, logstd_steer, logstd_throttle to
 * verdict[r][j][0..4); verdict device fp32 [n_out][n_members][4], 16-byte aligned.  Entries that no list names are not written.
 * verdict[r][j] holds the bits copo_mlp_forward_seats_f32 writes to dist_inputs[r] when member j's list there contains r, at every
 * hidden width it supports and whichever other rows share r's tile.  No sampling, no action, no eps.  One launch, grid ceil(cap / 16) x
 * n_members, always the one-tile kernel, fp32 operands; a workgroup past its judge's count leaves before any weight load; no atomics,
 * fixed summation order: two launches give the same bits.  NULL theta / theta_t / rows / counts / obs_src / verdict: COPO_ERR_NULL;
 * cap < 1, n_out < 1, n_members outside 1..65535, member_stride below cfg->n_params or no multiple of 4, bfloat16 operands, a hidden
 * width outside {64, 128, 256, 512}, a mirror that is not 16-byte aligned: COPO_ERR_DIM.  A refused call launches nothing. */
int copo_jury_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                            int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                            const float* obs_src, float* verdict, void* stream);
/* The hidden-layer pass of a seated bank (eval/similarity.py): the fourth mode of the bank's forward, the jury pass
 * stopped behind layer 2.  Lists, parameters and launch shape as copo_jury_obs_seats_f32.  For the row r at position p of judge j's list
 * it writes h1 = tanh(W1 o + b1) to hidden[j][p][0][0..H) and h2 = tanh(W2 h1 + b2) to hidden[j][p][1][0..H): hidden device fp32
 * [n_members][cap][2][hidden], unit fastest, 16-byte aligned -- indexed by POSITION in the judge's list, which is what copo_cka_accumulate
 * stages with 128-bit loads (sixteen lanes on 256 consecutive bytes of one position).  The values are the bits the jury kernel holds in
 * its two LDS tiles for that judge and row, whichever other rows share the tile.  Positions at or past counts[j] (the masked rows of a
 * last, partial tile among them) and positions whose index lies outside [0, n_out) are not written; verdict[row][judge] is not
 * written at all.  No sampling, no atomics, fixed summation order: two launches give the same bits.  Refusals as
 * copo_jury_obs_seats_f32, with `hidden` in `verdict`'s place. */
int copo_hidden_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                              int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                              const float* obs_src, float* hidden, void* stream);
/* ---- representation similarity: linear centred kernel alignment of the hidden layers of a panel of bank members
 * on the same rows.  Stateless.  copo_cka_accumulate, once per env step: hidden as copo_hidden_obs_seats_f32 wrote it (n_members, cap, H =
 * the hidden width, a multiple of 64 up to COPO_CKA_MAX_HIDDEN); panel device [n_panel] int32, the members compared (n_panel in
 * 1..COPO_CKA_MAX_PANEL; an entry outside [0, n_members) adds nothing); rows device [cap] int64 and count device [1] int32: the common
 * list (every panel member's list is this one); flags device [n_out] uint8 (the step's output), seat device [n_out] int32; rows_of: < 0,
 * or the member whose driven rows alone are counted.  Position p is COUNTED when p < min(count, cap), 0 <= rows[p] < n_out,
 * flags[rows[p]] carries COPO_F_ACTED and (rows_of < 0 or seat[rows[p]] == rows_of).  With P = n_panel (n_panel + 1) / 2 pairs a <= b of
 * panel indices, pair (a, b) at index a n_panel - a (a - 1) / 2 + (b - a), over the counted positions and both layers l:
 *     S[r][pair][l][i][j] += sum_p h_a,l[p][i] h_b,l[p][j]     s[r][a][l][i] += sum_p h_a,l[p][i]     n[r] += counted positions
 * S device float64 [n_planes][P][2][H][H], s device float64 [n_planes][n_panel][2][H], n device int64 [n_planes]; plane r holds the
 * chunks r, r + n_planes, ... of COPO_CKA_CHUNK positions (n_planes in 1..COPO_CKA_MAX_PLANES is the caller's: a fixed row split that
 * fills the chip at a small panel, a property of the plan and never of the device).  The products are accumulated in fp32 on
 * v_mfma_f32_16x16x4_f32 and added to the float64 accumulator after every COPO_CKA_PROMOTE_ROWS positions of a plane and at the end of
 * the launch; every accumulator element has one owner and one order, no atomics: the same sequence of launches leaves the same bits.  A
 * position that is not counted contributes exact zeros whatever the workspace holds there.  All three outputs ACCUMULATE (the caller
 * clears them).  copo_cka_finish: the planes summed in plane order, n = sum_r n[r], then in float64 with a fixed summation order
 *     hsic[a][b][l] = || S[a,b,l] - s[a,l] s[b,l]^T / n ||_F^2      (hsic device float64 [n_panel][n_panel][2], both triangles)
 *     mean[a][l][i] = s[a,l][i] / n,   var[a][l][i] = S[a,a,l][i][i] / n - mean^2      (device float64 [n_panel][2][H] each)
 * and *n_out = n (device int64); with n < 2 every float64 output is zero.  Linear CKA is hsic[a][b] / sqrt(hsic[a][a] hsic[b][b]), the
 * host's to form.  One launch each on the caller's stream, no allocation, no host synchronisation; both may be captured in a graph.
 * NULL pointers: COPO_ERR_NULL; dimensions outside the ranges above, rows_of >= n_members, a hidden pointer that is not 16-byte
 * aligned: COPO_ERR_DIM; a refused call launches nothing. */
#define COPO_CKA_CHUNK 32
#define COPO_CKA_PROMOTE_ROWS 128
#define COPO_CKA_MAX_PLANES 8
#define COPO_CKA_MAX_PANEL 255
#define COPO_CKA_MAX_HIDDEN 512
int copo_cka_accumulate(const float* hidden, int32_t n_members, int64_t cap, int32_t H, const int32_t* panel, int32_t n_panel,
                        const int64_t* rows, const int32_t* count, const uint8_t* flags, const int32_t* seat, int64_t n_out,
                        int32_t rows_of, int32_t n_planes, double* S, double* s, int64_t* n, void* stream);
int copo_cka_finish(const double* S, const double* s, const int64_t* n, int32_t n_panel, int32_t H, int32_t n_planes, double* hsic,
                    int64_t* n_out, double* mean, double* var, void* stream);
/* ---- linear probes (eval/probes.py; ABI 8, new symbols): the sufficient statistics of ridge regressions from feature
 * blocks (the hidden layers copo_hidden_obs_seats_f32 keeps, the observation as a control) to per-row targets, on a train and a test fold.
 * Stateless.  Lists as copo_cka_accumulate: rows device [cap] int64, count device [1] int32, the common list.
 * copo_probe_targets, once per env step behind the simulator step, one wave per position p < min(count, cap) whose row r = rows[p] lies
 * in [0, n_out): obs device fp32 [n_out][obs_dim], the observation the policy read; the LiDAR block is columns lidar_lo .. lidar_lo +
 * num_lasers (beam 0 looks ahead, beam k is turned clockwise); trig device fp32 [num_lasers][2] = (cos, sin)(2 pi k / num_lasers), the
 * host's float64 values rounded to fp32; flags device [n_out] uint8 and reward device fp32 [n_out], the step's outputs.  It writes
 * targets[p][0..COPO_PROBE_PANEL): [0] nearest = the least beam (1 where no beam is below 1), [1] / [2] (1 - nearest) cos / sin of the LOWEST
 * beam at that value (0 where no beam is below 1), [3] the share of beams below 1, [4] the least beam of the front quadrant (the beams k
 * with ((k + n / 8) % n) 4 / n == 0; 1 at the most), [5] reward[r], [6] / [7] 1.0 where flags[r] carry COPO_F_CRASH / COPO_F_DONE, else
 * 0.0; [COPO_PROBE_TARGETS .. 14] 0.0; [15] 1.0 -- and xobs[p][0..padded_dim) = obs[r], 0.0 beyond obs_dim (padded_dim a multiple of 64
 * from obs_dim up to COPO_PROBE_MAX_WIDTH).  Other positions are not written.  Every fold over lanes is a total order or an integer sum:
 * two launches give the same bits, and they are the bits of the same individually rounded fp32 operations on the host.
 * copo_probe_accumulate, once per env step and workspace: x device fp32, x_floats floats, 16-byte aligned; block b in [0, n_blocks) is
 * the width features at x[block_base[b] + p pos_stride ..) of every position p (block_base device [n_blocks] int64; a base that is
 * negative, no multiple of 4 or does not hold cap positions inside x_floats adds nothing); targets device fp32 [cap][COPO_PROBE_PANEL];
 * fold device uint8 [n_out / slots], the fold of the scene r / slots: 0 train, 1 test, COPO_PROBE_FOLD_NONE never counted.  Position p
 * is COUNTED in fold f when copo_cka_accumulate would count it and fold[rows[p] / slots] == f.  Over the counted positions
 *     G[r][f][b][i][j] += sum_p x_b[p][i] x_b[p][j]      (only the 64 x 64 tiles with i / 64 <= j / 64; the others are never written)
 *     C[r][f][b][i][c] += sum_p x_b[p][i] targets[p][c]  T[r][f][c][d] += sum_p targets[p][c] targets[p][d]
 * G device float64 [n_planes][2][n_blocks][width][width], C [n_planes][2][n_blocks][width][16], T [n_planes][2][16][16] (with column 15
 * == 1: C[..][15] the unit sums, T[15][15] the counted rows).  Planes, fp32 v_mfma_f32_16x16x4_f32 partials, promotion every
 * COPO_CKA_PROMOTE_ROWS positions of a plane, one owner and one order per element, masking of the operands and accumulation as
 * copo_cka_accumulate.  One launch each on the caller's stream, grid (nt (nt + 1) / 2 + 1) x n_blocks x 2 n_planes with nt = width / 64;
 * no allocation, no host synchronisation; both may be captured in a graph.  NULL pointers: COPO_ERR_NULL; width no multiple of 64 in
 * 64..COPO_PROBE_MAX_WIDTH, n_blocks outside 1..COPO_PROBE_MAX_BLOCKS, n_planes outside 1..COPO_CKA_MAX_PLANES, cap or n_out < 1, n_out no
 * multiple of slots, pos_stride below width or no multiple of 4, cap positions beyond x_floats, num_lasers < 1 or a LiDAR block outside
 * the row, a misaligned x: COPO_ERR_DIM; a refused call launches nothing. */
#define COPO_PROBE_TARGETS 8
#define COPO_PROBE_PANEL 16
#define COPO_PROBE_MAX_WIDTH 512
#define COPO_PROBE_MAX_BLOCKS 510
#define COPO_PROBE_FOLD_NONE 255
int copo_probe_targets(const float* obs, int64_t n_out, int32_t obs_dim, int32_t lidar_lo, int32_t num_lasers, const float* trig,
                       const uint8_t* flags, const float* reward, const int64_t* rows, const int32_t* count, int64_t cap, float* targets,
                       float* xobs, int32_t padded_dim, void* stream);
int copo_probe_accumulate(const float* x, int64_t x_floats, const int64_t* block_base, int32_t n_blocks, int64_t pos_stride, int32_t width,
                          const float* targets, const int64_t* rows, const int32_t* count, int64_t cap, const uint8_t* flags,
                          const int32_t* seat, const uint8_t* fold, int64_t n_out, int32_t slots, int32_t rows_of, int32_t n_planes, double* G,
                          double* C, double* T, void* stream);
/* ---- low-precision policy forward of a seated bank (eval/precision.py; ABI 8, new symbols).  A format is
 * COPO_LOWP_BF16 (bfloat16) or COPO_LOWP_E4M3 (OCP float8 e4m3fn: no infinities, largest value 448).  rnd rounds to nearest even into the
 * format (e4m3: after a clamp to [-448, 448]; subnormals kept).
 * copo_lowp_pack writes, for each of n_members members (parameters theta + k member_stride floats, the policy net of cfg), the image
 * packed + k packed_stride BYTES: q1 [hidden][K1P] and q2 [hidden][hidden] elements of the format, output-unit-major with k contiguous,
 * K1P = in_dim rounded up to a multiple of 32 and zero beyond in_dim; then fp32 words q3 [4][hidden], s1 [hidden], s2 [hidden], s3 [4],
 * b1 [hidden], b2 [hidden], b3 [4].  s_l[u] is 1 for bfloat16 and, for e4m3, the smallest power of two with max_k |W_l[u][k]| / s <= 448
 * (1 for a zero row); q_l[u][k] = rnd(W_l[u][k] / s_l[u]); the biases are fp32 as stored for e4m3 and rounded to bfloat16 for bfloat16
 * (the places COPO_OPERAND_BF16 rounds).  packed: device, 16-byte aligned, packed_stride a multiple of 16 and at least the image's size,
 * hidden * (K1P + hidden) * (2 or 1) + 4 * (8 * hidden + 8) bytes.  Outside captured graphs or inside, one launch.
 * copo_lowp_forward_seats is copo_mlp_forward_seats_f32 on such images: the same lists (rows, counts, cap, n_out; a count above cap is
 * cap, an index outside [0, n_out) is skipped, rows in no list are not written), grid ceil(cap / 16) x n_members, a workgroup past its
 * member's count leaves before any weight load.  Per listed row with observation o: x = rnd(o); h1 = rnd(tanh(z1)), z1 = s1 (q1 x) + b1;
 * h2 alike from h1; dist_inputs = s3 (q3 h2) + b3; for bfloat16 z1, z2 and the four outputs are themselves rounded to bfloat16, as
 * COPO_OPERAND_BF16 does.  Both hidden layers run on the 16x16x32 matrix instruction of the format with fp32 accumulation (e4m3: one k per lane group and
 * issue, the partial sums added in fp32 on the lanes, because the instruction's own sum over a lane's eight k is narrower), the heads in fp32
 * on the lanes; fixed order, no atomics: two launches give the same bits.  From dist_inputs on the outputs (eps, action, logp, clipped:
 * as copo_mlp_forward_f32) are those of copo_mlp_forward_seats_f32: equal dist_inputs bits give equal action, logp and clipped bits.
 * One launch serves one format: members of another format get a count of 0.  NULL cfg / packed / rows / counts / obs_src, neither
 * dist_inputs nor eps, eps without action and logp: COPO_ERR_NULL; another fmt, hidden outside {64, 128, 256, 512}, in_dim < 1, n_members
 * outside 1..65535, cap < 1, n_out < 1, a short or misaligned image, an input so wide that the tiles pass 64 KiB of LDS: COPO_ERR_DIM.
 * A refused call launches nothing. */
#define COPO_LOWP_BF16 1
#define COPO_LOWP_E4M3 2
int copo_lowp_pack(const copo_ppo_cfg* cfg, const float* theta, int64_t member_stride, int32_t n_members, int32_t fmt, void* packed,
                   int64_t packed_stride, void* stream);
int copo_lowp_forward_seats(const copo_ppo_cfg* cfg, const void* packed, int64_t packed_stride, int32_t fmt, int32_t n_members,
                            const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out, const float* obs_src,
                            float* dist_inputs, const float* eps, float* action, float* logp, float* clipped, void* stream);
/* host only (tests): out[i] = rnd(in[i]) in fmt, and the e4m3 scale of a row whose largest magnitude is amax[i] -- the code the kernels run */
int copo_debug_lowp_round(int32_t fmt, const float* in, int64_t n, float* out);
int copo_debug_lowp_scale(const float* amax, int64_t n, float* out);
/* The same pass over a LIST of rows: launch row m reads row rows[m] of the sources ([n_src_rows][..]) and writes
 * values[net][rows[m]] (values is [n_nets][n_src_rows]; entries of unlisted rows are left alone).  The dense postprocess
 * of a rollout buffer uses it with the rows that hold an agent -- about half of the slots. */
int copo_mlp_forward_rows_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, const float* obs_src,
                              const float* cc_src, const int64_t* rows, int64_t n_rows, int64_t n_src_rows,
                              int32_t first_net, int32_t n_nets, float* values, void* stream);

/* ---- critic audit (eval/critics.py) ------------------------------------------------------------------------
 * copo_value_obs_seats_f32: the VALUE nets of a seated bank in one launch.  rows / counts / cap / n_out are seat mode's
 * (copo_mlp_forward_seats_f32); for every row r of member k's list and head h in [0, n_value_heads)
 *     values[r][h] = val[h] net of member k on cc_src[r]      (cc_src NULL = obs_src; [n_out][val[h].in_dim], one width for all heads)
 * into values [n_out][n_value_heads].  Grid ceil(cap / 16) x n_members x heads, always the 16-row tile; a workgroup past counts[k]
 * leaves before any weight load, the last tile is masked, a row index outside [0, n_out) and rows in no list are not written.  No
 * atomics, fixed summation order: two launches give the same bits, and member k's values hold the bits
 * copo_mlp_forward_rows_f32(first_net = 1, n_nets = heads) writes for that member alone on its rows at the one-tile variant.  No
 * allocation, no host synchronisation; may be captured in a graph.  NULL cfg / theta / theta_t / rows / counts / obs_src / values:
 * COPO_ERR_NULL; bfloat16 operands, hidden outside {64, 128, 256, 512}, n_value_heads outside 1..3, cap < 1, n_out < 1, n_members
 * outside 1..65535, a member_stride below n_params or no multiple of 4, a mirror that is not 16-byte aligned, heads of different
 * input widths, tiles beyond the workgroup's LDS: COPO_ERR_DIM.  A refused call launches nothing. */
int copo_value_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                             int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                             const float* obs_src, const float* cc_src, float* values, void* stream);
/* copo_audit_*: V(s_t) against the discounted return that follows it, folded forward.  Per (scene, slot, head) a float64 state lives
 * as long as the agent in the slot; head h has discount gamma[h] and the reward stream rew (0), nei_rew (1), glob_rew[e] (2).  One
 * record per env step, after the step, with V the value of the observation the agent acted on.  A slot is audited where 0 <= seat < K
 * and 0 <= group[e] < G.  For a row with COPO_F_ACTED, in this order, every operation individually rounded in float64:
 *     q = gamma^2 q + 1;  c = gamma c + 1;  z = gamma z + V;  sV += V;  sVV += V^2;  n += 1
 *     sG += r c;  sVG += r z;  sGG += r (r q + 2 gamma u);  u = gamma u + r q
 *     per bin b: e_b = gamma e_b + [bin(V) == b];  nb_b += [..];  sVb_b += V [..];  sGb_b += r e_b
 * so that with G_t = sum_{k >= t} gamma^(k - t) r_k up to the agent's last step (no bootstrap) sG = sum G_t, sVG = sum V_t G_t,
 * sGG = sum G_t^2, sGb_b = sum_{t in b} G_t.  bin(V) = floor((V - lo) / (hi - lo) * bins) clamped into [0, bins - 1] (NaN: bin 0).
 * With COPO_F_DONE on that row the agent's sums are clamped to +-2^32, quantised once to 2^-16 steps (round to nearest even) and
 * added by 64-bit integer atomics to acc[group][member][head][COPO_AUDIT_WORDS]; `agents`, `steps` and the bin counts are plain counts.
 * An agent that ends by COPO_F_MAXSTEP without ARRIVE / CRASH / OUT is truncated: it adds 1 to `truncated`, and its other words only
 * when count_truncated is set.  Then -- and on COPO_F_SPAWNED or COPO_F_ENV_RESET -- the state is zeroed: a row with DONE | SPAWNED
 * counts for the agent that acted and the new occupant starts from zero; agents still open are never counted.  The per-slot updates
 * are independent and only the commits are atomic, on integers, so the result does not depend on scheduling.
 * Range: |word| <= 2^48 per agent and sum (the clamp), so a cell holds 2^15 agents at the clamp; at the simulator's magnitudes (sums
 * of squared returns near 1e7 per agent) some 1e7 agents.
 * create: E, N, G >= 1, K in 1..65535, heads in 1..3, bins in 1..COPO_AUDIT_MAX_BINS (COPO_ERR_DIM, before the device is touched);
 * gamma in [0, 1], lo < hi finite (COPO_ERR_CONFIG).  Allocates 8 (10 + 4 bins) E N heads + 448 G K heads bytes.
 * record: flags [E][N] uint8, values [E N][heads], rew / nei_rew [E][N], glob_rew [E] fp32 (nei_rew with heads >= 2, glob_rew with
 * heads = 3, else they may be NULL), seat [E][N] and group [E] int32, all on the device; one launch, may be captured in a graph.
 * read: acc, device to device, int64 [G][K][heads][COPO_AUDIT_WORDS].  reset: state and accumulator to zero. */
#define COPO_AUDIT_AGENTS 0
#define COPO_AUDIT_STEPS 1
#define COPO_AUDIT_TRUNCATED 2
#define COPO_AUDIT_SUM_V 3
#define COPO_AUDIT_SUM_VV 4
#define COPO_AUDIT_SUM_G 5
#define COPO_AUDIT_SUM_VG 6
#define COPO_AUDIT_SUM_GG 7
#define COPO_AUDIT_BIN_COUNT 8       /* [8, 24): rows of bin b */
#define COPO_AUDIT_BIN_VALUE 24      /* [24, 40): sum of V over the rows of bin b, 2^-16 steps */
#define COPO_AUDIT_BIN_RETURN 40     /* [40, 56): sum of G over the rows of bin b, 2^-16 steps */
#define COPO_AUDIT_WORDS 56
#define COPO_AUDIT_MAX_BINS 16
typedef struct copo_audit_cfg {
    int32_t E, N, K, G;        /* scenes, slots, bank members, scene groups */
    int32_t heads, bins;
    int32_t count_truncated, reserved0;
    double gamma[3], lo[3], hi[3];
} copo_audit_cfg;
typedef struct copo_audit copo_audit;
int copo_audit_create(const copo_audit_cfg* cfg, copo_audit** out);
int copo_audit_record(copo_audit* h, const uint8_t* flags, const float* values, const float* rew, const float* nei_rew,
                      const float* glob_rew, const int32_t* seat, const int32_t* group, void* stream);
int copo_audit_read(copo_audit* h, int64_t* acc_out, void* stream);
int copo_audit_reset(copo_audit* h, void* stream);
int copo_audit_destroy(copo_audit* h);
/* Adam on the flat buffers (the data-parallel path: after the gradient all-reduce); theta_t as above or NULL.
 * workspace: the workspace of the copo_ppo_fused_step_f32(apply_adam = 0, `step` given) call that produced `grad` --
 * that call published the step number and the next minibatch index there, so this one needs no trailing counter
 * launch -- or NULL: *step + 1 is used and both counters are advanced by a separate 1-thread kernel. */
int copo_adam_step_f32(const copo_ppo_cfg* cfg, float* theta, float* adam_m, float* adam_v, const float* grad,
                       int64_t n, int64_t* step, int64_t* mb_index, float* theta_t, float* workspace, void* stream);

/* ---- data-parallel SGD step: the local step's two launches, gradients summed over the ranks INSIDE the weight-gradient
 * kernel (replaces RLlib's multi_gpu_train_one_step + the weight broadcasts, algo_copo.py:555-558, 572-613).  One process per
 * GPU; every rank owns an exchange workspace of copo_dp_workspace_bytes(cfg, world) bytes from copo_peer_alloc (uncached
 * device memory), exported / opened with copo_ipc_* so that `dp_workspaces[r]` is rank r's workspace as mapped HERE.
 * Every 32 x 32 gradient tile is sent to the rank that owns it (tile index mod world), added up there in rank order and
 * sent back; then every rank applies the same Adam update, so parameters, moments and the transposed mirror stay
 * bit-identical on all ranks without being communicated.  Arguments as copo_ppo_fused_step_f32 (PPO head mode, Adam
 * applied, `w / denom` with the GLOBAL row count in denom); every rank must make the same calls in the same order.
 * world == 1 is the local step.  A peer that does not answer within ~10 s raises an error word (copo_dp_status) instead of
 * hanging the GPU; every later wait then returns at once. */
int64_t copo_dp_workspace_bytes(const copo_ppo_cfg* cfg, int32_t world);
int copo_ppo_fused_step_dp_f32(const copo_ppo_cfg* cfg, float* theta, float* adam_m, float* adam_v, const float* obs_src,
                               const float* cc_src, const float* pack_src, const int64_t* rows, const float* w,
                               const float* denom, const float* kl_coeff, int64_t* step, float* workspace, float* stats,
                               int64_t* mb_index, int32_t bump_index, float* theta_t, void* const* dp_workspaces,
                               int32_t rank, int32_t world, void* stream);
int copo_dp_status(void* workspace, const copo_ppo_cfg* cfg, int32_t world, void* stream);

/* ---- LCF meta update (CoPOPolicy.meta_update, algo_copo.py:228-309) in three calls ------------------------------
 * (1) both policy gradients in one grouped pass: g_new = d mean(-clip-surrogate(global adv)) / d theta on the
 *     current policy, g_old = d mean(logp) / d theta_target on the target policy (flat layout; only the policy
 *     block is written).  stats_new[1] / stats_old[1] accumulate the two losses, stats_new[7] the mean advantage. */
int copo_meta_grads_f32(const copo_ppo_cfg* cfg, float* theta, float* theta_target, float* g_new, float* g_old,
                        const float* obs_src, const float* pack_src, const int64_t* rows, const float* w,
                        const float* denom, float* workspace, float* stats_new, float* stats_old,
                        double* dot_partials /* [COPO_META_DOT_PARTIALS], zero-initialised once by the caller */,
                        int64_t* mb_index, void* stream);
/* (2) fp64 LCF terms of the minibatch: tail = {dS/dp0, dS/dp1, S, mean(A')} with S = mean((A' - mu)/sigma),
 *     A' = cos(phi) A_ego + sin(phi) A_nei, phi = (lcf_mean + lcf_std * eps) * pi/2 (reparameterised sample).
 *     eps [n_mb][mb] doubles; lcf_param [2] doubles (the model's lcf_parameters); raw_mean_std [2] doubles. */
int copo_meta_lcf_f64(const float* pack_src, int32_t pack_width, int32_t col_adv, int32_t col_nei_adv,
                      const int64_t* rows, const float* w, const float* denom, const double* eps, int32_t mb,
                      const int64_t* mb_index, const double* lcf_param, const double* raw_mean_std, double* tail,
                      void* stream);
/* (3) grad_value = <g_new[0:n], g_old[0:n]> -- from the per-workgroup partials that (1) left in dot_partials, or,
 *     when dot_partials is NULL (data-parallel: the gradients were all-reduced in between), recomputed from
 *     g_new / g_old -- (fp64 accumulate), LCF gradient grad_value * tail[0:2], Adam (fp64,
 *     betas 0.9/0.999, eps 1e-8) on lcf_param in place; adam_state [5] doubles = {m0, m1, v0, v1, step};
 *     stats [7] doubles accumulate {new loss, old loss, S, grad_value*S, grad_value, mean A', mean global adv}.
 *     Data-parallel runs all-reduce g_new/g_old (and tail) between (2) and (3). */
int copo_meta_finish_f64(const float* g_new, const float* g_old, int64_t n, const double* dot_partials,
                         const double* tail, double* lcf_param, double* adam_state, double lr, float* stats_new,
                         float* stats_old, double* stats, int64_t* mb_index, int32_t bump_index, void* stream);

/* (1)+(2)+(3) in one call for the single-process case (no gradient all-reduce in between): the last workgroup of
 * the gradient fold runs the LCF part and the LCF Adam step, so a whole meta step (`CoPOPolicy.meta_update`,
 * algo_copo.py:228-309) is six kernel launches.  Arguments as in the three calls above. */
int copo_meta_step_f64(const copo_ppo_cfg* cfg, float* theta, float* theta_target, float* g_new, float* g_old,
                       const float* obs_src, const float* pack_src, const int64_t* rows, const float* w,
                       const float* denom, float* workspace, float* stats_new, float* stats_old, double* dot_partials,
                       int32_t col_adv, int32_t col_nei_adv, const double* eps, double* lcf_param,
                       const double* raw_mean_std, double* tail, double* adam_state, double lr, double* stats,
                       int64_t* mb_index, int32_t bump_index, void* stream);

/* ---- batched LCF meta pass ------------------------------------------------------------------------------------
 * The two policy gradients of `meta_update` depend on the minibatch and on the policy / target parameters, which
 * the LCF loop (algo_copo.py:581-589) does not change -- only the two LCF parameters move.  So the gradient pairs
 * of many minibatches are computed in ONE grouped launch chain (phase A), and the sequential fp64 LCF Adam steps
 * run afterwards in one kernel (phase B).  Results equal the step-by-step calls above.
 *
 * Phase A: minibatches mb_first .. mb_first + nb - 1 of the row tables (rows / w [n_mb][mb], denom [n_mb]).
 *   gv_out [nb] doubles = <g_new, g_old> of each minibatch; stats_out [nb][2][COPO_PPO_STATS] = loss statistics of
 *   the new-policy / old-policy pass; g_out NULL, or [nb][2][copo_meta_fold_len()] to export the gradients
 *   (data-parallel: all-reduce them, then copo_meta_batch_dot_f64 recomputes gv).  workspace:
 *   copo_meta_batch_workspace_floats(cfg, nb_cap) floats, 8-byte aligned, zero-initialised once; nb <= nb_cap. */
int64_t copo_meta_fold_len(const copo_ppo_cfg* cfg);
int64_t copo_meta_batch_workspace_floats(const copo_ppo_cfg* cfg, int32_t nb);
int copo_meta_batch_grads_f32(const copo_ppo_cfg* cfg, float* theta, float* theta_target, const float* obs_src,
                              const float* pack_src, const int64_t* rows, const float* w, const float* denom,
                              float* workspace, int32_t nb_cap, int64_t mb_first, int32_t nb, float* g_out,
                              double* gv_out, float* stats_out, void* stream);
/* gv_out[b] = <g[b][0], g[b][1]> (fp64 accumulation, fixed order) of exported -- all-reduced -- gradient pairs; denom (may be
 * NULL): [nb] row counts D_b, the result is scaled by 1 / D_b^2 (exported gradients of the row-store path carry unit weights).
 * partials: caller-owned scratch of nb * COPO_META_DOT_SPLIT doubles (stream-ordered like every other argument: calls on different
 * streams need different scratch), or NULL: one workgroup per minibatch, no scratch, slower. */
#define COPO_META_DOT_SPLIT 8
int copo_meta_batch_dot_f64(const float* g /* [nb][2][n] */, int64_t n, int32_t nb, double* gv_out, const float* denom, double* partials,
                            void* stream);
/* Row store.  Everything of phase A that is local to a ROW (both forward passes, the loss gradients, the activation
 * gradients -- with unit row weight) does not depend on how a meta pass groups the rows into minibatches, and the
 * `lcf_num_iters` passes of one training iteration regroup the same rows.  copo_meta_rows_f32 computes it once for rows
 * [0, n_rows) of the dense sources into rows_ws (copo_meta_rows_workspace_floats floats) + rowstat [2 * ceil(n_rows / mb)
 * * mb][2]; copo_meta_batch_wgrads_f32 is then phase A of one chunk of minibatches: only the weight-gradient GEMMs,
 * gathering their operands from the row store through the minibatch row tables, the dot products (scaled by
 * 1 / denom^2) and the loss statistics regrouped from rowstat.  Same results as copo_meta_batch_grads_f32.
 * Exported gradients (g_out) carry unit row weights: divide by denom before use. */
int64_t copo_meta_rows_workspace_floats(const copo_ppo_cfg* cfg, int64_t n_rows);
int copo_meta_rows_f32(const copo_ppo_cfg* cfg, float* theta, float* theta_target, const float* obs_src,
                       const float* pack_src, int64_t n_rows, float* rows_ws, float* rowstat, void* stream);
int copo_meta_batch_wgrads_f32(const copo_ppo_cfg* cfg, const float* obs_src, const int64_t* rows, const float* w,
                               const float* denom, const float* rows_ws, int64_t n_rows, const float* rowstat,
                               float* workspace, int32_t nb_cap, int64_t mb_first, int32_t nb, float* g_out,
                               double* gv_out, float* stats_out, void* stream);
/* (ABI 6) stats_out == NULL: the chunk's loss statistics are not regrouped here -- the caller has them from ONE
 * copo_meta_rowstat_f32 launch for all minibatches [mb_first, mb_first + nb) of the pass (they depend on the row tables and the
 * row store only, not on the GEMMs): stats_out [nb][2][8] as copo_meta_batch_wgrads_f32 writes them.  nb <= 65535. */
int copo_meta_rowstat_f32(const copo_ppo_cfg* cfg, const int64_t* rows, const float* w, const float* denom, const float* rowstat,
                          int64_t mb_first, int32_t nb, float* stats_out, void* stream);
/* Phase B: n_mb sequential LCF Adam steps (minibatch order) in one kernel.  Row inputs either gathered from
 * pack_src via rows (ego_nei NULL, n_seg 1) or dense: ego_nei [n_seg][n_mb][mb][2] = {A_ego, A_nei} with w / eps
 * [n_seg][n_mb][mb] (data-parallel: the all-gathered rows of every rank).  gv [n_mb], stats_in [n_mb][2][8] from
 * phase A; lcf_param / adam_state / stats as in copo_meta_finish_f64.
 * n_wg workgroups share the rows of every step (0 = automatic: 1 up to eight segments, where one workgroup is as fast, then
 * one per four segments; <= 16): each adds up
 * its rows, publishes three partial sums in `exchange` (COPO_META_SEQ_XCHG_DOUBLES doubles of device memory, zeroed ONCE by the
 * caller and then left to the kernel) and applies the same Adam step to the sum of all partials -- with N ranks' rows a step
 * then costs what it costs with one.  A workgroup that never arrives (2 s) turns lcf_param into NaN.
 * (ABI 6) k_first / k_count: the launch takes the steps of minibatches [k_first, k_first + k_count) of the n_mb the arrays hold
 * (k_count < 0: all from k_first on) -- a meta pass can run its LCF steps chunk by chunk, behind the dot products of each chunk. */
#define COPO_META_SEQ_XCHG_DOUBLES 256
int copo_meta_batch_lcf_f64(const float* pack_src, int32_t pack_width, int32_t col_adv, int32_t col_nei_adv,
                            const int64_t* rows, const float* ego_nei, int32_t n_seg, const float* w, const double* eps,
                            const float* denom, int32_t mb, int32_t n_mb, const double* gv, const float* stats_in,
                            double* lcf_param, const double* raw_mean_std, double* adam_state, double lr, double* stats,
                            int32_t k_first, int32_t k_count, int32_t n_wg, double* exchange, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Peer all-reduce (replaces the in-process tower averaging of RLlib's multi-GPU learner,
 * algo_copo.py:519-577, for one process per GPU): a two-shot sum over device memory that every rank of the node has mapped.
 *   workspace = copo_peer_alloc(copo_peer_workspace_bytes(n, world))      uncached device memory, zeroed; its first n floats are
 *               the buffer that is reduced in place (the caller writes its gradient sums there)
 *   copo_ipc_export / copo_ipc_open     64-byte handles, exchanged by the host side (torch.distributed all_gather_object)
 *   copo_peer_allreduce_sum_f32(workspaces[world] as mapped in THIS process, n, rank, world, stream)
 *               one kernel: shards scattered to their owners' inboxes, added up in rank order (bit-identical on every rank),
 *               results stored to every rank's buffer; flags in the workspaces order the two hops.  Every rank must call it the
 *               same number of times.  A peer that does not answer within ~2 s raises an error word instead of hanging the GPU:
 *   copo_peer_status(workspace, n, world, stream)    COPO_OK, or COPO_ERR_DEVICE after a timed-out wait
 */
#define COPO_PEER_MAX_WORLD 16
#define COPO_IPC_HANDLE_BYTES 64
int64_t copo_peer_workspace_bytes(int64_t n, int32_t world);
int copo_peer_alloc(int64_t bytes, void** out);
int copo_peer_free(void* workspace);
int copo_ipc_export(void* dev_ptr, unsigned char* handle64);
int copo_ipc_open(const unsigned char* handle64, void** out);
int copo_ipc_close(void* mapped);
int copo_peer_allreduce_sum_f32(void* const* workspaces, int64_t n, int32_t rank, int32_t world, void* stream);
int copo_peer_status(void* workspace, int64_t n, int32_t world, void* stream);
/* test entry: all `world` ranks in one launch (the workspaces all belong to the calling process) */
int copo_debug_peer_allreduce_all_ranks(void* const* workspaces, int64_t n, int32_t world, void* stream);
/* profiling entries (scripts/ only): device-side wall-clock stamps that profiling calls of the fused learner leave behind --
 * 16 phase stamps of one row-pass workgroup / [2][1024][2] start-end stamps per workgroup of the two kernels of a step */
int copo_debug_rowpass_stamps(unsigned long long* out16);
int copo_debug_wg_times(unsigned long long* out4096);
/* test entries: the launch plan of the fused learner -- which kernels a configuration would launch, in order, computed by the code
 * the entry points above launch from.  Pure host code: the device is not touched.
 *   mode   0 PPO step, 1 PPO gradients only, 2 data-parallel step, 3 step-by-step meta pair, 4 the same with the LCF tail,
 *          5 batched meta pass, 6 row store, 7 weight gradients from the row store (5..7: n = minibatches / row blocks of the launch),
 *          8 forward pass (n = rows, nets [first_net, first_net + n_nets), n_members > 0: the bank forward with n rows per member)
 *   head_mode   COPO_HEAD_* of modes 0..2;  world   data-parallel ranks (1: none)
 *   facts  what the caller's pointers are: 1 sources, parameters and workspace 16-byte aligned, 2 transposed mirror given,
 *          4 the mirror (with parameters and workspace) 16-byte aligned, 8 row store aligned with operand slabs below 4 GB
 * out (HOST, cap int32): {launches, fold workgroups, fold length, fold offset low / high word, mirror refresh after the chain,
 * row splits, weight-gradient workgroups}, then per launch {kernel id, grid x, y, z, workgroup size, dynamic LDS bytes}.
 * A configuration the entry points refuse returns their code (COPO_ERR_DEVICE, or COPO_ERR_DIM for a forward shape).
 * copo_debug_learner_kernel: name of a kernel id (NULL beyond the table), its workgroup size and dynamic-LDS ceiling. */
int copo_debug_learner_plan(const copo_ppo_cfg* cfg, int32_t mode, int32_t head_mode, int64_t n, int32_t world, int32_t facts,
                            int32_t first_net, int32_t n_nets, int32_t n_members, int32_t* out, int32_t cap);
const char* copo_debug_learner_kernel(int32_t id, int32_t* block_out, int32_t* lds_cap_out);

#ifdef __cplusplus
}
#endif
#endif /* COPO_HIP_H */
