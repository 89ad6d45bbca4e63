// Fused minibatch learner for the CoPO / CCPPO / IPPO MLPs on gfx950.
//
// The reference runs the PPO minibatch step through torch autograd (algo_copo.py:311-424 `loss`, RLlib
// `train_one_step`, torch.optim.Adam): ~250 tiny kernels per 512-row minibatch, launch-bound on any GPU.
// Everything here works on ONE flat fp32 parameter buffer (+ a mirror with W1 / W2 transposed).
//
// Contents, in file order:
//   1. FusedArgs, group / workspace-layout helpers (WsLay), counter hand-over slots
//   2. tile-GEMM engine (gemm_tile: 64x64 tiles, K slabs through LDS, v_mfma_f32_32x32x2_f32) and its operand functors
//        FwdOpT<1|2>  h = tanh(X W^T + b)            BxOp  dz1 = (dz2 W2) (1 - h1^2)
//        BwOpT<l, GA> partial dW_l = dz^T [In | 1]   (GA: operands gathered from the meta row store)
//      -- the path of shapes without a row-pass instantiation, of the batched meta pass and of the row store
//   3. head_row_terms (PPO / value / meta loss terms + analytic gradient), head_kernel
//   4. rowpass_kernel: layers 1-2, heads, dz2, dz1 of 16 rows in one workgroup (v_mfma_f32_16x16x4_f32, weights
//      streamed through BRing register rings); mlp_fwd_kernel: its forward-only sibling (rollouts, critic heads);
//      learn_seat.inc: the argument head and the tile prologue of the four seat passes below;
//      learn_inputgrad.inc: adv_obs_kernel, the forward plus the backward pass down to the INPUT row of a seated bank (evaluation);
//      learn_pgd.inc: pgd_obs_kernel, that pass iterated in one resident workgroup (projected gradient descent on the input row);
//      learn_certify.inc: cert_obs_kernel, interval bounds of the action means over an L-infinity box of the input row
//      learn_linbound.inc: lin_obs_kernel, linear bounds of the same means (one relaxation per tanh unit, carried backward), intersected with them
//      learn_jury.inc: jury_obs_kernel, the forward of every JUDGE of a row into a plane of its own (a row may stand in many members' lists)
//      learn_attrib.inc: ig_obs_kernel, integrated gradients of both action means down to the input row, all quadrature points in one resident workgroup
//      learn_hidden.inc: hidden_obs_kernel, the jury's forward stopped behind layer 2: both tanh layers of every judge's rows, kept by position
//   5. LCF meta kernels: meta_lcf / meta_finish (step by step), meta_batch_fold / dot / rowstat, meta_seq (all LCF
//      Adam steps of a pass in one workgroup)
//   6. reduce_adam_kernel (fold of row-split partials + Adam; legacy two-net meta step), wgrad_adam_kernel (weight
//      gradients + fold + Adam in one kernel), adam_flat_kernel (after a gradient all-reduce), transposes
//   7. learn_plan.inc, host only: the kernel table (every instantiation of the kernels above that the learner launches: id, name,
//      function, workgroup size, dynamic-LDS ceiling) and the launch plan -- plan_step / plan_forward decide, from the configuration,
//      the caller's mode and a few facts about its pointers, which table entries run with which grid, and the fold geometry
//   8. here: gemm_lds_attrs (the ceilings of the table as attributes), launch_kernel (the one launch, by table id),
//      launch_fused_step (walks a plan) and the C ABI; copo_debug_learner_plan returns a plan without touching the device, and the
//      size queries (exchange workspace, fold length, batched workspace) read their geometry from the same plan
//
// One PPO minibatch step = rowpass_kernel + wgrad_adam_kernel (2 launches).  One LCF meta pass over n_mb minibatches =
// ceil(n_mb / 32) x [gemm_bw_kernel<GA> + fold + rowstat + dot] + meta_seq_kernel, on top of a row store computed once
// per training iteration (F1, F2, head, Bx over all rows).  DESIGN.md section 4 has the measurements.
#include <cstring>
#include <type_traits>

#include "sim_common.h"

#pragma clang fp contract(fast)

namespace copo {
#include "learn_args.inc"
#include "learn_gemm.inc"
#include "learn_rowpass.inc"
#include "learn_seat.inc"
#include "learn_inputgrad.inc"
#include "learn_pgd.inc"
#include "learn_certify.inc"
#include "learn_linbound.inc"
#include "learn_jury.inc"
#include "learn_attrib.inc"
#include "learn_hidden.inc"
#include "learn_meta.inc"
#include "learn_update.inc"
#include "learn_plan.inc"

// ------------------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------------------
// entries above the default limit get their ceiling as an attribute, once per process; a launch beyond an entry's ceiling is refused
// here, not by the runtime
static hipError_t gemm_lds_attrs() {
    static hipError_t once = [] {
        hipError_t e = hipSuccess, r;
        for (const KernelEntry& k : g_kernels)
            if (k.lds_cap > LDS_DEFAULT && (r = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_cap)) != hipSuccess) e = r;
        return e;
    }();
    return once;
}
static hipError_t launch_kernel(const Launch& l, void** args, hipStream_t s) {
    if (l.id < 0 || l.id >= K_COUNT || l.lds > g_kernels[l.id].lds_cap) return hipErrorInvalidValue;
    return hipLaunchKernel(g_kernels[l.id].fn, dim3(l.gx, l.gy, l.gz), dim3(l.block), args, (size_t)l.lds, s);
}

struct MetaTail { MetaArgs lcf; MetaFinishArgs fin; };
// what the fold of a meta mode writes besides the gradients: the batched fold's exports, or the LCF step of PLAN_META_PAIR_TAIL
struct FoldSink { float* g_out; double* dot_out; float* stats_out; const MetaTail* tail; };

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static int facts_of(const FusedArgs& a) {
    const copo_ppo_cfg& c = a.c;
    // the gather-all tiles address the row store with 32-bit byte offsets (buffer loads): every operand slab must stay below 4 GB
    const uint64_t widest = (uint64_t)(c.hidden > c.pol.in_dim ? c.hidden : c.pol.in_dim);
    return (aligned16(a.obs_src) && aligned16(a.cc_src) && aligned16(a.theta) && aligned16(a.ws) && aligned16(a.theta2) ? FACT_ALIGNED : 0) |
           (a.theta_t ? FACT_MIRROR : 0) | (aligned16(a.theta) && aligned16(a.theta_t) && aligned16(a.ws) ? FACT_MIRROR_ALIGNED : 0) |
           (aligned16(a.ws0) && (uint64_t)a.gcap0 * (uint64_t)c.mb * widest * 4u < 0xfffffff0ull ? FACT_STORE_OK : 0);
}

// walks the plan of `mode` for these arguments; plan_out: the plan it walked (its fold geometry, for the kernels a caller adds)
hipError_t launch_fused_step(FusedArgs a, PlanMode mode, int nb, hipStream_t s, FoldSink sink = {}, Plan* plan_out = nullptr) {
    if (hipError_t e = gemm_lds_attrs(); e != hipSuccess) return e;
    const Plan p = plan_step(a.c, mode, a.head_mode, nb, a.dp_world, facts_of(a), switches());
    if (p.refused) return hipErrorInvalidValue;
    if (plan_out) *plan_out = p;
    a.groups = p.groups;
    a.ksplit = p.ksplit;
    a.dbg = profile_dbg_bits();
    a.stat_tiles = p.stat_tiles;
    MetaTail tail{};
    if (sink.tail) {
        tail = *sink.tail;
        tail.fin.n_partials = p.fold_blocks;      // only the partials this launch writes
    }
    int64_t lo = p.lo;
    int n_fold = p.n_fold, meta_tail = sink.tail ? 1 : 0;
    for (int i = 0; i < p.n; ++i) {
        Launch l = p.l[i];
        void* step_args[] = {&a, &l.arg[0], &l.arg[1], &l.arg[2], &l.arg[3]};
        void* batch_fold_args[] = {&a, &lo, &n_fold, &sink.g_out, &sink.dot_out, &sink.stats_out};
        void* fold_args[] = {&a, &lo, &n_fold, &meta_tail, &tail.lcf, &tail.fin};
        if (hipError_t e = launch_kernel(l, l.id == K_META_FOLD ? batch_fold_args : l.id == K_REDUCE_ADAM ? fold_args : step_args, s); e != hipSuccess)
            return e;
    }
    // the next row pass would read stale weights otherwise (the fused weight-gradient kernel keeps the mirror itself)
    if (p.refresh_mirror) return launch_refresh_transposed(a.c, a.theta, a.theta_t, s);
    return hipGetLastError();
}

hipError_t launch_adam_flat(const FusedArgs& a, long long n, hipStream_t s) {
    const int slots = a.ws != nullptr;
    const int n_tiles = a.theta_t ? adam_tile_count(a.c) : 0;
    hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)(n_tiles + (n + 256 * ADAM_EPT - 1) / (256 * ADAM_EPT))), dim3(256), 0, s, a, n, slots, n_tiles);
    if (!slots)
        hipLaunchKernelGGL(bump_kernel, dim3(1), dim3(1), 0, s, const_cast<int64_t*>(a.step),
                           a.bump_k ? const_cast<int64_t*>(a.kptr) : nullptr);
    return hipGetLastError();
}

}  // namespace copo

// ---- C ABI ---------------------------------------------------------------------------------------------------
using namespace copo;

extern "C" int copo_debug_rowpass_stamps(unsigned long long* out16) {
    return hipMemcpyFromSymbol(out16, HIP_SYMBOL(copo::g_rp_stamps), 16 * sizeof(unsigned long long)) == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

extern "C" int copo_debug_wg_times(unsigned long long* out4096) {
    return hipMemcpyFromSymbol(out4096, HIP_SYMBOL(copo::g_wg_times), 4096 * sizeof(unsigned long long)) == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

extern "C" int64_t copo_ppo_workspace_floats(const copo_ppo_cfg* cfg) { return cfg ? (int64_t)fused_ws_floats(*cfg) : -1; }

static int check_cfg(const copo_ppo_cfg* c) {
    if (!c) return COPO_ERR_NULL;
    if (c->mb < 1 || c->mb > COPO_PPO_MAX_MB || c->hidden < 1 || c->hidden > 1024 || c->act_dim != 2 ||
        c->n_value_heads < 0 || c->n_value_heads > 3 || c->n_params < 1)
        return COPO_ERR_DIM;
    if (c->pol.out_dim != 4) return COPO_ERR_DIM;
    if (c->operand_dtype != COPO_OPERAND_F32 && c->operand_dtype != COPO_OPERAND_BF16) return COPO_ERR_DIM;
    for (int g = 0; g < c->n_value_heads; ++g)
        if (c->val[g].out_dim != 1) return COPO_ERR_DIM;
    return COPO_OK;
}

static void fill_common(FusedArgs& a, const copo_ppo_cfg* cfg, const float* obs_src, const float* cc_src,
                        const float* pack_src, const int64_t* rows, const float* w, const float* denom, float* workspace,
                        int64_t* mb_index) {
    memset(&a, 0, sizeof(a));
    a.c = *cfg;
    a.obs_src = obs_src; a.cc_src = cc_src ? cc_src : obs_src; a.pack_src = pack_src;
    a.rows = rows; a.w = w; a.denom = denom; a.ws = workspace; a.kptr = mb_index;
    a.gcap = 4; a.nreg = 2;
}

extern "C" int copo_ppo_fused_step_f32(const copo_ppo_cfg* cfg, float* theta, float* adam_m, float* adam_v, float* grad,
                                       const float* obs_src, const float* cc_src, const float* pack_src,
                                       const int64_t* rows, const float* w, const float* denom, const float* kl_coeff,
                                       int64_t* step, float* workspace, float* stats, int32_t apply_adam,
                                       int32_t head_mode, int64_t* mb_index, int32_t bump_index, float* theta_t,
                                       void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!theta || !obs_src || !pack_src || !w || !denom || !workspace) return COPO_ERR_NULL;
    if (!rows && head_mode != COPO_HEAD_PPO) return COPO_ERR_NULL;       // (sources in minibatch order: the PPO step only)
    if (apply_adam && (!adam_m || !adam_v || !step)) return COPO_ERR_NULL;
    if (!apply_adam && !grad) return COPO_ERR_NULL;
    if (head_mode < COPO_HEAD_PPO || head_mode > COPO_HEAD_META_OLD) return COPO_ERR_DIM;
    if (head_mode == COPO_HEAD_PPO && cfg->use_kl && !kl_coeff) return COPO_ERR_NULL;
    FusedArgs a;
    fill_common(a, cfg, obs_src, cc_src, pack_src, rows, w, denom, workspace, mb_index);
    a.theta = theta; a.adam_m = adam_m; a.adam_v = adam_v; a.grad = grad;
    a.kl_coeff = kl_coeff; a.step = step; a.stats = stats; a.apply_adam = apply_adam; a.head_mode = head_mode;
    a.bump_k = (mb_index && bump_index) ? 1 : 0;
    a.theta_t = theta_t;
    hipError_t e = launch_fused_step(a, apply_adam ? PLAN_PPO_STEP : PLAN_PPO_GRADS, 0, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

// workgroups of the weight-gradient kernel of a PPO step over all nets of `c`: the tiles of the data-parallel exchange
static int wgrad_tiles(const copo_ppo_cfg& c) {
    return plan_step(c, PLAN_DP_STEP, COPO_HEAD_PPO, 0, 1, FACT_ALIGNED | FACT_MIRROR | FACT_MIRROR_ALIGNED, switches()).wgrad_tiles;
}

extern "C" int64_t copo_dp_workspace_bytes(const copo_ppo_cfg* cfg, int32_t world) {
    if (check_cfg(cfg) != COPO_OK || world < 1 || world > COPO_PEER_MAX_WORLD) return -1;
    return (int64_t)(DpLay(wgrad_tiles(*cfg), world).words() * sizeof(float));
}

extern "C" int copo_ppo_fused_step_dp_f32(const copo_ppo_cfg* cfg, float* theta, float* adam_m, float* adam_v,
                                          const float* obs_src, const float* cc_src, const float* pack_src,
                                          const int64_t* rows, const float* w, const float* denom, const float* kl_coeff,
                                          int64_t* step, float* workspace, float* stats, int64_t* mb_index, int32_t bump_index,
                                          float* theta_t, void* const* dp_workspaces, int32_t rank, int32_t world, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!theta || !obs_src || !pack_src || !w || !denom || !workspace || !adam_m || !adam_v || !step) return COPO_ERR_NULL;
    if (cfg->use_kl && !kl_coeff) return COPO_ERR_NULL;
    if (world < 1 || world > COPO_PEER_MAX_WORLD || rank < 0 || rank >= world) return COPO_ERR_DIM;
    if (world > 1 && !dp_workspaces) return COPO_ERR_NULL;
    FusedArgs a;
    fill_common(a, cfg, obs_src, cc_src, pack_src, rows, w, denom, workspace, mb_index);
    a.theta = theta; a.adam_m = adam_m; a.adam_v = adam_v;
    a.kl_coeff = kl_coeff; a.step = step; a.stats = stats; a.apply_adam = 1; a.head_mode = COPO_HEAD_PPO;
    a.bump_k = (mb_index && bump_index) ? 1 : 0;
    a.theta_t = theta_t;
    a.dp_rank = rank; a.dp_world = world;
    for (int r = 0; r < world && world > 1; ++r) {
        if (!dp_workspaces[r]) return COPO_ERR_NULL;
        a.dp_ws[r] = static_cast<float*>(dp_workspaces[r]);
    }
    hipError_t e = launch_fused_step(a, PLAN_DP_STEP, 0, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

// error word of this rank's exchange workspace (0 = every wait so far was answered); synchronises the stream first
extern "C" int copo_dp_status(void* workspace, const copo_ppo_cfg* cfg, int32_t world, void* stream) {
    if (!workspace || check_cfg(cfg) != COPO_OK || world < 1 || world > COPO_PEER_MAX_WORLD) return COPO_ERR_NULL;
    uint32_t ctl[8];
    if (hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) return COPO_ERR_DEVICE;
    if (hipMemcpy(ctl, static_cast<float*>(workspace) + DpLay(wgrad_tiles(*cfg), world).control(), sizeof(ctl), hipMemcpyDeviceToHost) != hipSuccess)
        return COPO_ERR_DEVICE;
    return ctl[0] ? COPO_ERR_DEVICE : COPO_OK;
}

static int mlp_forward(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, const float* obs_src,
                       const float* cc_src, int64_t n_rows, int32_t first_net, int32_t n_nets, float* values,
                       float* dist_inputs, const float* eps, float* action, float* logp, float* clipped,
                       const int64_t* rows, int64_t n_out, void* stream, int32_t n_members = 0, int64_t member_stride = 0,
                       const int32_t* counts = nullptr) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!theta || !theta_t || !obs_src) return COPO_ERR_NULL;
    if (rows && n_out < 1) return COPO_ERR_DIM;
    if (n_rows < 1 || first_net < 0 || n_nets < 1 || first_net + n_nets > 1 + cfg->n_value_heads) return COPO_ERR_DIM;
    const bool bank = n_members > 0, seats = counts != nullptr;      // seat mode: the bank with a row list per member (n_rows = cap)
    if (bank && (first_net != 0 || n_nets != 1 || (rows != nullptr) != seats || n_members > 65535 || member_stride < cfg->n_params ||
                 member_stride % 4 != 0))
        return COPO_ERR_DIM;
    if (seats && !bank) return COPO_ERR_DIM;
    if (first_net + n_nets > 1 && !values) return COPO_ERR_NULL;
    if (first_net == 0 && eps && (!action || !logp)) return COPO_ERR_NULL;
    Launch l;
    rc = plan_forward(*cfg, n_rows, first_net, n_nets, n_members, (aligned16(theta_t) ? FACT_MIRROR_ALIGNED : 0) | (seats ? FACT_SEATS : 0), &l);
    if (rc != COPO_OK) return rc;
    if (gemm_lds_attrs() != hipSuccess) return COPO_ERR_DEVICE;
    FwdBankArgs a;      // (the single-member kernels take its FwdArgs base)
    static_cast<FwdArgs&>(a) = FwdArgs{*cfg, theta, theta_t, obs_src, cc_src ? cc_src : obs_src, n_rows, first_net, n_nets, values, dist_inputs, eps,
                                       action, logp, clipped, rows, rows ? n_out : n_rows};
    a.member_stride = member_stride;
    a.counts = counts;
    void* args[] = {static_cast<FwdArgs*>(&a)};
    return launch_kernel(l, args, static_cast<hipStream_t>(stream)) == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

// ---- plan query (tests): what a configuration would launch; the device is not touched ---------------------------------
extern "C" const char* copo_debug_learner_kernel(int32_t id, int32_t* block_out, int32_t* lds_cap_out) {
    if (id < 0 || id >= K_LEARNER_COUNT) return nullptr;
    if (block_out) *block_out = g_kernels[id].block;
    if (lds_cap_out) *lds_cap_out = g_kernels[id].lds_cap;
    return g_kernels[id].name;
}

extern "C" int copo_debug_learner_plan(const copo_ppo_cfg* cfg, int32_t mode, int32_t head_mode, int64_t n, int32_t world, int32_t facts,
                                       int32_t first_net, int32_t n_nets, int32_t n_members, int32_t* out, int32_t cap) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!out) return COPO_ERR_NULL;
    if (mode < 0 || mode > PLAN_FORWARD || head_mode < COPO_HEAD_PPO || head_mode > COPO_HEAD_META_OLD || world < 1 || world > COPO_PEER_MAX_WORLD ||
        n_members < 0 || n_members > 65535 || (mode >= PLAN_META_BATCH && mode < PLAN_FORWARD && (n < 1 || 2 * n > 65535)))
        return COPO_ERR_DIM;
    Plan p{};
    if (mode == PLAN_FORWARD) {
        if ((rc = plan_forward(*cfg, n, first_net, n_nets, n_members, facts, &p.l[0])) != COPO_OK) return rc;
        p.n = 1;
    } else {
        p = plan_step(*cfg, (PlanMode)mode, head_mode, (int)n, world, facts, switches());
        if (p.refused) return COPO_ERR_DEVICE;      // (what the entry points answer)
    }
    if (cap < 8 + 6 * p.n) return COPO_ERR_DIM;
    const int32_t head[8] = {p.n, p.fold_blocks, p.n_fold, (int32_t)(p.lo & 0xffffffff), (int32_t)(p.lo >> 32), p.refresh_mirror, p.ksplit, p.wgrad_tiles};
    memcpy(out, head, sizeof(head));
    for (int i = 0; i < p.n; ++i) memcpy(out + 8 + 6 * i, &p.l[i], 6 * sizeof(int32_t));      // id, grid x / y / z, block, LDS bytes
    return COPO_OK;
}

extern "C" int copo_mlp_forward_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, const float* obs_src,
                                    const float* cc_src, int64_t n_rows, int32_t first_net, int32_t n_nets, float* values,
                                    float* dist_inputs, const float* eps, float* action, float* logp, float* clipped,
                                    void* stream) {
    return mlp_forward(cfg, theta, theta_t, obs_src, cc_src, n_rows, first_net, n_nets, values, dist_inputs, eps, action, logp,
                       clipped, nullptr, n_rows, stream);
}

extern "C" int copo_mlp_forward_bank_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                                         int32_t n_members, int64_t rows_per_member, const float* obs_src, float* dist_inputs,
                                         const float* eps, float* action, float* logp, float* clipped, void* stream) {
    if (n_members < 1) return COPO_ERR_DIM;
    return mlp_forward(cfg, theta, theta_t, obs_src, nullptr, rows_per_member, 0, 1, nullptr, dist_inputs, eps, action, logp, clipped,
                       nullptr, rows_per_member, stream, n_members, member_stride);
}

extern "C" int copo_mlp_forward_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                                          int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                                          const float* obs_src, float* dist_inputs, const float* eps, float* action, float* logp,
                                          float* clipped, void* stream) {
    if (!rows || !counts) return COPO_ERR_NULL;
    if (n_members < 1 || cap < 1 || n_out < 1) return COPO_ERR_DIM;
    return mlp_forward(cfg, theta, theta_t, obs_src, nullptr, cap, 0, 1, nullptr, dist_inputs, eps, action, logp, clipped, rows, n_out,
                       stream, n_members, member_stride, counts);
}

// The one launch path of the four seat passes.  `h`: the head of the pass's argument struct, filled by the entry point but for the
// configuration, which is copied in here once it is known to be there; `out`: the pass's required output; `own_ok`: the entry point's own
// dimension checks (pad, max_iters); first_id / lds_floats / lds_cap: plan_seat_pass; `args`: the struct `h` is the head of.
static int seat_pass_launch(const copo_ppo_cfg* cfg, SeatHead& h, const void* out, bool own_ok, int first_id, size_t (*lds_floats)(int, int),
                            int lds_cap, void* args, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!h.theta || !h.theta_t || !h.rows || !h.counts || !h.obs_src || !out || !h.group || !h.level_of || !h.levels) return COPO_ERR_NULL;
    if (h.n_out < 1 || h.n_slots < 1 || h.n_out % h.n_slots != 0 || h.n_groups < 1 || h.n_levels < 1 || h.member_stride < cfg->n_params ||
        h.member_stride % 4 != 0 || h.col_lo < 0 || h.col_lo > h.col_hi || h.col_hi > cfg->pol.in_dim || !own_ok)
        return COPO_ERR_DIM;
    Launch l;
    rc = plan_seat_pass(*cfg, h.cap, h.n_members, aligned16(h.theta_t) ? FACT_MIRROR_ALIGNED : 0, first_id,
                        lds_floats(cfg->hidden, rowpass_k1p(cfg->pol.in_dim)), lds_cap, &l);
    if (rc != COPO_OK) return rc;
    if (gemm_lds_attrs() != hipSuccess) return COPO_ERR_DEVICE;
    h.c = *cfg;
    return launch_kernel(l, &args, static_cast<hipStream_t>(stream)) == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}
// the head of a seat pass from the leading arguments of its entry point
#define COPO_SEAT_HEAD                                                                                                          \
    SeatHead { {}, theta, theta_t, member_stride, rows, counts, cap, n_out, obs_src, col_lo, col_hi, n_slots, group, n_groups, level_of, \
               reinterpret_cast<const float*>(levels), n_levels, n_members }

extern "C" int copo_adv_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                                      int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                                      const float* obs_src, float* obs_seen, float* grad, int32_t col_lo, int32_t col_hi, int32_t n_slots,
                                      const int32_t* group, int32_t n_groups, const int32_t* level_of, const float* levels,
                                      int32_t n_levels, void* stream) {
    AdvArgs a{COPO_SEAT_HEAD, obs_seen, grad};
    return seat_pass_launch(cfg, a.h, obs_seen, true, K_ADV_1_4, adv_lds_floats, LDS_ROWPASS, &a, stream);
}

extern "C" int copo_pgd_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                                      int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                                      const float* obs_src, float* obs_seen, int32_t col_lo, int32_t col_hi, int32_t n_slots,
                                      const int32_t* group, int32_t n_groups, const int32_t* level_of, const uint32_t* levels,
                                      int32_t n_levels, uint64_t seed, int32_t* tick, int32_t max_iters, float* trace, void* stream) {
    PgdArgs a{COPO_SEAT_HEAD, obs_seen, trace, seed, tick, max_iters};
    return seat_pass_launch(cfg, a.h, obs_seen, max_iters >= 1 && max_iters <= PGD_MAX_ITERS, K_PGD_1_4, pgd_lds_floats, LDS_ROWPASS, &a, stream);
}

static bool pad_ok(float pad) { return pad >= 0.0f && __builtin_isfinite(pad); }

extern "C" int copo_cert_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                                       int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                                       const float* obs_src, float* bounds, int32_t col_lo, int32_t col_hi, int32_t n_slots,
                                       const int32_t* group, int32_t n_groups, const int32_t* level_of, const float* levels,
                                       int32_t n_levels, float pad, void* stream) {
    CertArgs a{COPO_SEAT_HEAD, bounds, pad};
    return seat_pass_launch(cfg, a.h, bounds, pad_ok(pad), K_CERT_1_4, cert_lds_floats, LDS_ROWPASS, &a, stream);
}

extern "C" int copo_lin_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                                      int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                                      const float* obs_src, float* bounds, float* parts, int32_t col_lo, int32_t col_hi, int32_t n_slots,
                                      const int32_t* group, int32_t n_groups, const int32_t* level_of, const float* levels,
                                      int32_t n_levels, float pad, void* stream) {
    LinArgs a{COPO_SEAT_HEAD, bounds, parts, pad};
    return seat_pass_launch(cfg, a.h, bounds, pad_ok(pad), K_LIN_1_4, lin_lds_floats, LDS_LINBOUND, &a, stream);
}

extern "C" int copo_ig_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                                     int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                                     const float* obs_src, float* attr, float* heads, int32_t col_lo, int32_t col_hi, int32_t n_slots,
                                     const int32_t* group, int32_t n_groups, const int32_t* level_of, const int32_t* levels,
                                     int32_t n_levels, const float* base, int32_t max_points, void* stream) {
    if (!heads || !base) return COPO_ERR_NULL;
    IgArgs a{COPO_SEAT_HEAD, attr, heads, base, max_points};
    return seat_pass_launch(cfg, a.h, attr, max_points >= 1 && max_points <= IG_MAX_POINTS, K_IG_1_4, ig_lds_floats, LDS_ROWPASS, &a, stream);
}

// The jury pass: seat mode's launch shape with a list per JUDGE; none of the level tables of the four passes above, so its checks are its own.
extern "C" int copo_jury_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                                       int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                                       const float* obs_src, float* verdict, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!theta || !theta_t || !rows || !counts || !obs_src || !verdict) return COPO_ERR_NULL;
    if (cap < 1 || n_out < 1 || n_members < 1 || n_members > 65535 || member_stride < cfg->n_params || member_stride % 4 != 0) return COPO_ERR_DIM;
    Launch l;      // (plan_seat_pass refuses the bfloat16 operand mode, as it does for the adversary pass)
    rc = plan_seat_pass(*cfg, cap, n_members, aligned16(theta_t) ? FACT_MIRROR_ALIGNED : 0, K_JURY_1_4,
                        jury_lds_floats(cfg->hidden, rowpass_k1p(cfg->pol.in_dim)), LDS_ROWPASS, &l);
    if (rc != COPO_OK) return rc;
    if (gemm_lds_attrs() != hipSuccess) return COPO_ERR_DEVICE;
    JuryArgs a{SeatHead{*cfg, theta, theta_t, member_stride, rows, counts, cap, n_out, obs_src, 0, 0, 1, nullptr, 0, nullptr, nullptr, 0, n_members},
               verdict};
    void* args[] = {&a};
    return launch_kernel(l, args, static_cast<hipStream_t>(stream)) == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

// The hidden-layer pass: the jury's launch shape and checks; the output is indexed by position in a judge's list, not by row.
extern "C" int copo_hidden_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                                         int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                                         const float* obs_src, float* hidden, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!theta || !theta_t || !rows || !counts || !obs_src || !hidden) return COPO_ERR_NULL;
    if (cap < 1 || n_out < 1 || n_members < 1 || n_members > 65535 || member_stride < cfg->n_params || member_stride % 4 != 0 || !aligned16(hidden))
        return COPO_ERR_DIM;
    Launch l;
    rc = plan_seat_pass(*cfg, cap, n_members, aligned16(theta_t) ? FACT_MIRROR_ALIGNED : 0, K_HIDDEN_1_4,
                        hidden_lds_floats(cfg->hidden, rowpass_k1p(cfg->pol.in_dim)), LDS_ROWPASS, &l);
    if (rc != COPO_OK) return rc;
    if (gemm_lds_attrs() != hipSuccess) return COPO_ERR_DEVICE;
    HiddenArgs a{SeatHead{*cfg, theta, theta_t, member_stride, rows, counts, cap, n_out, obs_src, 0, 0, 1, nullptr, 0, nullptr, nullptr, 0, n_members},
                 hidden};
    void* args[] = {&a};
    return launch_kernel(l, args, static_cast<hipStream_t>(stream)) == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

extern "C" int copo_mlp_forward_rows_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t,
                                         const float* obs_src, const float* cc_src, const int64_t* rows, int64_t n_rows,
                                         int64_t n_src_rows, int32_t first_net, int32_t n_nets, float* values, void* stream) {
    if (!rows) return COPO_ERR_NULL;
    return mlp_forward(cfg, theta, theta_t, obs_src, cc_src, n_rows, first_net, n_nets, values, nullptr, nullptr, nullptr, nullptr,
                       nullptr, rows, n_src_rows, stream);
}

extern "C" int copo_transpose_weights_f32(const copo_ppo_cfg* cfg, const float* theta, float* theta_t, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!theta || !theta_t) return COPO_ERR_NULL;
    return launch_refresh_transposed(*cfg, theta, theta_t, static_cast<hipStream_t>(stream)) == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

// the meta modes: both policies of the LCF meta update on the policy net
static void fill_meta(FusedArgs& a, const copo_ppo_cfg* cfg, float* theta, float* theta_target, const float* obs_src, const float* pack_src,
                      const int64_t* rows, const float* w, const float* denom, float* workspace, int64_t* mb_index) {
    fill_common(a, cfg, obs_src, nullptr, pack_src, rows, w, denom, workspace, mb_index);
    a.theta = theta; a.theta2 = theta_target; a.apply_adam = 0; a.head_mode = MODE_META_BOTH;
}
static void fill_meta_pair(FusedArgs& a, float* g_new, float* g_old, float* stats_new, float* stats_old, double* dot_partials) {
    a.grad = g_new; a.grad2 = g_old; a.stats = stats_new; a.stats2 = stats_old; a.dot_partials = dot_partials;
}

extern "C" int copo_meta_grads_f32(const copo_ppo_cfg* cfg, float* theta, float* theta_target, float* g_new, float* g_old,
                                   const float* obs_src, const float* pack_src, const int64_t* rows, const float* w,
                                   const float* denom, float* workspace, float* stats_new, float* stats_old,
                                   double* dot_partials, int64_t* mb_index, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!theta || !theta_target || !g_new || !g_old || !obs_src || !pack_src || !rows || !w || !denom || !workspace ||
        !dot_partials)
        return COPO_ERR_NULL;
    FusedArgs a;
    fill_meta(a, cfg, theta, theta_target, obs_src, pack_src, rows, w, denom, workspace, mb_index);
    fill_meta_pair(a, g_new, g_old, stats_new, stats_old, dot_partials);
    hipError_t e = launch_fused_step(a, PLAN_META_PAIR, 0, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

extern "C" int copo_meta_step_f64(const copo_ppo_cfg* cfg, float* theta, float* theta_target, float* g_new, float* g_old,
                                  const float* obs_src, const float* pack_src, const int64_t* rows, const float* w,
                                  const float* denom, float* workspace, float* stats_new, float* stats_old,
                                  double* dot_partials, int32_t col_adv, int32_t col_nei_adv, const double* eps,
                                  double* lcf_param, const double* raw_mean_std, double* tail, double* adam_state,
                                  double lr, double* stats, int64_t* mb_index, int32_t bump_index, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!theta || !theta_target || !g_new || !g_old || !obs_src || !pack_src || !rows || !w || !denom || !workspace ||
        !dot_partials || !eps || !lcf_param || !raw_mean_std || !tail || !adam_state)
        return COPO_ERR_NULL;
    FusedArgs a;
    fill_meta(a, cfg, theta, theta_target, obs_src, pack_src, rows, w, denom, workspace, mb_index);
    fill_meta_pair(a, g_new, g_old, stats_new, stats_old, dot_partials);
    MetaTail mt;
    mt.lcf = MetaArgs{pack_src, rows, w, denom, eps, mb_index, cfg->mb, cfg->pack_width, col_adv, col_nei_adv, lcf_param,
                      raw_mean_std, tail};
    mt.fin = MetaFinishArgs{g_new, g_old, 0, dot_partials, COPO_META_DOT_PARTIALS, tail, lcf_param, adam_state, lr, stats_new,
                            stats_old, stats, mb_index, (mb_index && bump_index) ? 1 : 0};
    hipError_t e = launch_fused_step(a, PLAN_META_PAIR_TAIL, 0, static_cast<hipStream_t>(stream), FoldSink{nullptr, nullptr, nullptr, &mt});
    return e == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

// ---- batched LCF meta pass --------------------------------------------------------------------------------------
static size_t batch_ws_base(const copo_ppo_cfg& c, int nb) {     // floats before the fp64 dot-partial scratch (kept even)
    const size_t t = WsLay(c, batch_gcap(nb), batch_gcap(nb)).total();
    return (t + 1) & ~(size_t)1;
}
// the fold geometry of the batched pass (it does not depend on nb or on the pointers)
static Plan batch_fold_plan(const copo_ppo_cfg& c) {
    return plan_step(c, PLAN_META_BATCH, COPO_HEAD_PPO, 1, 1, FACT_ALIGNED | FACT_STORE_OK, switches());
}
// a chunk of a batched pass: the layout is fixed by nb_cap, so that a short last chunk reuses the same (zero-padded) regions;
// returns the fp64 dot-partial scratch behind it
static double* fill_meta_batch(FusedArgs& a, int nb_cap, int64_t mb_first) {
    a.gcap = a.nreg = batch_gcap(nb_cap);
    a.k_first = mb_first;
    return reinterpret_cast<double*>(a.ws + batch_ws_base(a.c, nb_cap));
}

extern "C" int64_t copo_meta_fold_len(const copo_ppo_cfg* cfg) { return cfg ? batch_fold_plan(*cfg).n_fold : -1; }

extern "C" int64_t copo_meta_batch_workspace_floats(const copo_ppo_cfg* cfg, int32_t nb) {
    if (!cfg || nb < 1) return -1;
    return (int64_t)(batch_ws_base(*cfg, nb) + (size_t)2 * nb * batch_fold_plan(*cfg).fold_blocks);
}

extern "C" int copo_meta_batch_grads_f32(const copo_ppo_cfg* cfg, float* theta, float* theta_target, const float* obs_src,
                                         const float* pack_src, const int64_t* rows, const float* w, const float* denom,
                                         float* workspace, int32_t nb_cap, int64_t mb_first, int32_t nb, float* g_out,
                                         double* gv_out, float* stats_out, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!theta || !theta_target || !obs_src || !pack_src || !rows || !w || !denom || !workspace || !gv_out || !stats_out)
        return COPO_ERR_NULL;
    if (nb < 1 || nb > nb_cap || nb_cap > COPO_META_BATCH_MAX || mb_first < 0) return COPO_ERR_DIM;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return COPO_ERR_DIM;
    FusedArgs a;
    fill_meta(a, cfg, theta, theta_target, obs_src, pack_src, rows, w, denom, workspace, nullptr);
    double* dot = fill_meta_batch(a, nb_cap, mb_first);
    Plan p;
    hipError_t e = launch_fused_step(a, PLAN_META_BATCH, nb, static_cast<hipStream_t>(stream), FoldSink{g_out, dot, stats_out, nullptr}, &p);
    if (e != hipSuccess) return COPO_ERR_DEVICE;
    hipLaunchKernelGGL(meta_batch_dot_kernel, dim3(nb), dim3(256), 0, static_cast<hipStream_t>(stream), dot, nullptr,
                       (int64_t)p.fold_blocks, gv_out);
    return hipGetLastError() == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

// ---- meta row store: row-local quantities once per training iteration, regrouped by every meta pass ---------------
static int rows_blocks(const copo_ppo_cfg& c, int64_t n_rows) { return (int)((n_rows + c.mb - 1) / c.mb); }
static int rows_gcap(const copo_ppo_cfg& c, int64_t n_rows) { return batch_gcap(rows_blocks(c, n_rows)); }

extern "C" int64_t copo_meta_rows_workspace_floats(const copo_ppo_cfg* cfg, int64_t n_rows) {
    if (!cfg || n_rows < 1) return -1;
    return (int64_t)WsLay(*cfg, rows_gcap(*cfg, n_rows), 0).total();      // activation slabs only: no gradient regions
}

extern "C" int copo_meta_rows_f32(const copo_ppo_cfg* cfg, float* theta, float* theta_target, const float* obs_src,
                                  const float* pack_src, int64_t n_rows, float* rows_ws, float* rowstat, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!theta || !theta_target || !obs_src || !pack_src || !rows_ws || !rowstat) return COPO_ERR_NULL;
    if (n_rows < 1 || 2 * rows_blocks(*cfg, n_rows) > 65535) return COPO_ERR_DIM;
    FusedArgs a;
    fill_meta(a, cfg, theta, theta_target, obs_src, pack_src, nullptr, nullptr, nullptr, rows_ws, nullptr);
    a.gcap = rows_gcap(*cfg, n_rows);
    a.nreg = 0;
    a.identity_rows = n_rows;
    a.rowstat = rowstat;
    hipError_t e = launch_fused_step(a, PLAN_ROW_STORE, rows_blocks(*cfg, n_rows), static_cast<hipStream_t>(stream));
    return e == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

extern "C" int copo_meta_batch_wgrads_f32(const copo_ppo_cfg* cfg, const float* obs_src, const int64_t* rows, const float* w,
                                          const float* denom, const float* rows_ws, int64_t n_rows, const float* rowstat,
                                          float* workspace, int32_t nb_cap, int64_t mb_first, int32_t nb, float* g_out,
                                          double* gv_out, float* stats_out, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!obs_src || !rows || !w || !denom || !rows_ws || !rowstat || !workspace || !gv_out) return COPO_ERR_NULL;      // (stats_out may be NULL: copo_meta_rowstat_f32)
    if (nb < 1 || nb > nb_cap || nb_cap > COPO_META_BATCH_MAX || mb_first < 0 || n_rows < 1) return COPO_ERR_DIM;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return COPO_ERR_DIM;
    FusedArgs a;
    fill_meta(a, cfg, nullptr, nullptr, obs_src, nullptr, rows, w, denom, workspace, nullptr);
    double* dot = fill_meta_batch(a, nb_cap, mb_first);
    a.ws0 = rows_ws;
    a.gcap0 = rows_gcap(*cfg, n_rows);
    a.rowstat = const_cast<float*>(rowstat);
    Plan p;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = launch_fused_step(a, PLAN_ROW_WGRADS, nb, st, FoldSink{g_out, dot, nullptr, nullptr}, &p);
    if (e != hipSuccess) return COPO_ERR_DEVICE;
    if (stats_out) hipLaunchKernelGGL(meta_rowstat_kernel, dim3(nb), dim3(256), 0, st, a, mb_first, denom, stats_out);
    hipLaunchKernelGGL(meta_batch_dot_kernel, dim3(nb), dim3(256), 0, st, dot, nullptr, (int64_t)p.fold_blocks, gv_out, denom + mb_first);
    return hipGetLastError() == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

extern "C" int copo_meta_rowstat_f32(const copo_ppo_cfg* cfg, const int64_t* rows, const float* w, const float* denom,
                                     const float* rowstat, int64_t mb_first, int32_t nb, float* stats_out, void* stream) {
    int rc = check_cfg(cfg);
    if (rc != COPO_OK) return rc;
    if (!rows || !w || !denom || !rowstat || !stats_out) return COPO_ERR_NULL;
    if (nb < 1 || nb > 65535 || mb_first < 0) return COPO_ERR_DIM;
    FusedArgs a;
    fill_common(a, cfg, nullptr, nullptr, nullptr, rows, w, denom, nullptr, nullptr);
    a.rowstat = const_cast<float*>(rowstat);
    hipLaunchKernelGGL(meta_rowstat_kernel, dim3(nb), dim3(256), 0, static_cast<hipStream_t>(stream), a, mb_first, denom, stats_out);
    return hipGetLastError() == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

extern "C" int copo_meta_batch_dot_f64(const float* g, int64_t n, int32_t nb, double* gv_out, const float* denom, double* partials,
                                       void* stream) {
    if (!g || !gv_out) return COPO_ERR_NULL;
    if (n < 1 || nb < 1) return COPO_ERR_DIM;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (partials && nb <= 65535) {      // grid (nb, COPO_META_DOT_SPLIT) fills the chip; the partials meet in the caller's buffer
        hipLaunchKernelGGL(meta_batch_dot_part_kernel, dim3(nb, DOT_SPLIT), dim3(512), 0, st, g, n, partials);
        hipLaunchKernelGGL(meta_batch_dot_fin_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, nb, gv_out, denom, partials);
    } else {
        hipLaunchKernelGGL(meta_batch_dot_kernel, dim3(nb), dim3(1024), 0, st, nullptr, g, n, gv_out, denom);
    }
    return hipGetLastError() == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

extern "C" int copo_meta_batch_lcf_f64(const float* pack_src, int32_t pack_width, int32_t col_adv, int32_t col_nei_adv,
                                       const int64_t* rows, const float* ego_nei, int32_t n_seg, const float* w,
                                       const double* eps, const float* denom, int32_t mb, int32_t n_mb, const double* gv,
                                       const float* stats_in, double* lcf_param, const double* raw_mean_std,
                                       double* adam_state, double lr, double* stats, int32_t k_first, int32_t k_count,
                                       int32_t n_wg, double* exchange, void* stream) {
    if (!w || !eps || !denom || !gv || !stats_in || !lcf_param || !raw_mean_std || !adam_state) return COPO_ERR_NULL;
    if (!ego_nei && (!pack_src || !rows)) return COPO_ERR_NULL;
    if (mb < 1 || n_mb < 0 || n_mb > 65534 || n_seg < 1 || (!ego_nei && n_seg != 1)) return COPO_ERR_DIM;
    if (n_wg < 0 || n_wg > SEQ_MAX_WG) return COPO_ERR_DIM;
    if (k_count < 0) k_count = n_mb - k_first;          // (-1: all steps from k_first on)
    if (k_first < 0 || k_first + k_count > n_mb) return COPO_ERR_DIM;
    // measured (scripts/meta_seq_time.py, 90 steps): one workgroup 2.4 / 2.6 / 3.3 / 4.9 us per step with the rows of 1 / 2 / 4 / 8
    // ranks (eight rows per thread are still latency, not work), the hand-over ~2.4 us per step on top of a workgroup's own rows
    // (8 ranks on 8 workgroups: 4.9 us) -- so several workgroups only pay beyond eight ranks' rows: then one per four segments
    if (n_wg == 0) n_wg = (n_seg > 8 && exchange) ? ((n_seg + 3) / 4 < SEQ_MAX_WG ? (n_seg + 3) / 4 : SEQ_MAX_WG) : 1;
    if (n_wg > 1 && !exchange) return COPO_ERR_NULL;
    if (n_mb == 0 || k_count == 0) return COPO_OK;
    MetaSeqArgs a{pack_src, rows, ego_nei, w, eps, denom, gv, stats_in, mb, n_mb, n_seg, pack_width, col_adv, col_nei_adv,
                  k_first, k_count, lcf_param, raw_mean_std, adam_state, lr, stats, exchange, n_wg};
    hipLaunchKernelGGL(meta_seq_kernel, dim3(n_wg), dim3(512), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

extern "C" int copo_meta_lcf_f64(const float* pack_src, int32_t pack_width, int32_t col_adv, int32_t col_nei_adv,
                                 const int64_t* rows, const float* w, const float* denom, const double* eps, int32_t mb,
                                 const int64_t* mb_index, const double* lcf_param, const double* raw_mean_std, double* tail,
                                 void* stream) {
    if (!pack_src || !rows || !w || !denom || !eps || !lcf_param || !raw_mean_std || !tail) return COPO_ERR_NULL;
    if (mb < 1) return COPO_ERR_DIM;
    MetaArgs a{pack_src, rows, w, denom, eps, mb_index, mb, pack_width, col_adv, col_nei_adv, lcf_param, raw_mean_std, tail};
    hipLaunchKernelGGL(meta_lcf_kernel, dim3(1), dim3(512), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

extern "C" int copo_meta_finish_f64(const float* g_new, const float* g_old, int64_t n, const double* dot_partials,
                                    const double* tail, double* lcf_param, double* adam_state, double lr,
                                    float* stats_new, float* stats_old, double* stats, int64_t* mb_index,
                                    int32_t bump_index, void* stream) {
    if (!tail || !lcf_param || !adam_state) return COPO_ERR_NULL;
    if (!dot_partials && (!g_new || !g_old)) return COPO_ERR_NULL;
    if (n < 0) return COPO_ERR_DIM;
    MetaFinishArgs a{g_new, g_old, n, dot_partials, COPO_META_DOT_PARTIALS, tail, lcf_param, adam_state, lr, stats_new,
                     stats_old, stats, mb_index, (mb_index && bump_index) ? 1 : 0};
    hipLaunchKernelGGL(meta_finish_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}

extern "C" int copo_adam_step_f32(const copo_ppo_cfg* cfg, float* theta, float* adam_m, float* adam_v, const float* grad,
                                  int64_t n, int64_t* step, int64_t* mb_index, float* theta_t, float* workspace,
                                  void* stream) {
    if (!cfg || !theta || !adam_m || !adam_v || !grad || !step) return COPO_ERR_NULL;
    if (n < 0) return COPO_ERR_DIM;
    FusedArgs a;
    memset(&a, 0, sizeof(a));
    a.c = *cfg;
    a.theta = theta; a.adam_m = adam_m; a.adam_v = adam_v; a.grad = const_cast<float*>(grad); a.step = step;
    a.kptr = mb_index; a.bump_k = mb_index ? 1 : 0;
    a.theta_t = theta_t;
    a.ws = workspace;        // non-NULL: step number / next index come from the slots the gradient pass published
    a.gcap = 4; a.nreg = 2;
    hipError_t e = launch_adam_flat(a, n, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? COPO_OK : COPO_ERR_DEVICE;
}
