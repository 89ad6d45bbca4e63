// Part of learn_fused.hip (one translation unit), host only: the kernel table and the launch plan.  Nothing here calls HIP.
// ------------------------------------------------------------------------------------------------------------
// kernel table: every instantiation the fused learner launches, once.  X(id, workgroup size, dynamic-LDS ceiling, kernel)
// ------------------------------------------------------------------------------------------------------------
constexpr int LDS_DEFAULT = 64 * 1024;      // what a kernel may use without an attribute
constexpr int LDS_ROWPASS = 150 * 1024;     // row-pass / forward workgroups (gfx950 has 160 KB per CU)
constexpr int LDS_GEMM = (int)GEMM_LDS_BYTES;
constexpr int LDS_LINBOUND = 136 * 1024;    // lin_obs_kernel keeps 11.5 KB of static partial sums next to its tiles: together under the CU's 160 KB
// a family of the four row-pass shapes, hidden = 16 NT WAVES = 64, 128, 256, 512: adjacent ids in this order (shape_index)
#define COPO_SHAPES(X, id, K, ...)                                                                                          \
    X(id##_1_4, 256, LDS_ROWPASS, K<1, 4, __VA_ARGS__>) X(id##_2_4, 256, LDS_ROWPASS, K<2, 4, __VA_ARGS__>)                   \
    X(id##_2_8, 512, LDS_ROWPASS, K<2, 8, __VA_ARGS__>) X(id##_4_8, 512, LDS_ROWPASS, K<4, 8, __VA_ARGS__>)
#define COPO_KERNELS(X)                                                                                                     \
    COPO_SHAPES(X, RP, rowpass_kernel, false) COPO_SHAPES(X, RP_TW, rowpass_kernel, true) COPO_SHAPES(X, RP_BF, rowpass_kernel, true, true) \
    X(RP_HO_2_8, 512, LDS_ROWPASS, rowpass_kernel<2, 8, true, false, true>)                                                  \
    X(RP_HO_2_8_RT8, 512, LDS_ROWPASS, rowpass_kernel<2, 8, true, false, true, 8>)                                           \
    X(RP_TW_2_8_RT8, 512, LDS_ROWPASS, rowpass_kernel<2, 8, true, false, false, 8>)                                          \
    X(RP8_4, 64 * R8_KS * 4, LDS_ROWPASS, rowpass8_kernel<4>) X(RP8_4_BF, 64 * R8_KS * 4, LDS_ROWPASS, rowpass8_kernel<4, true>) \
    COPO_SHAPES(X, FWD, mlp_fwd_kernel, false) COPO_SHAPES(X, FWD_BF, mlp_fwd_kernel, true)                                  \
    COPO_SHAPES(X, FWD_BANK, mlp_fwd_kernel, false, 1, true) COPO_SHAPES(X, FWD_BANK_BF, mlp_fwd_kernel, true, 1, true)      \
    X(FWD_RT2, 512, LDS_ROWPASS, mlp_fwd_kernel<2, 8, false, 2>) X(FWD_BF_RT2, 512, LDS_ROWPASS, mlp_fwd_kernel<2, 8, true, 2>) \
    X(FWD_BANK_RT2, 512, LDS_ROWPASS, mlp_fwd_kernel<2, 8, false, 2, true>)                                                  \
    X(FWD_BANK_BF_RT2, 512, LDS_ROWPASS, mlp_fwd_kernel<2, 8, true, 2, true>)                                                \
    /* scalar variant, then vector variant (id + 1) */                                                                      \
    X(GEMM_F1, 256, LDS_GEMM, gemm_kernel<FwdOpT<1>, false>) X(GEMM_F1_VEC, 256, LDS_GEMM, gemm_kernel<FwdOpT<1>, true>)     \
    X(GEMM_F2, 256, LDS_GEMM, gemm_kernel<FwdOpT<2>, false>) X(GEMM_F2_VEC, 256, LDS_GEMM, gemm_kernel<FwdOpT<2>, true>)     \
    X(GEMM_BX, 256, LDS_GEMM, gemm_kernel<BxOp, false>) X(GEMM_BX_VEC, 256, LDS_GEMM, gemm_kernel<BxOp, true>)               \
    X(GEMM_BW, 256, LDS_GEMM, gemm_bw_kernel<false>) X(GEMM_BW_VEC, 256, LDS_GEMM, gemm_bw_kernel<true>)                     \
    X(GEMM_BW_GA, 256, LDS_GEMM, gemm_bw_kernel<false, true>) X(GEMM_BW_GA_VEC, 256, LDS_GEMM, gemm_bw_kernel<true, true>)   \
    X(WGRAD, 64 * WG_WAVES, LDS_DEFAULT, wgrad_adam_kernel<1>) X(WGRAD_FAST, 64 * WG_WAVES, LDS_DEFAULT, wgrad_adam_kernel<1, false, true>) \
    X(WGRAD_BF, 64 * WG_WAVES, LDS_DEFAULT, wgrad_adam_kernel<1, true>)                                                      \
    X(WGRAD_BF_FAST, 64 * WG_WAVES, LDS_DEFAULT, wgrad_adam_kernel<1, true, true>)                                           \
    X(WGRAD_OT2, 64 * WG_WAVES, 80 * 1024, wgrad_adam_kernel<2>)                                                             \
    X(HEAD, 256, LDS_DEFAULT, head_kernel) X(META_FOLD, 256, LDS_DEFAULT, meta_batch_fold_kernel)                            \
    X(REDUCE_ADAM, 256, LDS_DEFAULT, reduce_adam_kernel)
// rows behind the learner's: kernels of the evaluation side that live in this translation unit (learn_seat.inc, learn_inputgrad.inc, learn_pgd.inc, learn_certify.inc, learn_linbound.inc, learn_jury.inc, learn_attrib.inc, learn_hidden.inc).  They are launched
// through the same launch_kernel and get their LDS ceilings from the same loop; copo_debug_learner_kernel lists the learner's rows only
// (ids below K_LEARNER_COUNT).  Per kernel the four shapes in shape_index order.
#define COPO_EVAL_KERNELS(X)                                                                                                \
    X(ADV_1_4, 256, LDS_ROWPASS, adv_obs_kernel<1, 4>) X(ADV_2_4, 256, LDS_ROWPASS, adv_obs_kernel<2, 4>)                    \
    X(ADV_2_8, 512, LDS_ROWPASS, adv_obs_kernel<2, 8>) X(ADV_4_8, 512, LDS_ROWPASS, adv_obs_kernel<4, 8>)                    \
    X(PGD_1_4, 256, LDS_ROWPASS, pgd_obs_kernel<1, 4>) X(PGD_2_4, 256, LDS_ROWPASS, pgd_obs_kernel<2, 4>)                    \
    X(PGD_2_8, 512, LDS_ROWPASS, pgd_obs_kernel<2, 8>) X(PGD_4_8, 512, LDS_ROWPASS, pgd_obs_kernel<4, 8>)                    \
    X(CERT_1_4, 256, LDS_ROWPASS, cert_obs_kernel<1, 4>) X(CERT_2_4, 256, LDS_ROWPASS, cert_obs_kernel<2, 4>)                \
    X(CERT_2_8, 512, LDS_ROWPASS, cert_obs_kernel<2, 8>) X(CERT_4_8, 512, LDS_ROWPASS, cert_obs_kernel<4, 8>)              \
    X(LIN_1_4, 256, LDS_LINBOUND, lin_obs_kernel<1, 4>) X(LIN_2_4, 256, LDS_LINBOUND, lin_obs_kernel<2, 4>)                  \
    X(LIN_2_8, 512, LDS_LINBOUND, lin_obs_kernel<2, 8>) X(LIN_4_8, 512, LDS_LINBOUND, lin_obs_kernel<4, 8>)                  \
    X(JURY_1_4, 256, LDS_ROWPASS, jury_obs_kernel<1, 4>) X(JURY_2_4, 256, LDS_ROWPASS, jury_obs_kernel<2, 4>)                \
    X(JURY_2_8, 512, LDS_ROWPASS, jury_obs_kernel<2, 8>) X(JURY_4_8, 512, LDS_ROWPASS, jury_obs_kernel<4, 8>)                \
    X(IG_1_4, 256, LDS_ROWPASS, ig_obs_kernel<1, 4>) X(IG_2_4, 256, LDS_ROWPASS, ig_obs_kernel<2, 4>)                        \
    X(IG_2_8, 512, LDS_ROWPASS, ig_obs_kernel<2, 8>) X(IG_4_8, 512, LDS_ROWPASS, ig_obs_kernel<4, 8>)                        \
    X(HIDDEN_1_4, 256, LDS_ROWPASS, hidden_obs_kernel<1, 4>) X(HIDDEN_2_4, 256, LDS_ROWPASS, hidden_obs_kernel<2, 4>)        \
    X(HIDDEN_2_8, 512, LDS_ROWPASS, hidden_obs_kernel<2, 8>) X(HIDDEN_4_8, 512, LDS_ROWPASS, hidden_obs_kernel<4, 8>)
struct KernelEntry { const char* name; const void* fn; int block, lds_cap; };
#define COPO_KERNEL_ID(id, block, cap, ...) K_##id,
#define COPO_KERNEL_ENTRY(id, block, cap, ...) {#__VA_ARGS__, reinterpret_cast<const void*>(__VA_ARGS__), block, cap},
enum KernelId : int32_t { COPO_KERNELS(COPO_KERNEL_ID) COPO_EVAL_KERNELS(COPO_KERNEL_ID) K_COUNT };
constexpr int K_LEARNER_COUNT = K_ADV_1_4;
static const KernelEntry g_kernels[K_COUNT] = {COPO_KERNELS(COPO_KERNEL_ENTRY) COPO_EVAL_KERNELS(COPO_KERNEL_ENTRY)};
static int shape_index(int hidden) { return hidden == 64 ? 0 : hidden == 128 ? 1 : hidden == 256 ? 2 : hidden == 512 ? 3 : -1; }

struct Launch { int32_t id; uint32_t gx, gy, gz; int32_t block, lds; int32_t arg[4]; };      // arg: the kernel's int arguments after its struct

// ------------------------------------------------------------------------------------------------------------
// launch plan: which kernels a configuration takes, with which grid -- pure host code, no HIP call
// ------------------------------------------------------------------------------------------------------------
size_t fused_ws_floats(const copo_ppo_cfg& c) { return WsLay(c, 4, 2).total(); }
static int pick_ksplit(int mb) { return mb < 256 ? 1 : mb / 128 > COPO_PPO_MAX_KSPLIT ? COPO_PPO_MAX_KSPLIT : mb / 128; }
// group slabs / gradient regions of the batched layouts for `nb` minibatches (> 4: see WsLay)
static int batch_gcap(int nb) { return 2 * nb > 4 ? 2 * nb : 8; }

// The shipped library takes no environment variables: one code path, all of the work, every time.  Profiling builds
// (`make prof`, -DCOPO_PROFILE_SKIP=<mask>, a separate .so that the package never loads) read COPO_RP_DBG for the
// phase-stamp / phase-skip bits of the row pass and can fall back to the older kernel chains for A/B measurements.
struct Switches { bool rowpass_4x4, rowpass_rt8, use_wgrad, use_rowpass; int wgrad_ot; };
#ifdef COPO_PROFILE_SKIP
static bool env_not_0(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }
static Switches switches() {
    static const Switches sw = {env_not_0("COPO_ROWPASS_4X4"), env_not_0("COPO_ROWPASS_RT8"), env_not_0("COPO_FUSED_WGRAD"), env_not_0("COPO_FUSED_ROWPASS"),
                                [] { const char* e = getenv("COPO_WGRAD_OT"); return (e && e[0] == '2') ? 2 : 1; }()};
    return sw;
}
static int profile_dbg_bits() { static const int dbg = [] { const char* e = getenv("COPO_RP_DBG"); return e ? atoi(e) : 0; }(); return dbg; }
#else
static constexpr Switches switches() { return {true, true, true, true, 1}; }
static constexpr int profile_dbg_bits() { return 0; }
#endif

// [lo, lo + n): the span of the flat parameter buffer that the first `nets` networks of the layout occupy
static void fold_range(const copo_ppo_cfg& c, int nets_n, int64_t* lo_out, int* n_out) {
    const copo_net_layout* nets[4] = {&c.pol, &c.val[0], &c.val[1], &c.val[2]};
    int64_t lo = c.pol.w1, hi = 0;
    for (int g = 0; g < nets_n; ++g) {
        const int64_t offs[6] = {nets[g]->w1, nets[g]->b1, nets[g]->w2, nets[g]->b2, nets[g]->w3, nets[g]->b3};
        const int64_t szs[6] = {(int64_t)c.hidden * nets[g]->in_dim, c.hidden, (int64_t)c.hidden * c.hidden, c.hidden,
                                (int64_t)nets[g]->out_dim * c.hidden, nets[g]->out_dim};
        for (int t = 0; t < 6; ++t) {
            lo = offs[t] < lo ? offs[t] : lo;
            hi = offs[t] + szs[t] > hi ? offs[t] + szs[t] : hi;
        }
    }
    *lo_out = lo;
    *n_out = (int)(hi - lo);
}

// who calls: the modes from PLAN_META_PAIR on run both policies of the LCF meta update (MODE_META_BOTH), those from PLAN_META_BATCH
// on `nb` minibatches per launch
enum PlanMode : int32_t {
    PLAN_PPO_STEP,          // one minibatch step with Adam (head mode PPO, or one policy of the legacy two-call meta step)
    PLAN_PPO_GRADS,         // the same without Adam: gradients only
    PLAN_DP_STEP,           // the PPO step of a data-parallel rank
    PLAN_META_PAIR,         // step-by-step meta pair
    PLAN_META_PAIR_TAIL,    // ... whose fold also runs the LCF step
    PLAN_META_BATCH,        // batched meta pass
    PLAN_ROW_STORE,         // row-local kernels only: fill the meta row store (nb = identity row blocks)
    PLAN_ROW_WGRADS,        // weight-gradient GEMMs that gather from the row store + fold
    PLAN_FORWARD            // (plan_forward; copo_debug_learner_plan only)
};
// what the plan needs to know about the caller's pointers
enum PlanFacts : int32_t {
    FACT_ALIGNED = 1,           // sources, parameters and workspace 16-byte aligned
    FACT_MIRROR = 2,            // transposed mirror present
    FACT_MIRROR_ALIGNED = 4,    // ... and it, the parameters and the workspace 16-byte aligned
    FACT_STORE_OK = 8,          // row store 16-byte aligned, every operand slab below 4 GB (32-bit byte offsets of the buffer loads)
    FACT_SEATS = 16,            // PLAN_FORWARD of a bank: seat mode (copo_mlp_forward_seats_f32), `n_rows` is the lists' capacity
};
struct Plan {
    bool refused;               // the entry points answer COPO_ERR_DEVICE and launch nothing
    int n;
    Launch l[6];
    int groups, ksplit, stat_tiles;     // FusedArgs fields of the same names
    int wgrad_tiles;            // workgroups of the weight-gradient kernel (sizes the data-parallel exchange workspace)
    int64_t lo;                 // the fold covers parameters [lo, lo + n_fold) in fold_blocks workgroups
    int n_fold, fold_blocks;
    bool refresh_mirror;        // the chain's Adam does not write the transposed mirror: bring it up to date afterwards
};
static void plan_add(Plan& p, int id, uint32_t gx, uint32_t gy, uint32_t gz, size_t lds, int a0 = 0, int a1 = 0, int a2 = 0, int a3 = 0) {
    p.l[p.n++] = Launch{id, gx, gy, gz, g_kernels[id].block, (int32_t)lds, {a0, a1, a2, a3}};
}

// head: COPO_HEAD_* of the PPO-step modes (the meta modes have their own); nb: minibatches of the batched modes; world: data-parallel ranks
static Plan plan_step(const copo_ppo_cfg& c, PlanMode mode, int head, int nb, int world, int facts, const Switches& sw) {
    Plan p{};
    const bool both = mode >= PLAN_META_PAIR, batched = mode >= PLAN_META_BATCH, ppo_head = !both && head == COPO_HEAD_PPO;
    const bool adam = mode == PLAN_PPO_STEP || mode == PLAN_DP_STEP;
    const int nets_n = ppo_head ? 1 + c.n_value_heads : 1, G = batched ? 2 * nb : both ? 2 : nets_n;
    const int H = c.hidden, mt = (c.mb + TM - 1) / TM, ht = (H + TN - 1) / TN;
    const copo_net_layout* nets[4] = {&c.pol, &c.val[0], &c.val[1], &c.val[2]};
    int kmax1 = 0;
    bool in4 = true, off4 = true;
    for (int g = 0; g < nets_n; ++g) {
        kmax1 = nets[g]->in_dim > kmax1 ? nets[g]->in_dim : kmax1;
        in4 = in4 && nets[g]->in_dim % 4 == 0;
        off4 = off4 && nets[g]->w1 % 4 == 0 && nets[g]->w2 % 4 == 0;
    }
    // vector path: every row the kernels touch is 16-byte aligned and a multiple of 4 floats long
    const bool vec = H % 4 == 0 && in4 && off4 && (facts & FACT_ALIGNED) && (mode != PLAN_ROW_WGRADS || (facts & FACT_STORE_OK));
    // with the transposed mirror the row pass reads no k-contiguous weight rows, so input widths that are not a
    // multiple of 4 (the 91-dim observation of IPPO / CCPPO) only cost a scalar input gather
    const bool tw = (facts & FACT_MIRROR) && !both, tw_ok = tw && H % 4 == 0 && off4 && (facts & FACT_MIRROR_ALIGNED);
    // row pass (one kernel for F1, F2, heads, B2x) for the shapes with an instantiation; else the four separate kernels
    const int sh = shape_index(H);
    const size_t rp_lds = rowpass_lds_floats(H, rowpass_k1p(kmax1)) * sizeof(float);
    const bool rowpass = (vec || tw_ok) && !batched && sw.use_rowpass && sh >= 0 && rp_lds <= (size_t)LDS_ROWPASS;
    // bfloat16 operands: only the row pass + fused weight-gradient kernels round where torch.autocast rounds
    const bool bf = c.operand_dtype == COPO_OPERAND_BF16;
    if (bf && !(rowpass && tw_ok && ppo_head && sw.use_wgrad)) p.refused = true;
    p.groups = G;
    p.ksplit = batched ? 1 : pick_ksplit(c.mb);
    p.stat_tiles = head_tiles(c);
    if (rowpass) {
        // 8-row tiles where 16-row tiles would leave compute units without a workgroup (rowpass_kernel, RT): the production
        // shape only (hidden 256 through the transposed mirror)
        const bool rt8 = tw && H == 256 && head_tiles(c) * G <= 160 && sw.rowpass_rt8 && (!bf || sw.rowpass_4x4), r8 = rt8 && sw.rowpass_4x4;
        const bool ho = H == 256 && kmax1 <= 128;      // hidden 256: layer 2 is two ring turns -> hand-over variant for narrow inputs
        if (rt8) p.stat_tiles = (c.mb + 7) / 8;
        const int id = bf ? (r8 ? K_RP8_4_BF : K_RP_BF_1_4 + sh) : r8 ? K_RP8_4 : rt8 ? (ho ? K_RP_HO_2_8_RT8 : K_RP_TW_2_8_RT8)
                          : tw ? (ho ? K_RP_HO_2_8 : K_RP_TW_1_4 + sh) : K_RP_1_4 + sh;
        plan_add(p, id, p.stat_tiles, G, 1, r8 ? rowpass8_lds_floats(256, rowpass8_k1p(kmax1)) * sizeof(float) : rp_lds);
    } else if (mode != PLAN_ROW_WGRADS) {
        plan_add(p, K_GEMM_F1 + vec, ht, mt, G, gemm_lds_bytes(c.mb), kmax1);
        plan_add(p, K_GEMM_F2 + vec, ht, mt, G, gemm_lds_bytes(c.mb), H);
        plan_add(p, K_HEAD, head_tiles(c), G, 1, (size_t)(HT * (H + 1) + 4 * H + HT * 4 + 32) * sizeof(float));
        plan_add(p, K_GEMM_BX + vec, ht, mt, G, gemm_lds_bytes(c.mb), H);
    }
    if (mode == PLAN_ROW_STORE) return p;
    if (world > 1 && (both || !sw.use_wgrad || sw.wgrad_ot != 1 || !adam)) p.refused = true;
    if (!both && sw.use_wgrad) {
        // weight gradients, fold and Adam in one kernel: the SGD step ends here
        const int ot = sw.wgrad_ot, nty = (H + 32 * ot - 1) / (32 * ot), wx2 = (H + 1 + 31) / 32, wx1 = (kmax1 + 1 + 31) / 32;
        const bool fastk = c.mb == 2 * WG_RING * WG_WAVES && (bf || ot == 1);      // buffer-load operand ring (learn_update.inc)
        const int id = bf ? (fastk ? K_WGRAD_BF_FAST : K_WGRAD_BF) : ot == 2 ? K_WGRAD_OT2 : fastk ? K_WGRAD_FAST : K_WGRAD;
        plan_add(p, id, (wx2 + wx1) * nty + wx2, G, 1, (size_t)WG_WAVES * 32 * (bf ? 1 : ot) * 33 * sizeof(float), nty, wx2, wx1);
        p.wgrad_tiles = ((wx2 + wx1) * nty + wx2) * G;
        return p;
    }
    // layers 2 / 3: no tile for the bias column alone when the hidden width fills whole tiles (BwOpT::bias_by_rowsum)
    const int nx2 = (H % TN == 0) ? H / TN : (H + 1 + TN - 1) / TN, nx1 = (kmax1 + 1 + TN - 1) / TN;
    const bool ga = mode == PLAN_ROW_WGRADS;       // gather-all mode; vector rows: the head layer is one workgroup on the lanes (head_wgrad_lanes)
    plan_add(p, (ga ? K_GEMM_BW_GA : K_GEMM_BW) + vec, (nx2 + nx1) * ht + (ga && vec ? 1 : nx2), G * p.ksplit, 1, gemm_lds_bytes(c.mb), c.mb, nx2, nx1, ht);
    // parameter range the fold covers: every net of this call (the policy only in the meta modes)
    fold_range(c, nets_n, &p.lo, &p.n_fold);
    p.fold_blocks = (p.n_fold + 256 * FOLD_EPT - 1) / (256 * FOLD_EPT);
    if (both && p.fold_blocks > COPO_META_DOT_PARTIALS) p.refused = true;
    if (batched) plan_add(p, K_META_FOLD, p.fold_blocks, nb, 1, 0);
    else plan_add(p, K_REDUCE_ADAM, p.fold_blocks, 1, 1, 0);
    p.refresh_mirror = !batched && adam && (facts & FACT_MIRROR) && ppo_head;
    return p;
}

// Forward-only pass.  n_members = 0: one parameter set, `n_rows` rows.  n_members >= 1 (copo_mlp_forward_bank_f32): the member is the
// grid's second dimension, `n_rows` rows EACH.  The variant rule counts a member's rows, not the launch's: the two-tile variant rounds a
// few rows in ten thousand differently from the one-tile variant (measured: 1 row of 16 536), and a member's rows must hold the bits of
// a launch of that member alone.
// FACT_SEATS (copo_mlp_forward_seats_f32): every member owns a row list of up to `n_rows` rows.  How many it holds is known on the device
// only, so the variant cannot follow it: seat mode always takes the one-tile variant, whatever the capacity, and a member's rows hold
// the bits of the one-tile single-member kernel (at hidden 256: of a single-member launch of fewer than 2 * 32 * 256 rows).
static int plan_forward(const copo_ppo_cfg& c, int64_t n_rows, int first_net, int n_nets, int n_members, int facts, Launch* out) {
    if (n_rows < 1 || first_net < 0 || n_nets < 1 || first_net + n_nets > 1 + c.n_value_heads) return COPO_ERR_DIM;
    const int H = c.hidden, sh = shape_index(H);
    if (sh < 0 || !(facts & FACT_MIRROR_ALIGNED)) return COPO_ERR_DIM;
    int kmax = 0;
    const copo_net_layout* nets[4] = {&c.pol, &c.val[0], &c.val[1], &c.val[2]};
    for (int g = first_net; g < first_net + n_nets; ++g) {
        kmax = nets[g]->in_dim > kmax ? nets[g]->in_dim : kmax;
        if (nets[g]->w1 % 4 != 0 || nets[g]->w2 % 4 != 0) return COPO_ERR_DIM;
    }
    // hidden 256 with at least two rounds of 256 workgroups of 32 rows per net: two 16-row tiles per workgroup (learn_rowpass.inc:
    // RT).  Measured: the critic heads on 72 k rows 580 -> 478 us; a rollout step's 10 240 rows (320 workgroups of 32 rows on 256
    // CUs) 39.5 -> 43.8 us, hence the threshold
    const bool seats = (facts & FACT_SEATS) != 0;
    if (seats && n_members < 1) return COPO_ERR_DIM;
    const bool rt2 = !seats && H == 256 && n_rows >= 2 * 32 * 256 && rowpass_k1p(kmax) <= H;
    const size_t lds = rt2 ? ((size_t)2 * 2 * HT * (H + 4) + 4 * H) * sizeof(float)
                           : ((size_t)HT * (rowpass_k1p(kmax) + 4) + (size_t)2 * HT * (H + 4) + 4 * H) * sizeof(float);
    if (lds > (size_t)LDS_ROWPASS) return COPO_ERR_DIM;
    const bool bank = n_members > 0, bf = c.operand_dtype == COPO_OPERAND_BF16;
    const int id = rt2 ? (bank ? (bf ? K_FWD_BANK_BF_RT2 : K_FWD_BANK_RT2) : bf ? K_FWD_BF_RT2 : K_FWD_RT2)
                       : (bank ? (bf ? K_FWD_BANK_BF_1_4 : K_FWD_BANK_1_4) : bf ? K_FWD_BF_1_4 : K_FWD_1_4) + sh;
    const int rws = rt2 ? 2 * HT : HT;
    *out = Launch{id, (uint32_t)((n_rows + rws - 1) / rws), (uint32_t)(bank ? n_members : n_nets), 1, g_kernels[id].block, (int32_t)lds, {}};
    return COPO_OK;
}

// The four seat passes of a seated bank (copo_adv / pgd / cert / lin_obs_seats_f32; learn_inputgrad.inc, learn_pgd.inc, learn_certify.inc,
// learn_linbound.inc), the jury pass (copo_jury_obs_seats_f32, learn_jury.inc) the attribution pass (copo_ig_obs_seats_f32, learn_attrib.inc) and the hidden-layer pass (copo_hidden_obs_seats_f32, learn_hidden.inc): the launch shape of seat mode -- `cap` rows per member at the most, the member as the grid's second dimension --
// and always the 16-row tile, at every hidden width.  fp32 operands only.  `first_id`: the pass's hidden-64 table entry; `lds_floats`:
// its dynamic LDS (every pass holds at least adv_obs_kernel's two h tiles, one input tile and the W3 rows: the iterate of the PGD pass is
// a second input tile, the bound passes hold three of each); `lds_cap`: LDS_ROWPASS, or LDS_LINBOUND for the linear pass, which keeps
// static partial sums next to its tiles (hidden 512 with an input wider than 128 columns is refused there).
static int plan_seat_pass(const copo_ppo_cfg& c, int64_t cap, int n_members, int facts, int first_id, size_t lds_floats, int lds_cap, Launch* out) {
    const int H = c.hidden, sh = shape_index(H);
    if (cap < 1 || n_members < 1 || n_members > 65535 || (cap + HT - 1) / HT > 0x7fffffff) return COPO_ERR_DIM;
    if (sh < 0 || c.operand_dtype != COPO_OPERAND_F32 || !(facts & FACT_MIRROR_ALIGNED)) return COPO_ERR_DIM;
    if (c.pol.in_dim < 1 || c.pol.w1 % 4 != 0 || c.pol.w2 % 4 != 0) return COPO_ERR_DIM;
    const size_t lds = lds_floats * sizeof(float);
    if (lds > (size_t)lds_cap) return COPO_ERR_DIM;
    const int id = first_id + sh;
    *out = Launch{id, (uint32_t)((cap + HT - 1) / HT), (uint32_t)n_members, 1, g_kernels[id].block, (int32_t)lds, {}};
    return COPO_OK;
}
