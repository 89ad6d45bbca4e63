// C entry points of the low-precision policy forward (include/copo_hip.h): argument checks in front of the launchers
// of lowp_kernels.hip, and the host-side checker of the rounding functions.
#include "capi_common.h"
#include "lowp_common.h"

using namespace copo;

// what both entry points ask of the configuration and the image; the message names the entry point
static int lowp_check(const char* who, const copo_ppo_cfg* cfg, int32_t fmt, int32_t n_members, const void* packed, int64_t packed_stride) {
    if (!cfg || !packed) return fail(COPO_ERR_NULL, "%s: NULL argument", who);
    if (fmt != COPO_LOWP_BF16 && fmt != COPO_LOWP_E4M3) return fail(COPO_ERR_DIM, "%s: fmt=%d (COPO_LOWP_BF16 or COPO_LOWP_E4M3)", who, fmt);
    const int H = cfg->hidden;
    if ((H != 64 && H != 128 && H != 256 && H != 512) || cfg->pol.in_dim < 1 || cfg->pol.out_dim != 4 || cfg->act_dim != 2 || cfg->n_params < 1)
        return fail(COPO_ERR_DIM, "%s: hidden=%d (64 / 128 / 256 / 512) in_dim=%d (>= 1) out_dim=%d (4)", who, H, cfg->pol.in_dim, cfg->pol.out_dim);
    if (n_members < 1 || n_members > 65535) return fail(COPO_ERR_DIM, "%s: n_members=%d (1..65535)", who, n_members);
    const LowpLay L(H, cfg->pol.in_dim, fmt);
    if (packed_stride < (int64_t)L.total() || packed_stride % 16 != 0 || (reinterpret_cast<uintptr_t>(packed) & 15) != 0)
        return fail(COPO_ERR_DIM, "%s: packed_stride=%lld bytes (>= %zu, a multiple of 16) and a 16-byte aligned image wanted", who,
                    (long long)packed_stride, L.total());
    return COPO_OK;
}

extern "C" int copo_lowp_pack(const copo_ppo_cfg* cfg, const float* theta, int64_t member_stride, int32_t n_members, int32_t fmt, void* packed,
                              int64_t packed_stride, void* stream) {
    const int rc = lowp_check("copo_lowp_pack", cfg, fmt, n_members, packed, packed_stride);
    if (rc != COPO_OK) return rc;
    if (!theta) return fail(COPO_ERR_NULL, "copo_lowp_pack: NULL theta");
    if (member_stride < cfg->n_params) return fail(COPO_ERR_DIM, "copo_lowp_pack: member_stride=%lld below n_params", (long long)member_stride);
    HIP_TRY(launch_lowp_pack(*cfg, theta, member_stride, n_members, fmt, static_cast<uint8_t*>(packed), packed_stride, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_lowp_forward_seats(const copo_ppo_cfg* cfg, const void* packed, int64_t packed_stride, int32_t fmt, int32_t n_members,
                                       const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out, const float* obs_src,
                                       float* dist_inputs, const float* eps, float* action, float* logp, float* clipped, void* stream) {
    const int rc = lowp_check("copo_lowp_forward_seats", cfg, fmt, n_members, packed, packed_stride);
    if (rc != COPO_OK) return rc;
    if (!rows || !counts || !obs_src || (!dist_inputs && !eps) || (eps && (!action || !logp)))
        return fail(COPO_ERR_NULL, "copo_lowp_forward_seats: NULL argument (rows, counts, obs_src; dist_inputs or eps; action and logp with eps)");
    if (cap < 1 || n_out < 1 || (cap + 15) / 16 > 0x7fffffff) return fail(COPO_ERR_DIM, "copo_lowp_forward_seats: cap=%lld n_out=%lld (>= 1)", (long long)cap, (long long)n_out);
    if (dist_inputs && (reinterpret_cast<uintptr_t>(dist_inputs) & 15) != 0)
        return fail(COPO_ERR_DIM, "copo_lowp_forward_seats: dist_inputs must be 16-byte aligned (a row is stored as one 128-bit word)");
    const size_t lds = lowp_fwd_lds_bytes(cfg->hidden, cfg->pol.in_dim, fmt);
    if (lds > 64 * 1024) return fail(COPO_ERR_DIM, "copo_lowp_forward_seats: in_dim=%d needs %zu bytes of LDS (64 KiB at the most)", cfg->pol.in_dim, lds);
    const LowpFwdArgs a{static_cast<const uint8_t*>(packed), packed_stride, rows, counts, cap, n_out, obs_src, cfg->pol.in_dim, dist_inputs, eps,
                        action, logp, clipped};
    HIP_TRY(launch_lowp_forward(cfg->hidden, fmt, n_members, a, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

// host only: out[i] = the value in[i] rounds to in `fmt` (tests: the rounding code of the kernels against framework casts)
extern "C" int copo_debug_lowp_round(int32_t fmt, const float* in, int64_t n, float* out) {
    if (!in || !out) return fail(COPO_ERR_NULL, "copo_debug_lowp_round: NULL argument");
    if ((fmt != COPO_LOWP_BF16 && fmt != COPO_LOWP_E4M3) || n < 0) return fail(COPO_ERR_DIM, "copo_debug_lowp_round: fmt=%d n=%lld", fmt, (long long)n);
    for (int64_t i = 0; i < n; ++i) out[i] = lowp_round(fmt, in[i]);
    return COPO_OK;
}

// host only: the scale of an e4m3 weight row whose largest magnitude is amax[i]
extern "C" int copo_debug_lowp_scale(const float* amax, int64_t n, float* out) {
    if (!amax || !out) return fail(COPO_ERR_NULL, "copo_debug_lowp_scale: NULL argument");
    for (int64_t i = 0; i < n; ++i) out[i] = e4m3_row_scale(amax[i]);
    return COPO_OK;
}
