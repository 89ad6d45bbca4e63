// C entry point of the value pass of a seated bank (include/copo_hip.h): argument checks in front of the launcher
// of value_kernels.hip.
#include "capi_common.h"
#include "value_common.h"

using namespace copo;

extern "C" int copo_value_obs_seats_f32(const copo_ppo_cfg* cfg, const float* theta, const float* theta_t, int64_t member_stride,
                                        int32_t n_members, const int64_t* rows, const int32_t* counts, int64_t cap, int64_t n_out,
                                        const float* obs_src, const float* cc_src, float* values, void* stream) {
    const char* who = "copo_value_obs_seats_f32";
    if (!cfg || !theta || !theta_t || !rows || !counts || !obs_src || !values)
        return fail(COPO_ERR_NULL, "%s: NULL argument (cfg, theta, theta_t, rows, counts, obs_src, values)", who);
    const int H = cfg->hidden, nv = cfg->n_value_heads;
    if ((H != 64 && H != 128 && H != 256 && H != 512) || nv < 1 || nv > 3 || cfg->operand_dtype != COPO_OPERAND_F32 || cfg->n_params < 1)
        return fail(COPO_ERR_DIM, "%s: hidden=%d (64 / 128 / 256 / 512) n_value_heads=%d (1..3) operand_dtype=%d (fp32 only)", who, H, nv,
                    cfg->operand_dtype);
    if (cap < 1 || n_out < 1 || (cap + 15) / 16 > 0x7fffffff || n_members < 1 || n_members > 65535 || member_stride < cfg->n_params ||
        member_stride % 4 != 0)
        return fail(COPO_ERR_DIM, "%s: cap=%lld n_out=%lld (>= 1) n_members=%d (1..65535) member_stride=%lld (a multiple of 4, at least n_params)",
                    who, (long long)cap, (long long)n_out, n_members, (long long)member_stride);
    if ((reinterpret_cast<uintptr_t>(theta_t) & 15) != 0) return fail(COPO_ERR_DIM, "%s: the transposed mirror must be 16-byte aligned", who);
    for (int h = 0; h < nv; ++h) {
        const copo_net_layout& L = cfg->val[h];
        // every net of one launch reads one source: the heads of one configuration share their input width
        if (L.in_dim < 1 || L.in_dim != cfg->val[0].in_dim || L.out_dim != 1 || L.w1 % 4 != 0 || L.w2 % 4 != 0 || L.w1 < 0 || L.w2 < 0 || L.w3 < 0 ||
            L.b1 < 0 || L.b2 < 0 || L.b3 < 0 || L.b3 >= cfg->n_params)
            return fail(COPO_ERR_DIM, "%s: value net %d: in_dim=%d (>= 1, one width for every head) out_dim=%d (1), W1 / W2 offsets multiples of 4 "
                        "inside n_params", who, h, L.in_dim, L.out_dim);
    }
    const size_t lds = value_seats_lds_bytes(*cfg);
    if (lds == 0 || lds > 150 * 1024)
        return fail(COPO_ERR_DIM, "%s: in_dim=%d needs %zu bytes of LDS (150 KiB at the most)", who, cfg->val[0].in_dim, lds);
    const ValueSeatArgs a{*cfg, theta, theta_t, member_stride, rows, counts, cap, n_out, cc_src ? cc_src : obs_src, values, n_members};
    HIP_TRY(launch_value_seats(a, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}
