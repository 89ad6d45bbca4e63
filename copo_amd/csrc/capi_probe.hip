// C entry points of the linear probes (include/copo_hip.h): argument checks in front of the launchers of
// probe_kernels.hip.
#include "capi_common.h"
#include "probe_common.h"

using namespace copo;

extern "C" int copo_probe_targets(const float* obs, int64_t n_out, int32_t O, int32_t lidar_lo, int32_t num_lasers, const float* trig,
                                  const uint8_t* flags, const float* reward, const int64_t* rows, const int32_t* count, int64_t cap, float* targets,
                                  float* xobs, int32_t Op, void* stream) {
    if (!obs || !trig || !flags || !reward || !rows || !count || !targets || !xobs) return fail(COPO_ERR_NULL, "copo_probe_targets: NULL argument");
    if (n_out < 1 || cap < 1 || cap > INT32_MAX || O < 1 || num_lasers < 1 || lidar_lo < 0 || (int64_t)lidar_lo + num_lasers > O)
        return fail(COPO_ERR_DIM, "copo_probe_targets: n_out=%lld cap=%lld (1..2^31-1) obs_dim=%d lidar_lo=%d num_lasers=%d (>= 1, inside the row)",
                    (long long)n_out, (long long)cap, O, lidar_lo, num_lasers);
    if (Op < O || Op > COPO_PROBE_MAX_WIDTH || Op % GRAM_TILE != 0)
        return fail(COPO_ERR_DIM, "copo_probe_targets: padded width=%d (a multiple of %d from obs_dim=%d up to %d)", Op, GRAM_TILE, O, COPO_PROBE_MAX_WIDTH);
    const ProbeTargetArgs a{obs, trig, flags, reward, rows, count, cap, n_out, O, Op, lidar_lo, num_lasers, targets, xobs};
    HIP_TRY(launch_probe_targets(a, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_probe_accumulate(const float* x, int64_t x_floats, const int64_t* block_base, int32_t n_blocks, int64_t pos_stride, int32_t D,
                                     const float* targets, const int64_t* rows, const int32_t* count, int64_t cap, const uint8_t* flags,
                                     const int32_t* seat, const uint8_t* fold, int64_t n_out, int32_t slots, int32_t rows_of, int32_t n_planes, double* G,
                                     double* C, double* T, void* stream) {
    if (!x || !block_base || !targets || !rows || !count || !flags || !seat || !fold || !G || !C || !T)
        return fail(COPO_ERR_NULL, "copo_probe_accumulate: NULL argument");
    if (D < GRAM_TILE || D > COPO_PROBE_MAX_WIDTH || D % GRAM_TILE != 0 || n_blocks < 1 || n_blocks > COPO_PROBE_MAX_BLOCKS || n_planes < 1 ||
        n_planes > COPO_CKA_MAX_PLANES)
        return fail(COPO_ERR_DIM, "copo_probe_accumulate: width=%d (a multiple of %d up to %d) n_blocks=%d (1..%d) n_planes=%d (1..%d)", D, GRAM_TILE,
                    COPO_PROBE_MAX_WIDTH, n_blocks, COPO_PROBE_MAX_BLOCKS, n_planes, COPO_CKA_MAX_PLANES);
    if (cap < 1 || cap > INT32_MAX || n_out < 1 || slots < 1 || n_out % slots != 0 || pos_stride < D || pos_stride % 4 != 0 || x_floats < 1 ||
        pos_stride > x_floats / cap)
        return fail(COPO_ERR_DIM, "copo_probe_accumulate: cap=%lld (1..2^31-1) n_out=%lld slots=%d (n_out a multiple of it) pos_stride=%lld (a multiple of 4, "
                    "from the width up, cap positions inside x_floats=%lld)", (long long)cap, (long long)n_out, slots, (long long)pos_stride, (long long)x_floats);
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0 || ((reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(C) | reinterpret_cast<uintptr_t>(T)) & 7) != 0)
        return fail(COPO_ERR_DIM, "copo_probe_accumulate: x must be 16-byte aligned (it is read in 128-bit words), the accumulators 8-byte aligned");
    const ProbeArgs a{x, block_base, targets, rows, count, flags, seat, fold, x_floats, pos_stride, cap, n_out, n_blocks, D, slots, rows_of < 0 ? -1 : rows_of,
                      n_planes, G, C, T};
    HIP_TRY(launch_probe_accumulate(a, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}
