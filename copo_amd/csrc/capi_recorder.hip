// C ABI of the device evaluation recorder (include/copo_hip.h, copo_recorder_*; kernels: recorder_kernels.hip).  Unlike the handles of
// capi_observers.hip it observes no simulator: it consumes the sampler's tensors, so it lives on the device that is current at create
// and owns its buffers through a DevPool (capi_common.h).  All launches are asynchronous on the caller's stream.
#include <new>

#include "capi_common.h"
#include "recorder_common.h"

using namespace copo;

struct copo_recorder {
    DevPool mem;
    int32_t E, N, max_rows, limit;
    DevBuf<double> acc;                    // [E][REC_ACC]
    DevBuf<double> slots;                  // [REC_SLOT_PLANES][E][N]
    DevBuf<long long> episodes;            // [E]
    DevBuf<int32_t> n_rows, base;          // [E]
    DevBuf<long long> counters;            // [ROWLOG_COUNTERS]
    DevBuf<double> rows;                   // [max_rows][REC_NCOL]
};

static int null_handle(const char* who) { return fail(COPO_ERR_NULL, "%s: NULL handle", who); }

extern "C" int copo_recorder_create(int32_t E, int32_t N, int32_t max_rows, int32_t limit, copo_recorder** out) {
    if (!out) return fail(COPO_ERR_NULL, "copo_recorder_create: NULL argument");
    *out = nullptr;
    static_assert(COPO_RECORDER_NCOL == REC_NCOL && COPO_RECORDER_MAX_SLOTS == REC_MAX_SLOTS, "copo_hip.h / recorder_common.h");
    if (E < 1 || N < 1 || N > REC_MAX_SLOTS || max_rows < 1 || limit < 0)
        return fail(COPO_ERR_DIM, "copo_recorder_create: E=%d (>= 1) N=%d (1..%d) max_rows=%d (>= 1) limit=%d (>= 0)", E, N, REC_MAX_SLOTS,
                    max_rows, limit);
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    copo_recorder* h = new (std::nothrow) copo_recorder();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->mem.device = device; h->E = E; h->N = N; h->max_rows = max_rows; h->limit = limit;
    const size_t scenes = (size_t)E;
    h->acc = h->mem.alloc<double>(scenes * REC_ACC);
    h->slots = h->mem.alloc<double>((size_t)REC_SLOT_PLANES * scenes * N);
    h->episodes = h->mem.alloc<long long>(scenes);
    h->n_rows = h->mem.alloc<int32_t>(scenes);
    h->base = h->mem.alloc<int32_t>(scenes);
    h->counters = h->mem.alloc<long long>(ROWLOG_COUNTERS);
    h->rows = h->mem.alloc<double>((size_t)max_rows * REC_NCOL);
    if (h->mem.err == hipSuccess) h->mem.err = launch_recorder_arm(h->acc, E, nullptr);
    return finish_create(h, out, "copo_recorder_create");
}

extern "C" int copo_recorder_destroy(copo_recorder* h) { return destroy_handle(h, "copo_recorder_destroy"); }

extern "C" int copo_recorder_add(copo_recorder* h, const uint8_t* flags, const float* infos, const float* rewards, const float* nei_rewards,
                                 const int32_t* nbr_cnt, int32_t T, void* stream) {
    if (!h) return null_handle("copo_recorder_add");
    if (!flags || !infos || !rewards || !nei_rewards || !nbr_cnt) return fail(COPO_ERR_NULL, "copo_recorder_add: NULL argument");
    if (T < 1) return fail(COPO_ERR_DIM, "copo_recorder_add: T=%d (>= 1)", T);
    if (reinterpret_cast<uintptr_t>(infos) % 16 != 0) return fail(COPO_ERR_CONFIG, "copo_recorder_add: infos is not 16-byte aligned");
    RecorderArgs a;
    a.flags = flags; a.infos = infos; a.rew = rewards; a.nei_rew = nei_rewards; a.nbr_cnt = nbr_cnt;
    a.T = T; a.E = h->E; a.N = h->N; a.limit = h->limit;
    a.acc = h->acc; a.slots = h->slots; a.episodes = h->episodes; a.n_rows = h->n_rows;
    a.ids = RowPoolArgs{h->max_rows, h->base, h->counters, nullptr};
    a.rows = h->rows;
    HIP_TRY(launch_recorder_add(a, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_recorder_count(copo_recorder* h, int64_t* out, void* stream) {
    if (!h || !out) return fail(COPO_ERR_NULL, "copo_recorder_count: NULL argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long c[ROWLOG_COUNTERS];
    HIP_TRY(hipMemcpyAsync(c, h->counters, sizeof(c), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out[0] = c[RL_ROWS];
    out[1] = c[RL_DROPPED];
    return COPO_OK;
}

extern "C" int copo_recorder_read(copo_recorder* h, int32_t first, int32_t n, double* rows_out, void* stream) {
    if (!h) return null_handle("copo_recorder_read");
    if (first < 0 || n < 0 || (int64_t)first + n > h->max_rows)
        return fail(COPO_ERR_DIM, "copo_recorder_read: rows [%d, %d + %d) of a pool of %d", first, first, n, h->max_rows);
    if (n == 0) return COPO_OK;
    if (!rows_out) return fail(COPO_ERR_NULL, "copo_recorder_read: NULL output");
    HIP_TRY(hipMemcpyAsync(rows_out, h->rows.p + (size_t)first * REC_NCOL, (size_t)n * REC_NCOL * sizeof(double), hipMemcpyDeviceToDevice,
                           static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_recorder_episodes(copo_recorder* h, int64_t* episodes_dev, void* stream) {
    if (!h || !episodes_dev) return fail(COPO_ERR_NULL, "copo_recorder_episodes: NULL argument");
    HIP_TRY(h->episodes.copy_to(episodes_dev, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

// (the rows need no clearing: nothing reads beyond the stored count)
extern "C" int copo_recorder_clear(copo_recorder* h, void* stream) {
    if (!h) return null_handle("copo_recorder_clear");
    HIP_TRY(h->counters.fill(0, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_recorder_reset(copo_recorder* h, void* stream) {
    if (!h) return null_handle("copo_recorder_reset");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(h->counters.fill(0, st));
    HIP_TRY(h->rows.fill(0, st));
    HIP_TRY(h->slots.fill(0, st));
    HIP_TRY(h->episodes.fill(0, st));
    HIP_TRY(launch_recorder_arm(h->acc, h->E, st));
    return COPO_OK;
}
