// C ABI of the critic audit (include/copo_hip.h, copo_audit_*; kernel: audit_kernels.hip).  Like the device recorder it observes no
// simulator: it consumes the sampler's tensors, lives on the device that is current at create and owns its buffers through a DevPool
// (capi_common.h).  All launches are asynchronous on the caller's stream.
#include <cmath>
#include <new>

#include "capi_common.h"
#include "audit_common.h"

using namespace copo;

struct copo_audit {
    DevPool mem;
    copo_audit_cfg cfg;
    DevBuf<double> state;        // [planes][E N heads]
    DevBuf<long long> acc;       // [G][K][heads][AUDIT_WORDS]
};

static int null_handle(const char* who) { return fail(COPO_ERR_NULL, "%s: NULL handle", who); }

extern "C" int copo_audit_create(const copo_audit_cfg* cfg, copo_audit** out) {
    if (!out || !cfg) return fail(COPO_ERR_NULL, "copo_audit_create: NULL argument");
    *out = nullptr;
    const copo_audit_cfg& c = *cfg;
    if (c.E < 1 || c.N < 1 || c.K < 1 || c.K > 65535 || c.G < 1 || c.heads < 1 || c.heads > 3 || c.bins < 1 || c.bins > AUDIT_MAX_BINS)
        return fail(COPO_ERR_DIM, "copo_audit_create: E=%d N=%d G=%d (>= 1) K=%d (1..65535) heads=%d (1..3) bins=%d (1..%d)", c.E, c.N, c.G, c.K,
                    c.heads, c.bins, AUDIT_MAX_BINS);
    for (int h = 0; h < c.heads; ++h)
        if (!(c.gamma[h] >= 0.0 && c.gamma[h] <= 1.0) || !std::isfinite(c.lo[h]) || !std::isfinite(c.hi[h]) || !(c.lo[h] < c.hi[h]))
            return fail(COPO_ERR_CONFIG, "copo_audit_create: head %d: gamma=%g (0..1) value range [%g, %g] (finite, lo < hi)", h, c.gamma[h], c.lo[h],
                        c.hi[h]);
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    copo_audit* h = new (std::nothrow) copo_audit();
    if (!h) return fail(COPO_ERR_DEVICE, "out of host memory");
    h->mem.device = device;
    h->cfg = c;
    h->state = h->mem.alloc<double>((size_t)audit_state_planes(c.bins) * c.E * c.N * c.heads);
    h->acc = h->mem.alloc<long long>((size_t)c.G * c.K * c.heads * AUDIT_WORDS);
    return finish_create(h, out, "copo_audit_create");
}

extern "C" int copo_audit_destroy(copo_audit* h) { return destroy_handle(h, "copo_audit_destroy"); }

extern "C" int copo_audit_record(copo_audit* h, const uint8_t* flags, const float* values, const float* rew, const float* nei_rew,
                                 const float* glob_rew, const int32_t* seat, const int32_t* group, void* stream) {
    if (!h) return null_handle("copo_audit_record");
    const copo_audit_cfg& c = h->cfg;
    if (!flags || !values || !rew || !seat || !group || (c.heads > 1 && !nei_rew) || (c.heads > 2 && !glob_rew))
        return fail(COPO_ERR_NULL, "copo_audit_record: NULL argument (flags, values, rew, seat, group; nei_rew with 2 heads, glob_rew with 3)");
    AuditArgs a{};
    a.flags = flags; a.values = values; a.rew[0] = rew; a.rew[1] = nei_rew; a.glob_rew = glob_rew; a.seat = seat; a.group = group;
    a.E = c.E; a.N = c.N; a.K = c.K; a.G = c.G; a.heads = c.heads; a.bins = c.bins; a.count_truncated = c.count_truncated != 0;
    for (int k = 0; k < 3; ++k) { a.gamma[k] = c.gamma[k]; a.lo[k] = c.lo[k]; a.hi[k] = c.hi[k]; }
    a.state = h->state;
    a.acc = reinterpret_cast<int64_t*>(h->acc.p);
    HIP_TRY(launch_audit_record(a, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_audit_read(copo_audit* h, int64_t* acc_out, void* stream) {
    if (!h) return null_handle("copo_audit_read");
    if (!acc_out) return fail(COPO_ERR_NULL, "copo_audit_read: NULL output");
    HIP_TRY(h->acc.copy_to(acc_out, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_audit_reset(copo_audit* h, void* stream) {
    if (!h) return null_handle("copo_audit_reset");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(h->state.fill(0, st));
    HIP_TRY(h->acc.fill(0, st));
    return COPO_OK;
}
