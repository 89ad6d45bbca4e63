// C entry points of representation similarity (include/copo_hip.h): argument checks in front of the launchers of
// cka_kernels.hip.
#include "capi_common.h"
#include "cka_common.h"

using namespace copo;

// what both entries ask of the accumulators' geometry; the message names the entry point
static int cka_check(const char* who, int32_t n_panel, int32_t H, int32_t n_planes) {
    if (n_panel < 1 || n_panel > COPO_CKA_MAX_PANEL || H < GRAM_TILE || H > COPO_CKA_MAX_HIDDEN || H % GRAM_TILE != 0 || n_planes < 1 ||
        n_planes > COPO_CKA_MAX_PLANES)
        return fail(COPO_ERR_DIM, "%s: n_panel=%d (1..%d) hidden=%d (a multiple of %d up to %d) n_planes=%d (1..%d)", who, n_panel, COPO_CKA_MAX_PANEL,
                    H, GRAM_TILE, COPO_CKA_MAX_HIDDEN, n_planes, COPO_CKA_MAX_PLANES);
    return COPO_OK;
}

extern "C" int copo_cka_accumulate(const float* hidden, int32_t n_members, int64_t cap, int32_t H, const int32_t* panel, int32_t n_panel,
                                   const int64_t* rows, const int32_t* count, const uint8_t* flags, const int32_t* seat, int64_t n_out,
                                   int32_t rows_of, int32_t n_planes, double* S, double* s, int64_t* n, void* stream) {
    if (!hidden || !panel || !rows || !count || !flags || !seat || !S || !s || !n) return fail(COPO_ERR_NULL, "copo_cka_accumulate: NULL argument");
    if (const int rc = cka_check("copo_cka_accumulate", n_panel, H, n_planes)) return rc;
    if (n_members < 1 || n_members > 65535 || cap < 1 || n_out < 1 || rows_of >= n_members)
        return fail(COPO_ERR_DIM, "copo_cka_accumulate: n_members=%d (1..65535) cap=%lld n_out=%lld (>= 1) rows_of=%d (negative, or a member)", n_members,
                    (long long)cap, (long long)n_out, rows_of);
    if ((reinterpret_cast<uintptr_t>(hidden) & 15) != 0 || ((reinterpret_cast<uintptr_t>(S) | reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(n)) & 7) != 0)
        return fail(COPO_ERR_DIM, "copo_cka_accumulate: hidden must be 16-byte aligned (it is read in 128-bit words), the accumulators 8-byte aligned");
    const CkaArgs a{hidden, panel, rows, count, flags, seat, cap, n_out, H, n_panel, rows_of < 0 ? -1 : rows_of, n_planes, n_members, S, s, n};
    HIP_TRY(launch_cka_accumulate(a, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}

extern "C" int copo_cka_finish(const double* S, const double* s, const int64_t* n, int32_t n_panel, int32_t H, int32_t n_planes, double* hsic,
                               int64_t* n_out, double* mean, double* var, void* stream) {
    if (!S || !s || !n || !hsic || !n_out || !mean || !var) return fail(COPO_ERR_NULL, "copo_cka_finish: NULL argument");
    if (const int rc = cka_check("copo_cka_finish", n_panel, H, n_planes)) return rc;
    HIP_TRY(launch_cka_finish(S, s, n, n_panel, H, n_planes, hsic, n_out, mean, var, static_cast<hipStream_t>(stream)));
    return COPO_OK;
}
