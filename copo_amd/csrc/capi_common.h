// Shared by the units of the C ABI (capi.hip, capi_observers.hip): error reporting, the simulator handle and the ownership of
// device buffers.  Host only; not part of the installed interface (include/copo_hip.h).
#pragma once
#include <cstddef>
#include <vector>

#include "sim_common.h"

namespace copo {

// Sets the calling thread's error string (copo_last_error) and returns `code`.  Defined once, in capi.hip, next to the buffer.
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess) return ::copo::fail(COPO_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// What the four tally entries (copo_seat_tally, copo_certify_tally, copo_jury_tally, copo_influence_tally) share: the ranges of the walk
// (seat_common.h).  A refusal is COPO_ERR_DIM in the entry point's name; E == 0 is accepted (the entry returns before its launch).
inline int check_tally(const char* name, int32_t E, int32_t N, int32_t K, int32_t G) {
    if (E < 0 || N < 1 || N > COPO_SEAT_MAX_SLOTS || K < 1 || K > 65535 || G < 1)
        return fail(COPO_ERR_DIM, "%s: E=%d N=%d (1..%d) K=%d (1..65535) G=%d (>= 1)", name, E, N, COPO_SEAT_MAX_SLOTS, K, G);
    return COPO_OK;
}

// A device buffer and its size: clears and whole-buffer copies take the byte count from here.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t bytes = 0;
    operator T*() const { return p; }
    hipError_t fill(int byte, hipStream_t st) const { return hipMemsetAsync(p, byte, bytes, st); }
    hipError_t copy_to(void* dst, hipStream_t st) const { return hipMemcpyAsync(dst, p, bytes, hipMemcpyDeviceToDevice, st); }
    hipError_t copy_from(const void* src, hipStream_t st) const { return hipMemcpyAsync(p, src, bytes, hipMemcpyDeviceToDevice, st); }
};

// Owner of a handle's device buffers.  The first failure is kept and every later request is a no-op, so a create is a straight list
// of requests followed by one `check`.  A count of 0 allocates one element.
struct DevPool {
    int device = 0;
    hipError_t err = hipSuccess;
    size_t requested = 0;          // bytes asked for so far (the error string names it)
    std::vector<void*> allocs;

    // `count` elements, every byte set to `byte`
    template <typename T>
    DevBuf<T> alloc(size_t count, int byte = 0) {
        DevBuf<T> b;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        void* d = nullptr;
        requested += bytes;
        if (err != hipSuccess) return b;
        err = hipMalloc(&d, bytes);
        if (err != hipSuccess) {
            (void)hipGetLastError();           // (a refused request must not show up as the next launch's error)
            return b;
        }
        allocs.push_back(d);
        err = hipMemset(d, byte, bytes);
        b.p = static_cast<T*>(d);
        b.bytes = bytes;
        return b;
    }

    // a copy of the host table `host[count]`
    template <typename T>
    DevBuf<T> upload(const T* host, size_t count) {
        DevBuf<T> b = alloc<T>(count);
        if (err == hipSuccess && count) err = hipMemcpy(b.p, host, count * sizeof(T), hipMemcpyHostToDevice);
        return b;
    }

    // COPO_OK once every request and its fill is done, else COPO_ERR_DEVICE with the first failure in `who`'s name
    int check(const char* who) {
        if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
        if (err == hipSuccess) return COPO_OK;
        (void)hipGetLastError();
        return fail(COPO_ERR_DEVICE, "%s: %s (%zu bytes of device memory requested)", who, hipGetErrorString(err), requested);
    }

    void release() {
        (void)hipSetDevice(device);
        for (void* a : allocs) (void)hipFree(a);
        allocs.clear();
    }
};

// The end of every *_create: hand the handle out, or leave nothing behind.  H has a `DevPool mem`.
template <typename H>
int finish_create(H* h, H** out, const char* who) {
    const int rc = h->mem.check(who);
    if (rc != COPO_OK) {
        h->mem.release();
        delete h;
        return rc;
    }
    *out = h;
    return COPO_OK;
}

// Every *_destroy.  It reads nothing but the handle itself: an observer may be destroyed after its simulator.
template <typename H>
int destroy_handle(H* h, const char* who) {
    if (!h) return fail(COPO_ERR_NULL, "%s: NULL handle", who);
    h->mem.release();
    delete h;
    return COPO_OK;
}

}  // namespace copo

struct copo_sim {
    copo::SimParams p;
    copo::SimParams* p_dev;    // device copy of p (the kernels' parameter block)
    int device;
    int block;
    bool started;
    double lcf_mean, lcf_std, force_lcf;
    int capacity;              // active agent slots (curriculum), num_agents by default
    float lcf_host[4];         // {mean, std, capacity, 0}: the first words of p.lcf_dist (the kernels read the capacity there)
    bool lcf_dirty;
    // The kernels draw scene e's LCF from row e of [E][2] {mean, std} at p.lcf_dist + 4, always: `lcf_rows` is the host image of those
    // rows -- `lcf_table` (copo_sim_set_lcf_table) while lcf_table_on and no LCF is forced, else the single pair in every row --
    // rebuilt and pushed when lcf_rows_dirty.  Both are sized once at create.
    std::vector<float> lcf_table, lcf_rows;
    bool lcf_table_on, lcf_rows_dirty;
    copo::DevPool mem;
    // host copies of the map tables for copo_render_create: road records [n_routes][seg_rows][COPO_SEG_STRIDE], route_meta,
    // lane lines (on the device only when a detector reads them) and static boxes
    std::vector<float> h_segs, h_meta, h_lines, h_boxes;
    bool boxes_hidden;
};
