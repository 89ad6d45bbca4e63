// The row pool under the trip log and the conflict log (trip_kernels.hip, conflict_kernels.hip, capi_observers.hip): a bounded pool of
// 64-byte rows that the device fills in an order that does not depend on scheduling.  A record is three launches:
//   close:   the log's own kernel decides what closes and leaves a count of closes per scene
//   assign:  ONE workgroup walks the scenes in order, a prefix over lanes and waves: every scene gets the row id of its first close,
//            ids from max_rows on are clamped to max_rows, then the counters {rows, dropped} move.  No atomic decides an id, so which rows
//            exist, their order and which are dropped do not depend on how workgroups are scheduled (the clip recorder's rule)
//   commit:  the log's own kernel gives the closes of a scene the ids base, base + 1, ... in its own order and writes the rows below
//            max_rows as four 16-byte stores
// The library is built without relocatable device code, so the device part is inline / template code.  DESIGN.md section 8g.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace copo {

constexpr int ROWLOG_WORDS = 16;           // 32-bit words of a row
enum { RL_ROWS = 0, RL_DROPPED, ROWLOG_COUNTERS };

// The pool's part of a log's arguments.  Device pointers.
struct RowPoolArgs {
    int32_t max_rows;              // pool size
    int32_t* base;                 // [E] row id of the scene's first close, min(id, max_rows); between the launches of one call
    long long* counters;           // [ROWLOG_COUNTERS]
    uint32_t* pool;                // [max_rows][ROWLOG_WORDS]
};

#ifdef __HIPCC__
namespace rowlog {

constexpr int TB = 256, NW = TB / 64;      // close and commit: one wave per scene, four scenes per workgroup
constexpr int MAX_WG = 1024;               // four workgroups per CU: beyond that a workgroup takes several batches of scenes
constexpr int ASSIGN_THREADS = 1024, ASSIGN_WAVES = ASSIGN_THREADS / 64;

typedef unsigned long long u64;

// The body of a log's assign kernel (ONE workgroup of ASSIGN_THREADS): the row ids of the closes in ascending scene order, then the
// counters.  closes(e): the closes of scene e in this call.
template <typename Closes>
__device__ __forceinline__ void assign(const RowPoolArgs& p, int E, Closes closes) {
    __shared__ int wsum[ASSIGN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long first = p.counters[RL_ROWS];      // (read by every thread before the first barrier, written after the last)
    long long total = 0;
    for (int e0 = 0; e0 < E; e0 += ASSIGN_THREADS) {
        const int e = e0 + tid;
        const int c = e < E ? closes(e) : 0;
        int inc = c;                                   // inclusive prefix over the wave's lanes (at most 64 x 2 016)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int off = 0, sum = 0;
#pragma unroll
        for (int w = 0; w < ASSIGN_WAVES; ++w) {
            const int s = wsum[w];
            off += w < wave ? s : 0;
            sum += s;
        }
        if (e < E) {
            const long long id = first + total + off + (inc - c);
            p.base[e] = (int32_t)(id < p.max_rows ? id : p.max_rows);       // (every id from max_rows on is dropped alike)
        }
        total += sum;
        __syncthreads();
    }
    if (tid == 0) {
        const long long stored = first + total < p.max_rows ? first + total : p.max_rows;
        p.counters[RL_ROWS] = stored;
        p.counters[RL_DROPPED] += first + total - stored;
    }
}

// Whether the pool stores row `id`, and then R = its four 16-byte words; an id from max_rows on is dropped.
__device__ __forceinline__ bool row(const RowPoolArgs& p, long long id, uint4*& R) {
    if (id >= p.max_rows) return false;
    R = reinterpret_cast<uint4*>(p.pool) + (size_t)id * (ROWLOG_WORDS / 4);
    return true;
}

inline dim3 scene_grid(int E) {
    const int batches = (E + NW - 1) / NW;
    return dim3(batches < MAX_WG ? batches : MAX_WG);
}

// The three launches of one call of a log with arguments A
template <typename A>
hipError_t launch(void (*close)(A, int), void (*assign_ids)(A), void (*commit)(A, int), const A& a, int flush, hipStream_t stream) {
    hipLaunchKernelGGL(close, scene_grid(a.E), dim3(TB), 0, stream, a, flush);
    hipLaunchKernelGGL(assign_ids, dim3(1), dim3(ASSIGN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(commit, scene_grid(a.E), dim3(TB), 0, stream, a, flush);
    return hipGetLastError();
}

}  // namespace rowlog
#endif

}  // namespace copo
