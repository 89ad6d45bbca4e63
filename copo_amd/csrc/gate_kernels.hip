// Traffic gates over the simulator's scenes (copo_gate_*, include/copo_hip.h): how much traffic gets through, and how fast.  A gate is a
// directed line segment; every record decides for every slot whether the same agent moved across each gate since the previous record
// and adds the crossings, their speeds, the headways between them and the travel times between an entry and an exit gate into int64
// accumulators per scene group.  Integer accumulators only, so no sum depends on the order the workgroups run in.  One launch per record:
//   one wave per scene, four scenes per 256-thread workgroup, lane n = slot n (every load and store over the slots is coalesced); a
//   workgroup walks the scenes in strides of the grid (at most GATE_MAX_WG workgroups), with the gate and section tables staged into LDS
//   once.  Per gate the wave decides by ballot + popcount: the counts of a (scene, gate, direction) that has crossings go out as ONE 64-bit
//   integer atomic each, the speed sum is reduced over the wave first, and the headway rule falls out of the ballot (the lowest set
//   lane takes r - last_fwd, bin 0 gets popcount - 1).  last_fwd, the entry records and the per-slot memory belong to the scene's wave:
//   no atomic touches them and nothing depends on scheduling.  What EVERY scene adds in every record (scene_records, alive) is summed
//   over the workgroup's scenes in LDS and leaves as one atomic per group and workgroup; crossings are rare and go straight to memory.
// All geometry is fp32 with every operation rounded by itself (the library is built with -ffp-contract=off), comparisons are plain, so
// a NaN never crosses.  The rules are restated in numpy by tests/gate_numpy.py.
#include "sim_device.h"
#include "gate_common.h"

namespace copo {

namespace {

constexpr int GB = 256, NW = GB / 64;
constexpr int GATE_MAX_WG = 1024;          // four workgroups per CU: beyond that a workgroup takes several batches of scenes

typedef unsigned long long u64;

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

}  // namespace

__global__ __launch_bounds__(GB) void gate_record_kernel(GateArgs a) {
    __shared__ float4 sgate[GATE_MAX_GATES];
    __shared__ int2 ssec[GATE_MAX_SECTIONS];
    __shared__ uint32_t s_rec[GATE_MAX_GROUPS], s_alive[GATE_MAX_GROUPS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < a.L) sgate[tid] = a.gates[tid];
    if (tid < a.S) ssec[tid] = a.sections[tid];
    if (tid < GATE_MAX_GROUPS) {
        s_rec[tid] = 0u;
        s_alive[tid] = 0u;
    }
    __syncthreads();
    const int N = a.N, L = a.L, S = a.S, r = a.r;
    const size_t EN = (size_t)a.E * N;
    u64* A = reinterpret_cast<u64*>(a.acc);
    for (int e = blockIdx.x * NW + wave; e < a.E; e += gridDim.x * NW) {      // (the whole wave)
        const size_t o = (size_t)e * N + lane;
        const bool in = lane < N;
        uint32_t xb = 0u, yb = 0u, pxb = 0u, pyb = 0u;
        int32_t aid = 0, paid = 0;
        int st = ST_EMPTY;
        float v = 0.0f;
        if (in) {
            const uint32_t* su = reinterpret_cast<const uint32_t*>(a.state);
            xb = su[o]; yb = (su + EN)[o]; v = (a.state + 3 * EN)[o];
            st = st_status((int32_t)(su + 13 * EN)[o]);
            aid = (int32_t)(su + 14 * EN)[o];
            pxb = a.mem_x[o]; pyb = a.mem_y[o]; paid = a.mem_aid[o];
        }
        const int32_t ep = a.env[(size_t)e * 4 + 1], pep = a.mem_episode[e];
        const u64 valid = a.mem_valid[e];
        const int g = SceneGroups{a.group, a.G}.of(e);
        const bool routed = g >= 0;
        const bool alive = in && st == ST_ALIVE;
        const bool followed = alive && ((valid >> lane) & 1ull) && paid == aid && pep == ep;
        const float cx = __uint_as_float(xb), cy = __uint_as_float(yb), px = __uint_as_float(pxb), py = __uint_as_float(pyb);
        const float mx = cx - px, my = cy - py;
        const int spq = __float2int_rn(fminf(fmaxf(v, 0.0f), 255.0f) * 256.0f);
        uint32_t fwd_gates = 0u;                                               // the gates this lane crossed forward
        for (int l = 0; l < L; ++l) {
            const float4 q = sgate[l];
            const float dx = q.z - q.x, dy = q.w - q.y;
            const float sp = dx * (py - q.y) - dy * (px - q.x), sc = dx * (cy - q.y) - dy * (cx - q.x);
            const float ea = mx * (q.y - py) - my * (q.x - px), eb = mx * (q.w - py) - my * (q.z - px);
            const bool within = followed && ((ea <= 0.0f && eb >= 0.0f) || (ea >= 0.0f && eb <= 0.0f));
            const bool f = within && sp < 0.0f && sc >= 0.0f, b = within && sp >= 0.0f && sc < 0.0f;
            const u64 mf = __ballot(f), mb = __ballot(b);
            if (!(mf | mb)) continue;                                          // (uniform over the wave)
            fwd_gates |= f ? 1u << l : 0u;
#pragma unroll
            for (int dir = 0; dir < 2; ++dir) {
                const u64 m = dir ? mb : mf;
                if (!m) continue;
                const long long sum = wave_sum((dir ? b : f) ? (long long)spq : 0ll);
                if (lane == 0 && routed) {
                    const size_t i = ((size_t)g * L + l) * 2 + dir;
                    const u64 n = (u64)__popcll(m);
                    atomicAdd(A + a.at.count + i, n);
                    if (sum) atomicAdd(A + a.at.speed_q + i, (u64)sum);
                    atomicAdd(A + a.at.series + i * a.T + a.tbin, n);
                }
            }
            if (mf && lane == 0) {
                int32_t* lf = a.last_fwd + (size_t)e * L + l;
                const int was = *lf;
                if (routed) {
                    u64* H = A + a.at.headway + ((size_t)g * L + l) * a.HB;
                    const int n = __popcll(mf);
                    if (was >= 0) atomicAdd(H + min(max(r - was, 0), a.HB - 1), 1ull);
                    if (n > 1) atomicAdd(H, (u64)(n - 1));
                }
                *lf = r;
            }
        }
        for (int s = 0; s < S; ++s) {
            const int2 io = ssec[s];
            int32_t* P = a.entry + ((size_t)e * S + s) * N + lane;
            int old = -1, ent = -1;
            if (in) {
                old = *P;
                ent = followed ? old : -1;
            }
            if ((fwd_gates >> io.x) & 1u) ent = r;
            const bool done = ((fwd_gates >> io.y) & 1u) && ent >= 0;
            const int tt = done ? max(r - ent, 0) : 0;
            if (done) ent = -1;
            if (in && ent != old) *P = ent;
            const u64 mc = __ballot(done);
            if (!mc) continue;
            const long long sum = wave_sum((long long)tt);
            if (routed) {
                const size_t i = (size_t)g * S + s;
                if (lane == 0) {
                    atomicAdd(A + a.at.sec_count + i, (u64)__popcll(mc));
                    if (sum) atomicAdd(A + a.at.sec_sum + i, (u64)sum);
                }
                if (done) atomicAdd(A + a.at.sec_hist + i * a.TB + min(tt / a.tt_bin, a.TB - 1), 1ull);
            }
        }
        // the memory of the next record
        if (in) {
            a.mem_x[o] = xb; a.mem_y[o] = yb; a.mem_aid[o] = aid;
        }
        const u64 ma = __ballot(alive);
        if (lane == 0) {
            a.mem_valid[e] = ma;
            a.mem_episode[e] = ep;
            if (routed) {
                atomicAdd(&s_rec[g], 1u);
                atomicAdd(&s_alive[g], (uint32_t)__popcll(ma));
            }
        }
    }
    __syncthreads();
    if (tid < a.G) {
        if (s_rec[tid]) atomicAdd(A + a.at.scene_records + tid, (u64)s_rec[tid]);
        if (s_alive[tid]) atomicAdd(A + a.at.alive + tid, (u64)s_alive[tid]);
    }
}

hipError_t launch_gate_record(const GateArgs& a, hipStream_t stream) {
    const int batches = (a.E + NW - 1) / NW;
    hipLaunchKernelGGL(gate_record_kernel, dim3(batches < GATE_MAX_WG ? batches : GATE_MAX_WG), dim3(GB), 0, stream, a);
    return hipGetLastError();
}

}  // namespace copo
