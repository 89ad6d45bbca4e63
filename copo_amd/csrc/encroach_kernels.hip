// Encroachment log over the simulator's scenes (copo_pet_*, include/copo_hip.h): post-encroachment times from a grid of stamps per scene;
// no counterpart in the reference.  Every cell of a scene's grid holds one 64-bit stamp: which driving agent's footprint covered it last,
// and in which record.  The first record in which agent b touches valid stamps of agent a leaves ONE 64-byte row -- the encounter's PET --
// in a bounded pool and adds to integer aggregates per scene group.  Four launches per record; the pool, the assign launch and the rule
// that decides the row ids are rowlog_common.h:
//   scan:    one wave per scene, four scenes per 256-thread workgroup, lane n = slot n; at most MAX_WG workgroups, beyond that a
//            workgroup walks its scenes in strides of the grid.  Slot turnover and the episode word first (the `met` masks, the
//            remembered ids, the scene's epoch); one word per slot (ALIVE, low id bits) is staged into LDS; then every ALIVE lane walks
//            the cells of its footprint, collects the slots with a valid stamp under it and leaves its mask of new partners and the
//            scene's count
//   assign:  a scene's rows are that count: every scene gets the row id of its first new encounter
//   commit:  wave per scene again over the still unchanged grid: a lane's first id is the scene's base + the popcounts of the masks of the
//            lanes below it; for every new partner it walks its footprint once more for the smallest PET, the lowest cell that attains
//            it and the number of cells, writes the row as four 16-byte stores and adds to the histogram and the critical map (64-bit
//            integer atomic adds: the sums do not depend on the order)
//   stamp:   every ALIVE slot writes max(old, its stamp of this record) into the cells of its footprint, a 64-bit atomic max: a later
//            record always wins, and two bodies over one cell centre in one record resolve by the word's value, not by timing
// Reads and writes of the grid are in different launches, so no read of a record sees a stamp of that record.  The footprint is `covers`
// of grid_common.h, the one the field maps count with; everything else is integer logic and one fp32 product (the heading's
// quantisation), so the numpy restatement (tests/pet_numpy.py) gives the same bits.  The rules are DESIGN.md section 8i.
#include "sim_device.h"
#include "encroach_common.h"

namespace copo {

using namespace rowlog;

namespace {

constexpr uint32_t SW_ALIVE = 1u << 16;        // above the 16 id bits of a slot word

// a body and the cells [lox, hix] x [loy, hiy] its footprint can reach (hix < lox: none)
struct Body {
    float x, y, cs, sn;
    int lox, hix, loy, hiy;
};

__device__ __forceinline__ Body body_of(const PetArgs& a, size_t o, size_t EN) {
    Body b;
    b.x = a.state[o]; b.y = (a.state + EN)[o]; b.cs = 1.0f; b.sn = 0.0f;
    if (a.grid.reach_box(b.x, b.y, a.hl, a.hw, b.lox, b.hix, b.loy, b.hiy)) sincos_det((a.state + 2 * EN)[o], b.sn, b.cs);
    else { b.lox = b.loy = 0; b.hix = b.hiy = -1; }
    return b;
}

// f(iy * W + ix) for every cell whose centre lies in the body, in ascending cell order
template <typename F>
__device__ __forceinline__ void for_cells(const PetArgs& a, const Body& b, F f) {
    for (int iy = b.loy; iy <= b.hiy; ++iy) {
        const float dy = a.grid.centre_y(iy) - b.y;
        for (int ix = b.lox; ix <= b.hix; ++ix)
            if (covers(a.grid.centre_x(ix) - b.x, dy, b.cs, b.sn, a.hl, a.hw)) f(iy * a.grid.W + ix);
    }
}

__device__ __forceinline__ uint32_t heading_q(float th) { return (uint32_t)__float2int_rn(th * (float)(128.0 / 3.14159265358979323846)) & 255u; }

__device__ __forceinline__ uint32_t slot_word(const PetArgs& a, size_t o, size_t EN, bool in, bool& alive, int32_t& aid) {
    const int32_t* si = reinterpret_cast<const int32_t*>(a.state);
    alive = in && st_status((si + 13 * EN)[o]) == ST_ALIVE;
    aid = in ? (si + 14 * EN)[o] : 0;
    return alive ? SW_ALIVE | ((uint32_t)aid & 0xffffu) : 0u;
}

// The PET in records of stamp `s` under the footprint of ALIVE slot n in record a.r, 0 when the stamp is not valid for it.  sw: the
// scene's slot words.
__device__ __forceinline__ int valid_pet(const PetArgs& a, u64 s, int n, int32_t epoch, const uint32_t* sw) {
    const uint32_t lo = (uint32_t)s, q = (uint32_t)(s >> 32);
    const int slot = (int)(lo & 63u);
    if (q == 0u || slot == n) return 0;
    if (sw[slot] != (SW_ALIVE | (lo >> 16))) return 0;        // the earlier agent is still driving
    if ((long long)q <= (long long)epoch) return 0;
    const long long d = (long long)a.r - ((long long)q - 1);
    return d >= 1 && d <= (long long)a.window ? (int)d : 0;
}

}  // namespace

__global__ __launch_bounds__(TB) void pet_scan_kernel(PetArgs a) {
    __shared__ uint32_t sw[NW][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N;
    const size_t EN = (size_t)a.E * N, HW = (size_t)a.grid.H * a.grid.W;
    for (int e0 = blockIdx.x * NW; e0 < a.E; e0 += gridDim.x * NW) {           // (the whole workgroup: the barriers below)
        const int e = e0 + wave;
        const bool in = e < a.E && lane < N;
        const size_t o = (size_t)(e < a.E ? e : 0) * N + (lane < N ? lane : 0);
        bool alive = false;
        int32_t aid = 0, aid_mem = 0, ep = 0, ep_mem = 0, epoch = 0;
        u64 met_mem = 0ull;
        if (e < a.E) {
            ep = a.env[(size_t)e * 4 + 1];
            ep_mem = a.episode[e];
            epoch = a.epoch[e];
            if (in) {
                aid_mem = a.aid[o];
                met_mem = a.met[o];
            }
        }
        sw[wave][lane] = slot_word(a, o, EN, in, alive, aid);
        const bool changed = ep != ep_mem;
        if (changed) epoch = a.r;
        const bool turn = in && (!alive || aid != aid_mem || changed);
        const u64 turned = __ballot(turn);                                      // (the whole wave)
        u64 met = (turn ? 0ull : met_mem) & ~turned;
        __syncthreads();
        u64 P = 0ull;
        if (alive) {
            const Body b = body_of(a, o, EN);
            const u64* G = a.stamps + (size_t)e * HW;
            for_cells(a, b, [&](int c) {
                const u64 s = G[c];
                if (valid_pet(a, s, lane, epoch, sw[wave])) P |= 1ull << ((uint32_t)s & 63u);
            });
        }
        const u64 fresh = P & ~met;
        met |= P;
        int c = __popcll(fresh);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
        if (in) {
            a.fresh[o] = fresh;
            if (met != met_mem) a.met[o] = met;
            if (aid != aid_mem) a.aid[o] = aid;
        }
        if (e < a.E && lane == 0) {
            a.n_fresh[e] = c;
            if (changed) {
                a.episode[e] = ep;
                a.epoch[e] = epoch;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(ASSIGN_THREADS) void pet_assign_kernel(PetArgs a) {
    assign(a.rows, a.E, [&](int e) { return a.n_fresh[e]; });
}

__global__ __launch_bounds__(TB) void pet_commit_kernel(PetArgs a) {
    __shared__ uint32_t sw[NW][64];
    __shared__ uint32_t sv[NW][64];            // speed bits of the slots
    __shared__ int32_t said[NW][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N;
    const size_t EN = (size_t)a.E * N, HW = (size_t)a.grid.H * a.grid.W;
    const uint32_t* su = reinterpret_cast<const uint32_t*>(a.state);
    for (int e0 = blockIdx.x * NW; e0 < a.E; e0 += gridDim.x * NW) {           // (the whole workgroup: the barriers below)
        const int e = e0 + wave;
        const bool in = e < a.E && lane < N;
        const size_t o = (size_t)(e < a.E ? e : 0) * N + (lane < N ? lane : 0);
        bool alive = false;
        int32_t aid = 0;
        sw[wave][lane] = slot_word(a, o, EN, in, alive, aid);
        sv[wave][lane] = in ? (su + 3 * EN)[o] : 0u;
        said[wave][lane] = aid;
        const u64 fresh = in ? a.fresh[o] : 0ull;
        __syncthreads();
        const int c = __popcll(fresh);
        int inc = c;                                   // inclusive prefix over the lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (fresh) {                                   // (a subset of the ALIVE lanes of a scene below E)
            const Body b = body_of(a, o, EN);
            const u64* G = a.stamps + (size_t)e * HW;
            const int32_t epoch = a.epoch[e], ep = a.env[(size_t)e * 4 + 1];
            const int g = a.groups.of(e);
            const uint32_t th = (su + 2 * EN)[o], hq_b = heading_q(__uint_as_float(th));
            long long id = (long long)a.rows.base[e] + (inc - c);
            for (u64 m = fresh; m; m &= m - 1ull, ++id) {
                const int s = __ffsll((long long)m) - 1;
                int pet = 0x7fffffff, cell = 0, n_cells = 0;
                uint32_t hq_a = 0u;
                for_cells(a, b, [&](int ci) {
                    const u64 w = G[ci];
                    if ((int)((uint32_t)w & 63u) != s) return;
                    const int d = valid_pet(a, w, lane, epoch, sw[wave]);
                    if (!d) return;
                    ++n_cells;
                    if (d < pet) {
                        pet = d; cell = ci; hq_a = ((uint32_t)w >> 8) & 255u;
                    }
                });
                uint4* R;
                if (row(a.rows, id, R)) {
                    R[0] = make_uint4((uint32_t)e, (uint32_t)lane | ((uint32_t)s << 6), (uint32_t)aid, (uint32_t)said[wave][s]);
                    R[1] = make_uint4((uint32_t)ep, (uint32_t)a.r, (uint32_t)pet, (uint32_t)cell);
                    R[2] = make_uint4((uint32_t)n_cells, sv[wave][s], su[o], (su + EN)[o]);
                    R[3] = make_uint4(th, sv[wave][lane], hq_a, hq_b);
                }
                if (g >= 0 && n_cells) {               // (pet is in 1..window then)
                    const uint32_t rel = (hq_b - hq_a) & 255u, d = rel < 256u - rel ? rel : 256u - rel;
                    const int type = d <= (uint32_t)PET_FOLLOW_Q ? 0 : (d >= (uint32_t)PET_OPPOSE_Q ? 2 : 1);
                    atomicAdd(reinterpret_cast<u64*>(a.hist) + ((size_t)g * PET_TYPES + type) * a.window + (pet - 1), 1ull);
                    if (pet <= a.critical_records) atomicAdd(reinterpret_cast<u64*>(a.critical) + (size_t)g * HW + cell, 1ull);
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(TB) void pet_stamp_kernel(PetArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N;
    const size_t EN = (size_t)a.E * N, HW = (size_t)a.grid.H * a.grid.W;
    for (int e = blockIdx.x * NW + wave; e < a.E; e += gridDim.x * NW) {
        if (lane >= N) continue;
        const size_t o = (size_t)e * N + lane;
        bool alive;
        int32_t aid;
        slot_word(a, o, EN, true, alive, aid);
        if (!alive) continue;
        const Body b = body_of(a, o, EN);
        const u64 stamp = ((u64)((uint32_t)a.r + 1u) << 32) | (u64)((((uint32_t)aid & 0xffffu) << 16) | (heading_q((a.state + 2 * EN)[o]) << 8) | (uint32_t)lane);
        u64* G = a.stamps + (size_t)e * HW;
        for_cells(a, b, [&](int c) { atomicMax(G + c, stamp); });
    }
}

hipError_t launch_pet_record(const PetArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(pet_scan_kernel, scene_grid(a.E), dim3(TB), 0, stream, a);
    hipLaunchKernelGGL(pet_assign_kernel, dim3(1), dim3(ASSIGN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(pet_commit_kernel, scene_grid(a.E), dim3(TB), 0, stream, a);
    hipLaunchKernelGGL(pet_stamp_kernel, scene_grid(a.E), dim3(TB), 0, stream, a);
    return hipGetLastError();
}

__global__ void pet_forget_kernel(int32_t* epoch, int E, int32_t r) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) epoch[e] = r;
}

hipError_t launch_pet_forget(int32_t* epoch, int E, int32_t r, hipStream_t stream) {
    hipLaunchKernelGGL(pet_forget_kernel, dim3((E + 255) / 256), dim3(256), 0, stream, epoch, E, r);
    return hipGetLastError();
}

}  // namespace copo
