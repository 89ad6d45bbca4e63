// Conflict log over the simulator's scenes (copo_conflict_*, include/copo_hip.h): one row per pairwise encounter; no counterpart in the
// reference.  An encounter of slots a < b opens in the record that sees both ALIVE closer than `radius`, is followed in the pair's 48
// bytes of memory (steps, the smallest squared distance and both poses at it) and leaves as ONE 64-byte row into a bounded pool when a
// party ends, vanishes or the two part beyond `leave_radius`.  Three launches per record; the pool, the assign launch and the rule that
// decides the row ids are rowlog_common.h:
//   close:   one wave per scene, four scenes per 256-thread workgroup, lane n = slot n; at most MAX_WG workgroups, beyond that a
//            workgroup walks its scenes in strides of the grid.  The positions and one word per slot (end flags, same identity, ALIVE) are
//            staged into LDS; lane a walks the partners of its open mask, decides which encounters close and writes its 64-bit closing
//            mask and the scene's close count
//   assign:  a scene's closes are its close count: every scene gets the row id of its first closing pair
//   commit:  wave per scene again: a closing pair's id is the scene's base + the popcounts of the closing masks of the lanes below a (a
//            prefix over lanes) + the popcount of a's mask below b; its row goes out as four 16-byte stores.  Then lane a walks the ALIVE
//            partners above it: pairs closer than `radius` open, every open pair accumulates this record
// No workgroup waits for another; the per-pair and per-slot memory belongs to the scene's wave and no atomic touches it.  Integer logic,
// two fp32 subtractions, two products, one add (each rounded by itself: the library is built with -ffp-contract=off) and plain fp32 `<`
// only -- no fused multiply-add, square root or division -- so the numpy restatement (tests/conflict_numpy.py) gives the same bits.
// The rules are DESIGN.md section 8h.
#include "sim_device.h"
#include "conflict_common.h"

namespace copo {

using namespace rowlog;

namespace {

constexpr uint32_t SW_SAME = 1u << 8, SW_ALIVE = 1u << 9;      // above the end byte of a slot word
constexpr uint32_t INF_BITS = 0x7f800000u;

// bits above lane a (a = 63: none)
__device__ __forceinline__ u64 above(int a) { return (~1ull) << a; }

// (a, b), a < b < N -> index of the pair's memory in its scene
__device__ __forceinline__ int pair_index(int a, int b, int N) { return a * (2 * N - a - 1) / 2 + (b - a - 1); }

// What both the close and the commit launch read of slot `lane` of scene e: the flags byte when it carries DONE (else 0), whether the slot
// is ALIVE now with the identity the handle remembers, whether it is ALIVE now.  Nothing it reads changes between the two launches.
__device__ __forceinline__ uint32_t slot_word(const ConflictArgs& a, int e, int lane, int32_t ep_now, int32_t ep_mem) {
    if (lane >= a.N) return 0u;
    const size_t EN = (size_t)a.E * a.N, o = (size_t)e * a.N + lane;
    const uint32_t* su = reinterpret_cast<const uint32_t*>(a.state);
    const uint32_t f = a.flags ? (uint32_t)a.flags[o] : 0u;
    const bool alive = st_status((int32_t)(su + 13 * EN)[o]) == ST_ALIVE;
    const bool same = alive && (int32_t)(su + 14 * EN)[o] == a.aid[o] && ep_now == ep_mem;
    return ((f & COPO_F_DONE) ? f : 0u) | (same ? SW_SAME : 0u) | (alive ? SW_ALIVE : 0u);
}

__device__ __forceinline__ float dist2(float xa, float ya, float xb, float yb) {
    const float dx = xb - xa, dy = yb - ya;
    const float px = dx * dx, py = dy * dy;
    return px + py;
}

}  // namespace

// flush != 0: every open encounter closes and nothing else is read
__global__ __launch_bounds__(TB) void conflict_close_kernel(ConflictArgs a, int flush) {
    __shared__ float sx[NW][64], sy[NW][64];
    __shared__ uint32_t sw[NW][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N;
    const size_t EN = (size_t)a.E * N;
    for (int e0 = blockIdx.x * NW; e0 < a.E; e0 += gridDim.x * NW) {           // (the whole workgroup: the barriers below)
        const int e = e0 + wave;
        const bool in = e < a.E && lane < N;
        const size_t o = (size_t)e * N + lane;
        const u64 om = in ? a.open[o] : 0ull;
        if (e < a.E && !flush) {
            sx[wave][lane] = in ? a.state[o] : 0.0f;
            sy[wave][lane] = in ? (a.state + EN)[o] : 0.0f;
            sw[wave][lane] = slot_word(a, e, lane, a.env[(size_t)e * 4 + 1], a.episode[e]);
        }
        __syncthreads();
        u64 cm = 0ull;
        if (flush) {
            cm = om;
        } else if (om) {
            const uint32_t wa = sw[wave][lane];
            const float xa = sx[wave][lane], ya = sy[wave][lane];
            for (u64 m = om; m; m &= m - 1ull) {
                const int b = __ffsll((long long)m) - 1;
                const uint32_t wb = sw[wave][b];
                bool close = ((wa | wb) & COPO_F_DONE) || !((wa & wb) & SW_SAME);
                if (!close) close = !(dist2(xa, ya, sx[wave][b], sy[wave][b]) < a.r2_out);
                if (close) cm |= 1ull << b;
            }
        }
        int c = __popcll(cm);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
        if (in) a.closing[o] = cm;
        if (e < a.E && lane == 0) a.n_closing[e] = c;
        __syncthreads();
    }
}

__global__ __launch_bounds__(ASSIGN_THREADS) void conflict_assign_kernel(ConflictArgs a) {
    assign(a.rows, a.E, [&](int e) { return a.n_closing[e]; });
}

// flush != 0: rows only, nothing opens or accumulates and no encounter stays open
__global__ __launch_bounds__(TB) void conflict_commit_kernel(ConflictArgs a, int flush) {
    __shared__ uint4 sp[NW][64];               // pose words {x, y, heading, speed} of the slots
    __shared__ uint32_t sw[NW][64];
    __shared__ int32_t said[NW][64];           // the remembered agent ids
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N;
    const size_t EN = (size_t)a.E * N;
    const size_t P = (size_t)N * (N - 1) / 2;
    const uint32_t* su = reinterpret_cast<const uint32_t*>(a.state);
    for (int e0 = blockIdx.x * NW; e0 < a.E; e0 += gridDim.x * NW) {           // (the whole workgroup: the barriers below)
        const int e = e0 + wave;
        const bool in = e < a.E && lane < N;
        const size_t o = (size_t)e * N + lane;
        const u64 om = in ? a.open[o] : 0ull, cm = in ? a.closing[o] : 0ull;
        int32_t ep_mem = 0, ep = 0, aid_mem = 0;
        if (e < a.E) {
            ep_mem = a.episode[e];
            ep = a.env[(size_t)e * 4 + 1];
            aid_mem = in ? a.aid[o] : 0;
            sp[wave][lane] = in ? make_uint4(su[o], (su + EN)[o], (su + 2 * EN)[o], (su + 3 * EN)[o]) : make_uint4(0u, 0u, 0u, 0u);
            sw[wave][lane] = flush ? 0u : slot_word(a, e, lane, ep, ep_mem);
            said[wave][lane] = aid_mem;
        }
        __syncthreads();
        uint4* mem = reinterpret_cast<uint4*>(a.pairs) + (size_t)(e < a.E ? e : 0) * P * (CONFLICT_PAIR_WORDS / 4);
        // the rows of the closing pairs
        const int c = __popcll(cm);
        int inc = c;                                   // inclusive prefix over the lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (cm) {
            const uint32_t wa = sw[wave][lane];
            long long id = (long long)a.rows.base[e] + (inc - c);
            uint4* R;
            for (u64 m = cm; m && row(a.rows, id, R); m &= m - 1ull, ++id) {
                const int b = __ffsll((long long)m) - 1;
                const uint32_t wb = sw[wave][b];
                uint32_t kind = CONFLICT_KIND_FLUSH, end_a = 0u, end_b = 0u;
                if (!flush) {
                    if ((wa | wb) & COPO_F_DONE) {
                        kind = CONFLICT_KIND_DONE; end_a = wa & 0xffu; end_b = wb & 0xffu;
                    } else {
                        kind = ((wa & wb) & SW_SAME) ? CONFLICT_KIND_PARTED : CONFLICT_KIND_VANISHED;
                    }
                }
                const uint4* M = mem + (size_t)pair_index(lane, b, N) * (CONFLICT_PAIR_WORDS / 4);
                const uint4 h = M[0];                  // {first_rec, steps, d2min bits, min_off}
                R[0] = make_uint4((uint32_t)e, (uint32_t)lane | ((uint32_t)b << 6) | (kind << 12) | (end_a << 16) | (end_b << 24), (uint32_t)aid_mem,
                                  (uint32_t)said[wave][b]);
                R[1] = make_uint4((uint32_t)ep_mem, h.x, h.y | (h.w << 16), h.z);
                R[2] = M[1];
                R[3] = M[2];
            }
        }
        u64 now = 0ull;
        const u64 alive_mask = __ballot(in && (sw[wave][lane] & SW_ALIVE));      // (the whole wave; flush: none)
        if (!flush && in) {
            const uint32_t wa = sw[wave][lane];
            const u64 after = om & ~cm;
            // the ALIVE slots above this lane: an encounter that is open after the closes has both parties among them
            const u64 cand = (wa & SW_ALIVE) ? alive_mask & above(lane) : 0ull;
            const uint4 pa = sp[wave][lane];
            const float xa = __uint_as_float(pa.x), ya = __uint_as_float(pa.y);
            now = after;
            for (u64 m = cand; m; m &= m - 1ull) {
                const int b = __ffsll((long long)m) - 1;
                const uint4 pb = sp[wave][b];
                const float d2 = dist2(xa, ya, __uint_as_float(pb.x), __uint_as_float(pb.y));
                const bool was = (after >> b) & 1ull;
                if (!was && !(d2 < a.r2_in)) continue;
                uint4* M = mem + (size_t)pair_index(lane, b, N) * (CONFLICT_PAIR_WORDS / 4);
                uint4 h = was ? M[0] : make_uint4((uint32_t)a.r, 0u, INF_BITS, 0u);
                h.y = h.y < 65535u ? h.y + 1u : 65535u;
                if (d2 < __uint_as_float(h.z)) {
                    const uint32_t off = (uint32_t)a.r - h.x;
                    h.z = __float_as_uint(d2);
                    h.w = off < 65535u ? off : 65535u;
                    M[1] = pa;
                    M[2] = pb;
                }
                M[0] = h;
                now |= 1ull << b;
            }
        }
        if (in) {
            if (now != om) a.open[o] = now;
            if (!flush) {
                const int32_t aid = (int32_t)(su + 14 * EN)[o];
                if (aid != aid_mem) a.aid[o] = aid;
                if (lane == 0 && ep != ep_mem) a.episode[e] = ep;
            }
        }
        __syncthreads();
    }
}

static hipError_t launch_all(const ConflictArgs& a, int flush, hipStream_t stream) {
    return launch(conflict_close_kernel, conflict_assign_kernel, conflict_commit_kernel, a, flush, stream);
}

hipError_t launch_conflict_record(const ConflictArgs& a, hipStream_t stream) { return launch_all(a, 0, stream); }

hipError_t launch_conflict_flush(const ConflictArgs& a, hipStream_t stream) { return launch_all(a, 1, stream); }

}  // namespace copo
