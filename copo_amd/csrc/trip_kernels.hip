// Trip log over the simulator's scenes (copo_trip_*, include/copo_hip.h): one row per finished agent.  A trip is followed in its slot
// from the first record that sees the agent ALIVE to the record that ends it, and then leaves as ONE 64-byte row into a bounded pool.
// Three launches per record; the pool, the assign launch and the rule that decides the row ids are rowlog_common.h:
//   close:   one wave per scene, four scenes per 256-thread workgroup, lane n = slot n (every load and store over the slots is coalesced);
//            at most MAX_WG workgroups, beyond that a workgroup walks its scenes in strides of the grid.  Adds the step's reward to
//            the open trips, decides which of them end and writes the scene's 64-bit closing mask and the slots' end words
//   assign:  a scene's closes are the popcount of its mask: every scene gets the row id of its first closing slot
//   commit:  wave per scene again: a closing lane's id is the scene's base + the popcount of the mask below its lane, its row goes out as
//            four 16-byte stores; then the slots that are ALIVE without a trip open one, and every open trip accumulates this record
// No workgroup waits for another; the per-slot memory belongs to the scene's wave and no atomic touches it.  Integer logic, one fp32 add
// (the reward, one per record and trip: sequential), one fp32 product (the speed quantisation) and plain fp32 `<` only, so the numpy
// restatement (tests/trip_numpy.py) gives the same bits.  The rules are DESIGN.md section 8g.
#include "sim_device.h"
#include "trip_common.h"

namespace copo {

using namespace rowlog;

namespace {

__device__ __forceinline__ uint32_t* plane(const TripArgs& a, int k) { return a.mem + (size_t)k * a.E * a.N; }

}  // namespace

// flush != 0: every open trip closes with kind 3 and nothing else is read
__global__ __launch_bounds__(TB) void trip_close_kernel(TripArgs a, int flush) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N;
    const size_t EN = (size_t)a.E * N;
    const uint32_t* su = reinterpret_cast<const uint32_t*>(a.state);
    for (int e = blockIdx.x * NW + wave; e < a.E; e += gridDim.x * NW) {       // (the whole wave)
        const size_t o = (size_t)e * N + lane;
        const u64 open_mask = a.open[e];
        const bool open = lane < N && ((open_mask >> lane) & 1ull);
        bool close = false;
        uint32_t endw = 0u;
        if (open && flush) {
            close = true;
            endw = (uint32_t)TRIP_KIND_FLUSH << 8;
        } else if (open) {
            const uint32_t f = a.flags ? (uint32_t)a.flags[o] : 0u;
            if ((f & COPO_F_ACTED) && a.rew) {
                float* R = reinterpret_cast<float*>(plane(a, TM_REWARD)) + o;
                *R = *R + a.rew[o];
            }
            if (f & COPO_F_DONE) {
                close = true;
                endw = f | ((uint32_t)TRIP_KIND_DONE << 8);
            } else {
                const bool same = st_status((int32_t)(su + 13 * EN)[o]) == ST_ALIVE && (su + 14 * EN)[o] == plane(a, TM_AID)[o] &&
                                  a.env[(size_t)e * 4 + 1] == a.episode[e];
                close = !same;
                endw = (uint32_t)TRIP_KIND_VANISHED << 8;
            }
        }
        const u64 m = __ballot(close);
        if (close) a.endw[o] = endw;
        if (lane == 0) a.closing[e] = m;
    }
}

__global__ __launch_bounds__(ASSIGN_THREADS) void trip_assign_kernel(TripArgs a) {
    assign(a.rows, a.E, [&](int e) { return __popcll(a.closing[e]); });
}

// flush != 0: rows only, nothing opens or accumulates and no trip stays open
__global__ __launch_bounds__(TB) void trip_commit_kernel(TripArgs a, int flush) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N;
    const size_t EN = (size_t)a.E * N;
    const uint32_t* su = reinterpret_cast<const uint32_t*>(a.state);
    for (int e = blockIdx.x * NW + wave; e < a.E; e += gridDim.x * NW) {       // (the whole wave)
        const size_t o = (size_t)e * N + lane;
        const bool in = lane < N;
        const u64 open_mask = a.open[e], m = a.closing[e];
        const int32_t ep_mem = a.episode[e];
        const bool closing = (m >> lane) & 1ull;       // (closing is a subset of open, open of the lanes below N)
        if (closing) {
            uint4* R;
            if (row(a.rows, (long long)a.rows.base[e] + __popcll(m & ((1ull << lane) - 1ull)), R)) {
                R[0] = make_uint4((uint32_t)e, (uint32_t)lane | (plane(a, TM_ROUTE)[o] << 16), plane(a, TM_AID)[o], (uint32_t)ep_mem);
                R[1] = make_uint4(plane(a, TM_FIRST)[o], plane(a, TM_STEPS)[o], a.endw[o], plane(a, TM_LCF)[o]);
                R[2] = make_uint4(plane(a, TM_PROG0)[o], plane(a, TM_PROG1)[o], plane(a, TM_SPEED_SUM)[o], plane(a, TM_SPEED_MAX)[o]);
                R[3] = make_uint4(plane(a, TM_STOPS)[o], plane(a, TM_REWARD)[o], plane(a, TM_MIN_GAP)[o], plane(a, TM_MIN_TTC)[o]);
            }
        }
        u64 now_open = 0ull;
        if (!flush) {
            const int32_t ep = a.env[(size_t)e * 4 + 1];
            const bool was_open = in && ((open_mask >> lane) & 1ull) && !closing;
            const bool alive = in && st_status((int32_t)(su + 13 * EN)[o]) == ST_ALIVE;
            const bool opening = alive && !was_open;
            uint32_t steps = 0u, speed_sum = 0u, speed_max = 0u, stops = 0u;
            float min_gap = __uint_as_float(0x7f800000u), min_ttc = __uint_as_float(0x7f800000u);
            if (opening) {
                plane(a, TM_AID)[o] = (su + 14 * EN)[o];
                plane(a, TM_FIRST)[o] = (uint32_t)a.r;
                plane(a, TM_ROUTE)[o] = (su + 12 * EN)[o] & 0xffffu;
                plane(a, TM_LCF)[o] = (su + 10 * EN)[o];
                plane(a, TM_PROG0)[o] = (su + 9 * EN)[o];
                plane(a, TM_REWARD)[o] = 0u;           // +0.0f
            } else if (was_open) {
                steps = plane(a, TM_STEPS)[o]; speed_sum = plane(a, TM_SPEED_SUM)[o]; speed_max = plane(a, TM_SPEED_MAX)[o];
                stops = plane(a, TM_STOPS)[o];
                min_gap = __uint_as_float(plane(a, TM_MIN_GAP)[o]); min_ttc = __uint_as_float(plane(a, TM_MIN_TTC)[o]);
            }
            if (opening || was_open) {
                const float v = (a.state + 3 * EN)[o];
                const uint32_t q = (uint32_t)__float2int_rn(fminf(fmaxf(v, 0.0f), 255.0f) * 256.0f);
                steps += 1u;
                speed_sum += q;
                speed_max = q > speed_max ? q : speed_max;
                stops += v < a.stop_speed ? 1u : 0u;
                if (a.gap) {
                    const float g = a.gap[o];
                    if (g < min_gap) min_gap = g;
                }
                if (a.ttc) {
                    const float t = a.ttc[o];
                    if (t < min_ttc) min_ttc = t;
                }
                plane(a, TM_PROG1)[o] = (su + 9 * EN)[o];
                plane(a, TM_STEPS)[o] = steps; plane(a, TM_SPEED_SUM)[o] = speed_sum; plane(a, TM_SPEED_MAX)[o] = speed_max;
                plane(a, TM_STOPS)[o] = stops;
                plane(a, TM_MIN_GAP)[o] = __float_as_uint(min_gap); plane(a, TM_MIN_TTC)[o] = __float_as_uint(min_ttc);
            }
            now_open = __ballot(opening || was_open);
            // (stored only when changed: the store then depends on the value read at the top of this scene)
            if (lane == 0 && ep != ep_mem) a.episode[e] = ep;
        }
        if (lane == 0 && now_open != open_mask) a.open[e] = now_open;
    }
}

static hipError_t launch_all(const TripArgs& a, int flush, hipStream_t stream) {
    return launch(trip_close_kernel, trip_assign_kernel, trip_commit_kernel, a, flush, stream);
}

hipError_t launch_trip_record(const TripArgs& a, hipStream_t stream) { return launch_all(a, 0, stream); }

hipError_t launch_trip_flush(const TripArgs& a, hipStream_t stream) { return launch_all(a, 1, stream); }

}  // namespace copo
