// Seat tally (copo_seat_tally, include/copo_hip.h): one step's flags and rewards of scenes whose slots ("seats") belong to different
// members of a policy bank, folded per (scene group, member) into eight int64 words.  Stateless, one launch, no allocation.
//   one wave per scene, four scenes per 256-thread workgroup, slot = lane + 64 j (up to COPO_SEAT_MAX_SLOTS slots);
//   per round of 64 slots the wave walks the members present in it: the first lane not yet served names a member, a ballot collects
//   that member's lanes, popcounts give its counts and an integer butterfly its reward sum; lanes 0..7 then own the eight words and
//   add the non-zero ones to the output with 64-bit integer atomics.
// Every word is an integer (the reward in 2^-16 steps, rounded per row), so the sums do not depend on the order the device adds in.
// The rules are restated as python loops by tests/crossplay_numpy.py.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sim_common.h"
#include "seat_common.h"

namespace copo {

namespace {

constexpr int SCENES_PER_WG = 4;       // waves of a 256-thread workgroup

// rint(min(max(r, -1024), 1024) * 65536): the clamp makes the product exact in fp32 (a power of two, no overflow), so the one rounding
// is rintf's, half to even.  NaN counts as 0.
__device__ inline int64_t seat_reward_q16(float r) {
    if (r != r) return 0;
    return (int64_t)rintf(fminf(fmaxf(r, -1024.0f), 1024.0f) * 65536.0f);
}

}  // namespace

__global__ __launch_bounds__(256) void seat_tally_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ rew,
                                                         const int32_t* __restrict__ seat, const int32_t* __restrict__ group,
                                                         int32_t E, int32_t N, int32_t K, int32_t G, int64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * SCENES_PER_WG + wave;
    if (e >= E) return;                        // (the whole wave; there is no barrier in this kernel)
    const int g = group[e];
    if (g < 0 || g >= G) return;               // (the whole wave)
    for (int j = 0; 64 * j < N; ++j) {
        const int n = lane + 64 * j;
        const size_t idx = (size_t)e * N + (n < N ? n : 0);
        const int s = n < N ? seat[idx] : -1;
        const bool seated = s >= 0 && s < K;
        const uint32_t f = seated ? (uint32_t)flags[idx] : 0u;
        const bool acted = (f & COPO_F_ACTED) != 0u, done = acted && (f & COPO_F_DONE) != 0u;
        const int64_t q = (rew && acted) ? seat_reward_q16(rew[idx]) : 0;
        uint64_t todo = __ballot((f & (COPO_F_ACTED | COPO_F_SPAWNED)) != 0u);      // lanes with something to add; uniform over the wave
        while (todo) {
            const int m = __shfl(s, __ffsll((unsigned long long)todo) - 1);          // a served lane is seated: 0 <= m < K
            const bool mine = seated && s == m;
            todo &= ~__ballot(mine);
            const int64_t qs = wave_sum_i64(mine ? q : 0);
            const int c_acted = __popcll(__ballot(mine && acted)), c_done = __popcll(__ballot(mine && done));
            const int c_arrive = __popcll(__ballot(mine && done && (f & COPO_F_ARRIVE) != 0u));
            const int c_crash = __popcll(__ballot(mine && done && (f & COPO_F_CRASH) != 0u));
            const int c_out = __popcll(__ballot(mine && done && (f & COPO_F_OUT) != 0u));
            const int c_maxstep = __popcll(__ballot(mine && done && (f & COPO_F_MAXSTEP) != 0u));
            const int c_spawned = __popcll(__ballot(mine && (f & COPO_F_SPAWNED) != 0u));
            if (lane < COPO_SEAT_WORDS) {
                const int64_t v = lane == COPO_SEAT_ACTED ? c_acted : lane == COPO_SEAT_DONE ? c_done : lane == COPO_SEAT_ARRIVE ? c_arrive
                                : lane == COPO_SEAT_CRASH ? c_crash : lane == COPO_SEAT_OUT ? c_out : lane == COPO_SEAT_MAXSTEP ? c_maxstep
                                : lane == COPO_SEAT_REWARD_Q16 ? qs : c_spawned;
                if (v != 0)
                    atomicAdd(reinterpret_cast<unsigned long long*>(out) + ((size_t)g * K + m) * COPO_SEAT_WORDS + lane, (unsigned long long)v);
            }
        }
    }
}

// Certify tally (copo_certify_tally): one step's certified bounds (copo_cert_obs_seats_f32) folded per (scene
// group, member) against the level's deltas.  The wave walk is seat_tally_kernel's; the words are counts, sums of quantised widths
// (rounded once per row, as the reward above) and one 64-bit atomic max, so the result does not depend on the order either.
namespace {

// rint(min(max(x, 0), 1024) * 65536): exact product, one rounding (the callers pass finite values)
__device__ inline int64_t cert_q16(float x) { return (int64_t)rintf(fminf(fmaxf(x, 0.0f), 1024.0f) * 65536.0f); }

}  // namespace

__global__ __launch_bounds__(256) void certify_tally_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ bounds,
                                                            const int32_t* __restrict__ seat, const int32_t* __restrict__ group,
                                                            const int32_t* __restrict__ level_of, const float* __restrict__ levels,
                                                            int32_t E, int32_t N, int32_t K, int32_t G, int32_t L, int64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * SCENES_PER_WG + wave;
    if (e >= E) return;                        // (the whole wave; there is no barrier in this kernel)
    const int g = group[e];
    if (g < 0 || g >= G) return;               // (the whole wave)
    for (int j = 0; 64 * j < N; ++j) {
        const int n = lane + 64 * j;
        const size_t idx = (size_t)e * N + (n < N ? n : 0);
        const int s = n < N ? seat[idx] : -1;
        const bool seated = s >= 0 && s < K;
        const int lv = seated ? level_of[(size_t)g * K + s] : -1;
        const bool counted = seated && lv >= 0 && lv < L && ((uint32_t)flags[idx] & COPO_F_ACTED) != 0u &&
                             bounds[idx * COPO_CERT_WORDS + 6] == 1.0f;
        bool finite = false, ok0 = false, ok1 = false;
        int64_t qw0 = 0, qw1 = 0, qdev = 0;
        if (counted) {
            const float* b = bounds + idx * COPO_CERT_WORDS;
            const float lo0 = b[0], hi0 = b[1], lo1 = b[2], hi1 = b[3], mu0 = b[4], mu1 = b[5];
            finite = isfinite(lo0) && isfinite(hi0) && isfinite(lo1) && isfinite(hi1) && isfinite(mu0) && isfinite(mu1);
            if (finite) {
                const float dev0 = fmaxf(hi0 - mu0, mu0 - lo0), dev1 = fmaxf(hi1 - mu1, mu1 - lo1);
                ok0 = dev0 <= levels[4 * lv + 1];
                ok1 = dev1 <= levels[4 * lv + 2];
                qw0 = cert_q16(hi0 - lo0);
                qw1 = cert_q16(hi1 - lo1);
                qdev = cert_q16(fmaxf(dev0, dev1));
            }
        }
        uint64_t todo = __ballot(counted);      // lanes with something to add; uniform over the wave
        while (todo) {
            const int m = __shfl(s, __ffsll((unsigned long long)todo) - 1);          // a served lane is seated: 0 <= m < K
            const bool mine = counted && s == m;
            todo &= ~__ballot(mine);
            const int64_t s0 = wave_sum_i64(mine ? qw0 : 0), s1 = wave_sum_i64(mine ? qw1 : 0), mx = wave_max_i64(mine ? qdev : 0);
            const int c_rows = __popcll(__ballot(mine)), c_both = __popcll(__ballot(mine && ok0 && ok1));
            const int c_steer = __popcll(__ballot(mine && ok0)), c_throttle = __popcll(__ballot(mine && ok1));
            const int c_bad = __popcll(__ballot(mine && !finite));
            if (lane < COPO_CERT_TALLY_WORDS) {
                const int64_t v = lane == 0 ? c_rows : lane == 1 ? c_both : lane == 2 ? c_steer : lane == 3 ? c_throttle : lane == 4 ? s0
                                : lane == 5 ? s1 : lane == 6 ? mx : c_bad;
                unsigned long long* at = reinterpret_cast<unsigned long long*>(out) + ((size_t)g * K + m) * COPO_CERT_TALLY_WORDS + lane;
                if (v != 0) {
                    if (lane == 6) atomicMax(at, (unsigned long long)v);
                    else atomicAdd(at, (unsigned long long)v);
                }
            }
        }
    }
}

// Jury tally (copo_jury_tally): one step's verdicts (copo_jury_obs_seats_f32) against the driver's own distribution
// inputs, folded per (scene group, driving member, judging member).  The wave walk is seat_tally_kernel's, once per judge of the scene's
// group (the judge loop is uniform over the wave: judges[g] is the scene's); the words are counts, sums of values quantised once per
// pair and one 64-bit atomic max, so the result does not depend on the order.  (jury_q16 / jury_kl: seat_common.h)
__global__ __launch_bounds__(256) void jury_tally_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ dist,
                                                         const float* __restrict__ verdict, const int32_t* __restrict__ seat,
                                                         const int32_t* __restrict__ group, const int32_t* __restrict__ judges, int32_t E,
                                                         int32_t N, int32_t K, int32_t G, float delta_steer, float delta_throttle,
                                                         int64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * SCENES_PER_WG + wave;
    if (e >= E) return;                        // (the whole wave; there is no barrier in this kernel)
    const int g = group[e];
    if (g < 0 || g >= G) return;               // (the whole wave)
    for (int j = 0; 64 * j < N; ++j) {
        const int n = lane + 64 * j;
        const size_t idx = (size_t)e * N + (n < N ? n : 0);
        const int s = n < N ? seat[idx] : -1;
        const bool counted = s >= 0 && s < K && ((uint32_t)flags[idx] & COPO_F_ACTED) != 0u;
        if (!__ballot(counted)) continue;      // (uniform)
        const float4 own = counted ? *reinterpret_cast<const float4*>(dist + idx * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int jj = 0; jj < K; ++jj) {
            if (judges[(size_t)g * K + jj] == 0) continue;      // (uniform: one word per wave)
            int64_t q0 = 0, q1 = 0, qs = 0, qkl = 0, qlk = 0, qmx = 0;
            bool apart = false;
            if (counted) {
                const float4 v = *reinterpret_cast<const float4*>(verdict + (idx * K + jj) * 4);
                const float d0 = fabsf(__fsub_rn(v.x, own.x)), d1 = fabsf(__fsub_rn(v.y, own.y));
                const float ds = __fadd_rn(fabsf(__fsub_rn(v.z, own.z)), fabsf(__fsub_rn(v.w, own.w)));
                apart = d0 > delta_steer || d1 > delta_throttle;
                q0 = jury_q16(d0);
                q1 = jury_q16(d1);
                qs = jury_q16(ds);
                qkl = jury_q16(jury_kl(own, v));
                qlk = jury_q16(jury_kl(v, own));
                qmx = jury_q16(fmaxf(d0, d1));
            }
            uint64_t todo = __ballot(counted);      // lanes with something to add; uniform over the wave
            while (todo) {
                const int m = __shfl(s, __ffsll((unsigned long long)todo) - 1);          // a served lane is seated: 0 <= m < K
                const bool mine = counted && s == m;
                todo &= ~__ballot(mine);
                const int c_pairs = __popcll(__ballot(mine)), c_apart = __popcll(__ballot(mine && apart));
                const int64_t s0 = wave_sum_i64(mine ? q0 : 0), s1 = wave_sum_i64(mine ? q1 : 0), ss = wave_sum_i64(mine ? qs : 0);
                const int64_t skl = wave_sum_i64(mine ? qkl : 0), slk = wave_sum_i64(mine ? qlk : 0), mx = wave_max_i64(mine ? qmx : 0);
                if (lane < COPO_JURY_WORDS) {
                    const int64_t v = lane == 0 ? c_pairs : lane == 1 ? c_apart : lane == 2 ? s0 : lane == 3 ? s1 : lane == 4 ? ss
                                    : lane == 5 ? skl : lane == 6 ? slk : mx;
                    unsigned long long* at = reinterpret_cast<unsigned long long*>(out) + (((size_t)g * K + m) * K + jj) * COPO_JURY_WORDS + lane;
                    if (v != 0) {
                        if (lane == 7) atomicMax(at, (unsigned long long)v);
                        else atomicAdd(at, (unsigned long long)v);
                    }
                }
            }
        }
    }
}

hipError_t launch_jury_tally(const uint8_t* flags, const float* dist, const float* verdict, const int32_t* seat, const int32_t* group,
                             const int32_t* judges, int32_t E, int32_t N, int32_t K, int32_t G, float delta_steer, float delta_throttle,
                             int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(jury_tally_kernel, dim3((E + SCENES_PER_WG - 1) / SCENES_PER_WG), dim3(256), 0, stream, flags, dist, verdict, seat, group,
                       judges, E, N, K, G, delta_steer, delta_throttle, out);
    return hipGetLastError();
}

hipError_t launch_certify_tally(const uint8_t* flags, const float* bounds, const int32_t* seat, const int32_t* group, const int32_t* level_of,
                                const float* levels, int32_t E, int32_t N, int32_t K, int32_t G, int32_t L, int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(certify_tally_kernel, dim3((E + SCENES_PER_WG - 1) / SCENES_PER_WG), dim3(256), 0, stream, flags, bounds, seat, group,
                       level_of, levels, E, N, K, G, L, out);
    return hipGetLastError();
}

hipError_t launch_seat_tally(const uint8_t* flags, const float* rew, const int32_t* seat, const int32_t* group, int32_t E, int32_t N,
                             int32_t K, int32_t G, int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(seat_tally_kernel, dim3((E + SCENES_PER_WG - 1) / SCENES_PER_WG), dim3(256), 0, stream, flags, rew, seat, group, E, N, K,
                       G, out);
    return hipGetLastError();
}

}  // namespace copo
