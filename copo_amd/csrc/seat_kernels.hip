// Seat tally (copo_seat_tally, include/copo_hip.h): one step's flags and rewards of scenes whose slots ("seats") belong to different
// members of a policy bank, folded per (scene group, member) into eight int64 words.  Stateless, one launch, no allocation.
//   one wave per scene, four scenes per 256-thread workgroup, slot = lane + 64 j (up to COPO_SEAT_MAX_SLOTS slots);
//   per round of 64 slots the wave walks the members present in it: the first lane not yet served names a member, a ballot collects
//   that member's lanes, popcounts give its counts and an integer butterfly its reward sum; lanes 0..7 then own the eight words and
//   add the non-zero ones to the output with 64-bit integer atomics.
// That walk is seat_walk / SeatLane::serve (seat_common.h), the only text of it: every tally below, and the influence tally
// (influence_kernels.hip), states the kinds of its eight words and what a lane contributes, nothing else.
// Every word is an integer (the reward in 2^-16 steps, rounded per row), so the sums do not depend on the order the device adds in.
// The rules are restated as python loops by tests/crossplay_numpy.py.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sim_common.h"
#include "seat_common.h"

namespace copo {

using SeatWords = WordKinds<W_COUNT, W_COUNT, W_COUNT, W_COUNT, W_COUNT, W_COUNT, W_SUM, W_COUNT>;
static_assert(COPO_SEAT_ACTED == 0 && COPO_SEAT_DONE == 1 && COPO_SEAT_ARRIVE == 2 && COPO_SEAT_CRASH == 3 && COPO_SEAT_OUT == 4 &&
              COPO_SEAT_MAXSTEP == 5 && COPO_SEAT_REWARD_Q16 == 6 && COPO_SEAT_SPAWNED == 7 && COPO_SEAT_WORDS == 8, "the order of v[] below");

__global__ __launch_bounds__(256) void seat_tally_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ rew,
                                                         const int32_t* __restrict__ seat, const int32_t* __restrict__ group,
                                                         int32_t E, int32_t N, int32_t K, int32_t G, int64_t* __restrict__ out) {
    seat_walk(seat, group, E, N, K, G, [&](const SeatLane& L) {
        const uint32_t f = L.seated ? (uint32_t)flags[L.idx] : 0u;
        const bool acted = (f & COPO_F_ACTED) != 0u, done = acted && (f & COPO_F_DONE) != 0u;
        const int64_t v[COPO_SEAT_WORDS] = {acted, done, done && (f & COPO_F_ARRIVE) != 0u, done && (f & COPO_F_CRASH) != 0u,
                                            done && (f & COPO_F_OUT) != 0u, done && (f & COPO_F_MAXSTEP) != 0u,
                                            (rew && acted) ? q16(rew[L.idx], -1024.0f) : 0, (f & COPO_F_SPAWNED) != 0u};
        L.serve(SeatWords{}, (f & (COPO_F_ACTED | COPO_F_SPAWNED)) != 0u, v, out, [&](int m) { return (size_t)L.g * K + m; });
    });
}

// Certify tally (copo_certify_tally): one step's certified bounds (copo_cert_obs_seats_f32) folded per (scene
// group, member) against the level's deltas.  The words are counts, sums of quantised widths (rounded once per row, as the reward
// above) and one 64-bit atomic max, so the result does not depend on the order either.
using CertWords = WordKinds<W_COUNT, W_COUNT, W_COUNT, W_COUNT, W_SUM, W_SUM, W_MAX, W_COUNT>;

__global__ __launch_bounds__(256) void certify_tally_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ bounds,
                                                            const int32_t* __restrict__ seat, const int32_t* __restrict__ group,
                                                            const int32_t* __restrict__ level_of, const float* __restrict__ levels,
                                                            int32_t E, int32_t N, int32_t K, int32_t G, int32_t L, int64_t* __restrict__ out) {
    seat_walk(seat, group, E, N, K, G, [&](const SeatLane& S) {
        const size_t idx = S.idx;
        const int lv = S.seated ? level_of[(size_t)S.g * K + S.s] : -1;
        const bool counted = S.seated && lv >= 0 && lv < L && ((uint32_t)flags[idx] & COPO_F_ACTED) != 0u &&
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
                qw0 = q16(hi0 - lo0);
                qw1 = q16(hi1 - lo1);
                qdev = q16(fmaxf(dev0, dev1));
            }
        }
        const int64_t v[COPO_CERT_TALLY_WORDS] = {1, ok0 && ok1, ok0, ok1, qw0, qw1, qdev, !finite};      // rows, both, steer, throttle, .., bad
        S.serve(CertWords{}, counted, v, out, [&](int m) { return (size_t)S.g * K + m; });
    });
}

// Jury tally (copo_jury_tally): one step's verdicts (copo_jury_obs_seats_f32) against the driver's own distribution
// inputs, folded per (scene group, driving member, judging member): the members of a round are served once per judge of the scene's
// group (the judge loop is uniform over the wave: judges[g] is the scene's), into cell [g][m][judge].  The words are counts, sums of
// values quantised once per pair and one 64-bit atomic max, so the result does not depend on the order.  (q16 / jury_kl: seat_common.h)
using JuryWords = WordKinds<W_COUNT, W_COUNT, W_SUM, W_SUM, W_SUM, W_SUM, W_SUM, W_MAX>;

__global__ __launch_bounds__(256) void jury_tally_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ dist,
                                                         const float* __restrict__ verdict, const int32_t* __restrict__ seat,
                                                         const int32_t* __restrict__ group, const int32_t* __restrict__ judges, int32_t E,
                                                         int32_t N, int32_t K, int32_t G, float delta_steer, float delta_throttle,
                                                         int64_t* __restrict__ out) {
    seat_walk(seat, group, E, N, K, G, [&](const SeatLane& L) {
        const size_t idx = L.idx;
        const bool counted = L.seated && ((uint32_t)flags[idx] & COPO_F_ACTED) != 0u;
        if (!__ballot(counted)) return;        // (uniform)
        const float4 own = counted ? *reinterpret_cast<const float4*>(dist + idx * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int jj = 0; jj < K; ++jj) {
            if (judges[(size_t)L.g * K + jj] == 0) continue;      // (uniform: one word per wave)
            int64_t w[COPO_JURY_WORDS] = {1, 0, 0, 0, 0, 0, 0, 0};      // pairs, apart, d0, d1, dlogstd, KL(own || v), KL(v || own), max dev
            if (counted) {
                const float4 v = *reinterpret_cast<const float4*>(verdict + (idx * K + jj) * 4);
                const float d0 = fabsf(__fsub_rn(v.x, own.x)), d1 = fabsf(__fsub_rn(v.y, own.y));
                const float ds = __fadd_rn(fabsf(__fsub_rn(v.z, own.z)), fabsf(__fsub_rn(v.w, own.w)));
                w[1] = d0 > delta_steer || d1 > delta_throttle;
                w[2] = q16(d0);
                w[3] = q16(d1);
                w[4] = q16(ds);
                w[5] = q16(jury_kl(own, v));
                w[6] = q16(jury_kl(v, own));
                w[7] = q16(fmaxf(d0, d1));
            }
            L.serve(JuryWords{}, counted, w, out, [&](int m) { return ((size_t)L.g * K + m) * K + jj; });
        }
    });
}

hipError_t launch_jury_tally(const uint8_t* flags, const float* dist, const float* verdict, const int32_t* seat, const int32_t* group,
                             const int32_t* judges, int32_t E, int32_t N, int32_t K, int32_t G, float delta_steer, float delta_throttle,
                             int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(jury_tally_kernel, tally_grid(E), dim3(256), 0, stream, flags, dist, verdict, seat, group, judges, E, N, K, G, delta_steer,
                       delta_throttle, out);
    return hipGetLastError();
}

hipError_t launch_certify_tally(const uint8_t* flags, const float* bounds, const int32_t* seat, const int32_t* group, const int32_t* level_of,
                                const float* levels, int32_t E, int32_t N, int32_t K, int32_t G, int32_t L, int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(certify_tally_kernel, tally_grid(E), dim3(256), 0, stream, flags, bounds, seat, group, level_of, levels, E, N, K, G, L, out);
    return hipGetLastError();
}

hipError_t launch_seat_tally(const uint8_t* flags, const float* rew, const int32_t* seat, const int32_t* group, int32_t E, int32_t N,
                             int32_t K, int32_t G, int64_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(seat_tally_kernel, tally_grid(E), dim3(256), 0, stream, flags, rew, seat, group, E, N, K, G, out);
    return hipGetLastError();
}

}  // namespace copo
