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

// Attribution tally (copo_attrib_tally): one step's integrated gradients (copo_ig_obs_seats_f32) folded per (scene
// group, member).  A slot counts by the seat tally's rule for `acted`; it is attributed where heads[..][6] == 1.  Every value is
// quantised once, q32(v) = llrint(min(|v|, 2^20) * 2^32) in float64 from the fp32 value (NaN counts as 0), so words and columns are
// integers and the result does not depend on the order.  The eight words go through the one walk.  The columns do not: a member's rows
// of ALL rounds of the scene are collected first (up to COPO_SEAT_MAX_SLOTS / 64 ballots), then the lanes take 64 adjacent (head,
// column) cells at a time and walk the member's rows -- coalesced reads, a private sum per lane, and one atomic per (scene, member
// seated in it, head, column) at the most.
using AttribWords = WordKinds<W_COUNT, W_SUM, W_SUM, W_SUM, W_SUM, W_MAX, W_COUNT, W_COUNT>;
constexpr int ATTRIB_ROUNDS = COPO_SEAT_MAX_SLOTS / 64;

__device__ inline int64_t q32(float v) {
    if (v != v) return 0;
    return (int64_t)llrint(fmin(fabs((double)v), 1048576.0) * 4294967296.0);
}

__global__ __launch_bounds__(256) void attrib_tally_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ attr,
                                                           const float* __restrict__ heads, const int32_t* __restrict__ seat,
                                                           const int32_t* __restrict__ group, int32_t E, int32_t N, int32_t K, int32_t G,
                                                           int32_t D, int64_t* __restrict__ words, int64_t* __restrict__ cols) {
    seat_walk(seat, group, E, N, K, G, [&](const SeatLane& L) {
        const bool counted = L.seated && ((uint32_t)flags[L.idx] & COPO_F_ACTED) != 0u;
        const float* h = heads + L.idx * COPO_IG_HEAD_WORDS;
        const bool valid = counted && h[6] == 1.0f;
        int64_t v[COPO_ATTRIB_TALLY_WORDS] = {valid, 0, 0, 0, 0, 0, !valid, 0};      // attributed, |delta| x 2, |gap| x 2, max |gap|, listed only, 0
        if (valid) {
            v[1] = q32(__fsub_rn(h[0], h[2]));
            v[2] = q32(__fsub_rn(h[1], h[3]));
            v[3] = q32(h[4]);
            v[4] = q32(h[5]);
            v[5] = v[3] > v[4] ? v[3] : v[4];
        }
        L.serve(AttribWords{}, counted, v, words, [&](int m) { return (size_t)L.g * K + m; });
    });
    // ---- the columns (the scene and group tests are seat_walk's: both take the whole wave) ----
    const int lane = threadIdx.x & 63, e = blockIdx.x * TALLY_SCENES_PER_WG + (threadIdx.x >> 6);
    if (e >= E) return;
    const int g = group[e];
    if (g < 0 || g >= G) return;
    int s_j[ATTRIB_ROUNDS];
    uint64_t todo[ATTRIB_ROUNDS];
#pragma unroll
    for (int j = 0; j < ATTRIB_ROUNDS; ++j) {
        const int n = lane + 64 * j;
        const size_t idx = (size_t)e * N + (n < N ? n : 0);
        const int s = n < N ? seat[idx] : -1;
        const bool ok = s >= 0 && s < K && ((uint32_t)flags[idx] & COPO_F_ACTED) != 0u && heads[idx * COPO_IG_HEAD_WORDS + 6] == 1.0f;
        s_j[j] = ok ? s : -1;
        todo[j] = __ballot(ok);
    }
    const int W = 2 * D;
    for (;;) {
        int m = -1;                        // the next member: the first lane of the first round that is not served yet (uniform)
#pragma unroll
        for (int j = 0; j < ATTRIB_ROUNDS; ++j) {
            const int first = __shfl(s_j[j], todo[j] ? __ffsll((unsigned long long)todo[j]) - 1 : 0);
            if (m < 0 && todo[j]) m = first;
        }
        if (m < 0) break;
        uint64_t mask[ATTRIB_ROUNDS];
#pragma unroll
        for (int j = 0; j < ATTRIB_ROUNDS; ++j) {
            mask[j] = __ballot(s_j[j] == m);
            todo[j] &= ~mask[j];
        }
        for (int c0 = 0; c0 < W; c0 += 64) {
            const int c = c0 + lane;
            int64_t acc = 0;
#pragma unroll
            for (int j = 0; j < ATTRIB_ROUNDS; ++j)
                for (uint64_t mk = mask[j]; mk; mk &= mk - 1) {
                    const size_t row = (size_t)e * N + 64 * j + (__ffsll((unsigned long long)mk) - 1);
                    if (c < W) acc += q32(attr[row * W + c]);
                }
            if (c < W && acc != 0)
                atomicAdd(reinterpret_cast<unsigned long long*>(cols) + ((size_t)g * K + m) * W + c, (unsigned long long)acc);
        }
    }
}

hipError_t launch_attrib_tally(const uint8_t* flags, const float* attr, const float* heads, const int32_t* seat, const int32_t* group,
                               int32_t E, int32_t N, int32_t K, int32_t G, int32_t in_dim, int64_t* words, int64_t* cols, hipStream_t stream) {
    hipLaunchKernelGGL(attrib_tally_kernel, tally_grid(E), dim3(256), 0, stream, flags, attr, heads, seat, group, E, N, K, G, in_dim, words, cols);
    return hipGetLastError();
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
