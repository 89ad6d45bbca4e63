// Shared declaration of the seat tally (seat_kernels.hip) and its C entry point (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace copo {

// cross-play: one step's flags / rewards folded per (scene group, bank member) into out[G][K][COPO_SEAT_WORDS] (one launch)
hipError_t launch_seat_tally(const uint8_t* flags, const float* rew, const int32_t* seat, const int32_t* group, int32_t E, int32_t N,
                             int32_t K, int32_t G, int64_t* out, hipStream_t stream);

// certified bounds of one step folded per (scene group, bank member) into out[G][K][COPO_CERT_TALLY_WORDS] (one launch)
hipError_t launch_certify_tally(const uint8_t* flags, const float* bounds, const int32_t* seat, const int32_t* group, const int32_t* level_of,
                                const float* levels, int32_t E, int32_t N, int32_t K, int32_t G, int32_t L, int64_t* out, hipStream_t stream);

// one step's jury verdicts folded per (scene group, driving member, judging member) into out[G][K][K][COPO_JURY_WORDS] (one launch)
hipError_t launch_jury_tally(const uint8_t* flags, const float* dist, const float* verdict, const int32_t* seat, const int32_t* group,
                             const int32_t* judges, int32_t E, int32_t N, int32_t K, int32_t G, float delta_steer, float delta_throttle,
                             int64_t* out, hipStream_t stream);

#ifdef __HIPCC__
// ---- device helpers of the tallies (seat_kernels.hip, influence_kernels.hip): 64-bit wave reductions, the one quantisation and the KL ----
__device__ inline int64_t wave_sum_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int32_t lo = __shfl_xor((int32_t)(uint32_t)((uint64_t)v & 0xffffffffu), o);
        const int32_t hi = __shfl_xor((int32_t)(uint32_t)((uint64_t)v >> 32), o);
        v += (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
    }
    return v;
}

__device__ inline int64_t wave_max_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int32_t lo = __shfl_xor((int32_t)(uint32_t)((uint64_t)v & 0xffffffffu), o);
        const int32_t hi = __shfl_xor((int32_t)(uint32_t)((uint64_t)v >> 32), o);
        const int64_t w = (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
        v = w > v ? w : v;
    }
    return v;
}

// q of the header for an fp32 value: NaN counts as 0, the clamp makes the product exact, rintf rounds once
__device__ inline int64_t jury_q16(float x) {
    if (x != x) return 0;
    return (int64_t)rintf(fminf(fmaxf(x, 0.0f), 1024.0f) * 65536.0f);
}
// ... and for a float64 value (the two divergences)
__device__ inline int64_t jury_q16(double x) {
    if (x != x) return 0;
    return (int64_t)rint(fmin(fmax(x, 0.0), 1024.0) * 65536.0);
}

// KL(p || q) of two diagonal Gaussians over the two action axes, (mean, log-std) in fp32, evaluated in float64 as the header states it;
// no contraction, so that the float64 restatement of the tests differs by the last ulp of exp at the most
__device__ inline double jury_kl(const float4& p, const float4& q) {
#pragma clang fp contract(off)
    const double mp[2] = {p.x, p.y}, sp[2] = {p.z, p.w}, mq[2] = {q.x, q.y}, sq[2] = {q.z, q.w};
    double kl = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const double dm = mp[a] - mq[a];
        kl = kl + ((sq[a] - sp[a]) + (0.5 * (exp(2.0 * (sp[a] - sq[a])) + dm * dm * exp(-2.0 * sq[a])) - 0.5));
    }
    return kl;
}
#endif

}  // namespace copo
