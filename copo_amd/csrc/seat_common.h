// The tallies of seated evaluation: the launches of seat_kernels.hip that capi.hip calls, and the device code every tally kernel shares
// (also influence_kernels.hip): the wave walk, the emission of a cell's words, the quantiser.
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

// one step's integrated gradients folded per (scene group, bank member) into words[G][K][COPO_ATTRIB_TALLY_WORDS] and
// cols[G][K][2][in_dim] (one launch)
hipError_t launch_attrib_tally(const uint8_t* flags, const float* attr, const float* heads, const int32_t* seat, const int32_t* group,
                               int32_t E, int32_t N, int32_t K, int32_t G, int32_t in_dim, int64_t* words, int64_t* cols, hipStream_t stream);

// Every tally's geometry: one wave per scene, four scenes per 256-thread workgroup.
constexpr int TALLY_SCENES_PER_WG = 4;
inline dim3 tally_grid(int32_t E) { return dim3((E + TALLY_SCENES_PER_WG - 1) / TALLY_SCENES_PER_WG); }

#ifdef __HIPCC__
// ---- device side of the tallies (seat_kernels.hip, influence_kernels.hip): 64-bit wave reductions, the one quantisation, the KL and
// the one wave walk ----
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

// q of the header for an fp32 value, rint(min(max(x, lo), 1024) * 65536): NaN counts as 0, the clamp makes the product exact in fp32 (a
// power of two, no overflow), so the one rounding is rintf's, half to even.  `lo` is -1024 for the reward and 0 for every distance and
// width.  (The certify tally quantises finite values only -- its `finite` flag --, so the NaN test changes none of its bits.)
__device__ inline int64_t q16(float x, float lo = 0.0f) {
    if (x != x) return 0;
    return (int64_t)rintf(fminf(fmaxf(x, lo), 1024.0f) * 65536.0f);
}
// ... and for a float64 value (the two divergences)
__device__ inline int64_t q16(double x) {
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

// ---- the wave walk of every tally.  A tally describes its eight words by their kinds and keeps only what a lane contributes. ----
enum { W_COUNT, W_SUM, W_MAX };      // lanes with a non-zero value (a ballot's popcount) / the sum of the values / their maximum
template <int... KINDS>
struct WordKinds {};

// Word w of the lanes `mine`: the WHOLE wave reduces (a ballot or a butterfly), then lane w keeps the result.
template <int KIND>
__device__ __forceinline__ void wave_word(int lane, int w, bool mine, int64_t v, int64_t& word, bool& is_max) {
    int64_t r;
    if constexpr (KIND == W_COUNT) r = __popcll(__ballot(mine && v != 0));
    else if constexpr (KIND == W_SUM) r = wave_sum_i64(mine ? v : 0);
    else r = wave_max_i64(mine ? v : 0);
    if (lane == w) {
        word = r;
        is_max = KIND == W_MAX;
    }
}

// One lane's slot in one round of the walk.
struct SeatLane {
    int lane, g, s;            // the lane, the scene's group (0 <= g < G) and the slot's member (-1 beyond the scene's N slots)
    size_t idx;                // e * N + n, clamped to the scene's first slot where n >= N
    bool seated;               // 0 <= s < K

    // The members among the `counted` lanes (seated ones; the ballot is uniform over the wave) served one after the other: the first lane
    // not yet served names a member m, a ballot collects m's lanes, lane i ends up with word i of their values v[] by the word's kind and
    // adds it -- a W_MAX word by atomicMax -- to word i of cell `cell(m)` of `out` unless it is zero.
    template <int... KINDS, class Cell>
    __device__ __forceinline__ void serve(WordKinds<KINDS...>, bool counted, const int64_t (&v)[sizeof...(KINDS)], int64_t* out, Cell cell) const {
        constexpr int WORDS = sizeof...(KINDS);
        uint64_t todo = __ballot(counted);
        while (todo) {
            const int m = __shfl(s, __ffsll((unsigned long long)todo) - 1);
            const bool mine = counted && s == m;
            todo &= ~__ballot(mine);
            int64_t word = 0;
            bool is_max = false;
            int w = 0;                         // (a constant in every term of the fold: the kinds are the template's)
            ((wave_word<KINDS>(lane, w, mine, v[w], word, is_max), ++w), ...);
            if (lane < WORDS && word != 0) {
                unsigned long long* at = reinterpret_cast<unsigned long long*>(out) + (size_t)cell(m) * WORDS + lane;
                if (is_max) atomicMax(at, (unsigned long long)word);
                else atomicAdd(at, (unsigned long long)word);
            }
        }
    }
};

// One wave per scene (the caller's launch: tally_grid x 256 threads), slot = lane + 64 j: `round(SeatLane)` once per round of 64 slots
// of every scene e < E whose group is inside [0, G).  Both early returns take the whole wave; there is no barrier in a tally.
template <class Round>
__device__ __forceinline__ void seat_walk(const int32_t* __restrict__ seat, const int32_t* __restrict__ group, int32_t E, int32_t N, int32_t K,
                                          int32_t G, Round round) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * TALLY_SCENES_PER_WG + wave;
    if (e >= E) return;
    const int g = group[e];
    if (g < 0 || g >= G) return;
    for (int j = 0; 64 * j < N; ++j) {
        const int n = lane + 64 * j;
        const size_t idx = (size_t)e * N + (n < N ? n : 0);
        const int s = n < N ? seat[idx] : -1;
        round(SeatLane{lane, g, s, idx, s >= 0 && s < K});
    }
}
#endif

}  // namespace copo
