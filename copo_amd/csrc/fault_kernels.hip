// Fault injection (copo_fault_obs, copo_fault_act; include/copo_hip.h): noisy sensors between the simulator's
// observation and the policy, noisy and sticky actuators between the policy's action and the simulator.  Both kernels are stateless
// (the caller owns `prev` and `tick`), one launch each, no allocation, no host read, no atomics: they sit inside a captured graph.
//
// fault_obs_kernel streams obs -> obs_seen.  ONE WAVE PER ROW, four rows per 256-thread workgroup, column = lane + 64 j, and not a flat
// index over E N O elements, for three reasons:
//   * O is odd on most maps (91 on the Intersection), so a row starts on a 4-byte boundary and no 8- or 16-byte access is possible without
//     peeling both ends of both buffers; the widest access left is one dword per lane.  With a wave on a row, consecutive lanes still
//     read and write consecutive dwords: 256 contiguous bytes per wave-instruction, the shape that streams at the plain-store rate.
//     The price is the tail: at O = 91 the second round has 27 of 64 lanes (71 % of the lanes, 100 % of the bytes useful), and the
//     lines a row shares with its neighbours are touched by two waves of the same workgroup, which the L2 absorbs.
//   * everything that depends on the row alone is uniform over the wave: the scene (one division), seat, group, level and its words,
//     the tick, and the first four of the six mixing rounds of every hash_rng draw (seed, seed, row, tick).  The wave index goes
//     through readfirstlane so that the compiler keeps these in scalar registers and loads.  A lane pays two rounds per draw, (c,
//     stream), instead of six; a flat index would pay two divisions, five dependent loads and six rounds per element, and at three
//     draws per beam that arithmetic, not the memory, would bound the kernel.
//   * the branches on the level (pass through, no dropout, no noise) do not diverge.
// fault_act_kernel has one thread per row (16 bytes of state): nothing is shared, so nothing races.
//
// Every float operation that the compiler could contract is written with __fmul_rn / __fadd_rn / __fsub_rn, and a clamp is two
// comparisons (clipf), so the sign of a zero and every rounding are the ones tests/fault_numpy.py restates in float32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sim_common.h"
#include "sim_math.h"
#include "fault_common.h"

namespace copo {

namespace {

constexpr int ROWS_PER_WG = 4;       // waves of a 256-thread workgroup

// hash_rng(seed, a, b, c, stream) = fault_hash_tail(fault_hash_head(seed, a, b), c, stream): the split of sim_math.h's chain after its
// fourth round
__device__ __forceinline__ uint32_t fault_hash_head(uint64_t seed, uint32_t a, uint32_t b) {
    uint32_t h = mix32((uint32_t)seed + 0x9E3779B9u);
    h = mix32(h ^ (uint32_t)(seed >> 32));
    h = mix32(h ^ a);
    return mix32(h ^ b);
}

__device__ __forceinline__ uint32_t fault_hash_tail(uint32_t head, uint32_t c, uint32_t stream) { return mix32(mix32(head ^ c) ^ stream); }

// The standard-normal stand-in: the four 16-bit halves of two hashes summed (an Irwin-Hall sum: mean 131070, variance (2^32 - 1) / 3),
// centred and scaled.  The conversion and the subtraction are exact (S < 2^18), the multiply is the one rounding.  |z| <= 3.4641.
__device__ __forceinline__ float fault_z(uint32_t h1, uint32_t h2) {
    const uint32_t S = (h1 & 0xffffu) + (h1 >> 16) + (h2 & 0xffffu) + (h2 >> 16);
    return __fmul_rn(__fsub_rn((float)S, kFaultZOffset), kFaultZScale);
}

// the level of row e * N + n, or -1: the row passes through
__device__ __forceinline__ int fault_level(int row, int N, const int32_t* __restrict__ seat, const int32_t* __restrict__ group, int K, int G,
                                           const int32_t* __restrict__ level_of, int L) {
    const int s = seat[row], g = group[row / N];
    if (s < 0 || s >= K || g < 0 || g >= G) return -1;
    const int l = level_of[(size_t)g * K + s];
    return (l < 0 || l >= L) ? -1 : l;
}

}  // namespace

__global__ __launch_bounds__(256) void fault_obs_kernel(const float* __restrict__ obs, float* __restrict__ obs_seen, int32_t EN, int32_t N,
                                                        int32_t O, int32_t col_lo, int32_t col_hi, const int32_t* __restrict__ seat,
                                                        const int32_t* __restrict__ group, int32_t K, int32_t G,
                                                        const int32_t* __restrict__ level_of, const uint32_t* __restrict__ levels, int32_t L,
                                                        const int32_t* __restrict__ tick, uint64_t fault_seed) {
    const int lane = threadIdx.x & 63;
    const int64_t row64 = (int64_t)blockIdx.x * ROWS_PER_WG + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row64 >= EN) return;                   // (the whole wave; there is no barrier in this kernel)
    const int row = (int)row64;
    const float* __restrict__ src = obs + (size_t)row * O;
    float* __restrict__ dst = obs_seen + (size_t)row * O;
    const int l = fault_level(row, N, seat, group, K, G, level_of, L);
    float sigma = 0.0f, dvalue = 0.0f;
    uint32_t thr = 0u;
    if (l >= 0) {
        const uint32_t* w = levels + (size_t)l * COPO_FAULT_LEVEL_WORDS;
        sigma = __uint_as_float(w[FAULT_W_LIDAR_SIGMA]);
        thr = w[FAULT_W_DROPOUT_THR];
        dvalue = __uint_as_float(w[FAULT_W_DROPOUT_VALUE]);
    }
    const bool noisy = sigma != 0.0f;
    if (thr == 0u && !noisy) {                 // the identity level and every pass-through row: a copy
        for (int c = lane; c < O; c += 64) dst[c] = src[c];
        return;
    }
    const uint32_t head = fault_hash_head(fault_seed, (uint32_t)row, (uint32_t)tick[row]);
    for (int c = lane; c < O; c += 64) {
        float x = src[c];
        if (c >= col_lo && c < col_hi) {
            const uint32_t b = (uint32_t)(c - col_lo);
            if (thr != 0u && (fault_hash_tail(head, b, RNG_FAULT_DROP) >> 8) < thr) {
                x = dvalue;
            } else if (noisy) {
                const float z = fault_z(fault_hash_tail(head, b, RNG_FAULT_LIDAR_A), fault_hash_tail(head, b, RNG_FAULT_LIDAR_B));
                x = clipf(__fadd_rn(x, __fmul_rn(sigma, z)), 0.0f, 1.0f);
            }
        }
        dst[c] = x;
    }
}

__global__ __launch_bounds__(256) void fault_act_kernel(float* __restrict__ act, float* __restrict__ prev,
                                                        const uint8_t* __restrict__ flags_prev, int32_t EN, int32_t N,
                                                        const int32_t* __restrict__ seat, const int32_t* __restrict__ group, int32_t K,
                                                        int32_t G, const int32_t* __restrict__ level_of,
                                                        const uint32_t* __restrict__ levels, int32_t L, int32_t* __restrict__ tick,
                                                        uint64_t fault_seed) {
    const int64_t row64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row64 >= EN) return;
    const int row = (int)row64;
    const size_t i0 = (size_t)row * 2;
    const int32_t t = tick[row];
    float a0 = act[i0], a1 = act[i0 + 1];
    const int l = fault_level(row, N, seat, group, K, G, level_of, L);
    if (l >= 0) {
        const uint32_t* w = levels + (size_t)l * COPO_FAULT_LEVEL_WORDS;
        const float sigma = __uint_as_float(w[FAULT_W_ACT_SIGMA]);
        const uint32_t thr = w[FAULT_W_STICKY_THR];
        if (flags_prev && thr != 0u) {
            // the slot holds the agent it held a step ago: that agent acted, did not terminate, nobody was spawned into the slot and the
            // scene was not reset (SPEC.md, steps (5), (6) and (8) of a simulator step)
            const uint32_t f = flags_prev[row];
            const bool same = (f & COPO_F_ACTED) != 0u && (f & (COPO_F_DONE | COPO_F_SPAWNED | COPO_F_ENV_RESET)) == 0u;
            if (same && (hash_rng(fault_seed, (uint32_t)row, (uint32_t)t, 0u, RNG_FAULT_STICKY) >> 8) < thr) {
                a0 = prev[i0];
                a1 = prev[i0 + 1];
            }
        }
        if (sigma != 0.0f) {
            const uint32_t head = fault_hash_head(fault_seed, (uint32_t)row, (uint32_t)t);
            const float z0 = fault_z(fault_hash_tail(head, 0u, RNG_FAULT_ACT_A), fault_hash_tail(head, 0u, RNG_FAULT_ACT_B));
            const float z1 = fault_z(fault_hash_tail(head, 1u, RNG_FAULT_ACT_A), fault_hash_tail(head, 1u, RNG_FAULT_ACT_B));
            a0 = clipf(__fadd_rn(a0, __fmul_rn(sigma, z0)), -1.0f, 1.0f);
            a1 = clipf(__fadd_rn(a1, __fmul_rn(sigma, z1)), -1.0f, 1.0f);
        }
        act[i0] = a0;
        act[i0 + 1] = a1;
    }
    prev[i0] = a0;                             // every row, pass-through rows included
    prev[i0 + 1] = a1;
    tick[row] = (int32_t)((uint32_t)t + 1u);
}

hipError_t launch_fault_obs(const float* obs, float* obs_seen, int32_t E, int32_t N, int32_t O, int32_t col_lo, int32_t col_hi,
                            const int32_t* seat, const int32_t* group, int32_t K, int32_t G, const int32_t* level_of,
                            const uint32_t* levels, int32_t L, const int32_t* tick, uint64_t fault_seed, hipStream_t stream) {
    const int32_t EN = E * N;
    hipLaunchKernelGGL(fault_obs_kernel, dim3((EN + ROWS_PER_WG - 1) / ROWS_PER_WG), dim3(256), 0, stream, obs, obs_seen, EN, N, O, col_lo,
                       col_hi, seat, group, K, G, level_of, levels, L, tick, fault_seed);
    return hipGetLastError();
}

hipError_t launch_fault_act(float* act, float* prev, const uint8_t* flags_prev, int32_t E, int32_t N, const int32_t* seat,
                            const int32_t* group, int32_t K, int32_t G, const int32_t* level_of, const uint32_t* levels, int32_t L,
                            int32_t* tick, uint64_t fault_seed, hipStream_t stream) {
    const int32_t EN = E * N;
    hipLaunchKernelGGL(fault_act_kernel, dim3((EN + 255) / 256), dim3(256), 0, stream, act, prev, flags_prev, EN, N, seat, group, K, G,
                       level_of, levels, L, tick, fault_seed);
    return hipGetLastError();
}

}  // namespace copo
