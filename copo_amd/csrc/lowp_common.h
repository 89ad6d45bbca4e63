// Low-precision policy forward: the number formats, the packed weight image and the launchers that
// lowp_kernels.hip defines and capi_lowp.hip checks arguments for.  The rounding functions are integer arithmetic in plain C++, compiled
// for the device (the pack and the forward kernel) and for the host (copo_debug_lowp_round, the checker of the CPU tests) from this text.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/copo_hip.h"

namespace copo {

// ---- formats ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t lowp_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}
__host__ __device__ inline float lowp_float(uint32_t u) {
    float x;
    memcpy(&x, &u, 4);
    return x;
}

// bfloat16, round to nearest even (the bf16r of the learner's bfloat16 operand mode, on the upper half word)
__host__ __device__ inline uint16_t bf16_encode(float x) {
    uint32_t u = lowp_bits(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);      // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__host__ __device__ inline float bf16_decode(uint16_t h) { return lowp_float((uint32_t)h << 16); }

// OCP e4m3fn: 1 + 4 + 3 bits, bias 7, no infinities, largest value 448 = 0x7e, 0x7f is NaN; subnormals m 2^-9 are kept.
// |x| > 448 (infinities too) is clamped to 448 first, then the value is rounded to nearest even.
__host__ __device__ inline uint8_t e4m3_encode(float x) {
    const uint32_t u = lowp_bits(x), sign = (u >> 24) & 0x80u;
    uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint8_t)(sign | 0x7fu);
    if (a > 0x43e00000u) a = 0x43e00000u;                 // 448
    const int e = (int)(a >> 23) - 127;
    if (e >= -6) {                                        // normal in e4m3: 23 -> 3 mantissa bits (a carry moves into the exponent)
        a += 0x7ffffu + ((a >> 20) & 1u);
        return (uint8_t)(sign | ((a >> 20) - (120u << 3)));
    }
    const int shift = 14 - e;                             // the value in units of 2^-9 is mant 2^-shift, shift >= 21
    if (shift > 24 || (a >> 23) == 0) return (uint8_t)sign;
    const uint32_t mant = (a & 0x7fffffu) | 0x800000u;
    const uint32_t q = (mant + (1u << (shift - 1)) - 1u + ((mant >> shift) & 1u)) >> shift;      // 0..8 (8 = the smallest normal, 0x08)
    return (uint8_t)(sign | q);
}
__host__ __device__ inline float e4m3_decode(uint8_t c) {
    const uint32_t sign = (uint32_t)(c & 0x80u) << 24, e = (c >> 3) & 15u, m = c & 7u;
    if ((c & 0x7fu) == 0x7fu) return lowp_float(sign | 0x7fc00000u);
    if (e == 0) return lowp_float(sign | lowp_bits((float)m * 0.001953125f));      // m 2^-9, exact
    return lowp_float(sign | ((e + 120u) << 23) | (m << 20));
}

__host__ __device__ inline float lowp_round(int fmt, float x) {
    return fmt == COPO_LOWP_E4M3 ? e4m3_decode(e4m3_encode(x)) : bf16_decode(bf16_encode(x));
}

// The scale of an e4m3 weight row of largest magnitude `amax`: the smallest power of two s with amax / s <= 448, 2^ceil(log2(amax / 448)),
// from the bits of amax = m 2^E: m <= 1.75 gives 2^(E - 8), else 2^(E - 7); kept a normal number; 1 for a zero row (and a NaN / inf one).
__host__ __device__ inline float e4m3_row_scale(float amax) {
    const uint32_t a = lowp_bits(amax) & 0x7fffffffu;
    if (a == 0 || a >= 0x7f800000u) return 1.0f;
    int e = (int)(a >> 23) - 127 - ((a & 0x7fffffu) <= 0x600000u ? 8 : 7);
    if ((a >> 23) == 0) e = -126;
    e = e < -126 ? -126 : (e > 127 ? 127 : e);
    return lowp_float((uint32_t)(e + 127) << 23);
}

// ---- packed image of one member (bytes) --------------------------------------------------------------------------------------------
// q1 [H][K1P] and q2 [H][H] elements of the format, unit-major with k contiguous, K1P = in_dim rounded up to 32 and zero beyond in_dim;
// then fp32: q3 [4][H], s1 [H], s2 [H], s3 [4], b1 [H], b2 [H], b3 [4].
struct LowpLay {
    int H, K1, K1P, esz;
    size_t q1, q2, f32;
    __host__ __device__ LowpLay(int hidden, int in_dim, int fmt)
        : H(hidden), K1(in_dim), K1P((in_dim + 31) / 32 * 32), esz(fmt == COPO_LOWP_E4M3 ? 1 : 2), q1(0), q2((size_t)H * K1P * esz),
          f32(q2 + (size_t)H * H * esz) {}
    __host__ __device__ size_t q3() const { return f32; }
    __host__ __device__ size_t s(int l) const { return f32 + 4 * (size_t)(4 * H + (l - 1) * H); }                  // l = 1, 2, 3
    __host__ __device__ size_t b(int l) const { return f32 + 4 * (size_t)(6 * H + 4 + (l - 1) * H); }
    __host__ __device__ size_t total() const { return f32 + 4 * (size_t)(8 * H + 8); }
};

struct LowpFwdArgs {
    const uint8_t* packed;
    int64_t packed_stride;     // bytes
    const int64_t* rows;       // [n_members][cap]
    const int32_t* counts;     // [n_members]
    int64_t cap, n_out;
    const float* obs_src;      // [n_out][in_dim]
    int32_t in_dim;
    float* dist_inputs;        // [n_out][4] or NULL
    const float* eps;          // [n_out][2] or NULL: no sampling
    float* action;
    float* logp;
    float* clipped;            // or NULL
};

size_t lowp_fwd_lds_bytes(int hidden, int in_dim, int fmt);
hipError_t launch_lowp_pack(const copo_ppo_cfg& c, const float* theta, int64_t member_stride, int32_t n_members, int32_t fmt, uint8_t* packed,
                            int64_t packed_stride, hipStream_t stream);
hipError_t launch_lowp_forward(int hidden, int32_t fmt, int32_t n_members, const LowpFwdArgs& a, hipStream_t stream);

}  // namespace copo
