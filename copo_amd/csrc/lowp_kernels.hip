// Low-precision policy forward of a seated bank (eval/precision.py): the pack of a bank's parameters into the
// bfloat16 / e4m3 image of lowp_common.h, and lowp_fwd_kernel, the forward of the policy net on 16 listed rows per workgroup with both
// hidden layers on v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x32_fp8_fp8.  A unit of its own: none of the learner's kernels
// (learn_fused.hip) is compiled with it, so none of them moves.  What it restates from there: the seat mode's list rules (learn_seat.inc,
// seat_row_at), tanh_fast (learn_gemm.inc) and the sampling epilogue of mlp_fwd_kernel (learn_rowpass.inc), the last two under the
// contraction mode of that unit so that equal inputs give equal bits.
#include <type_traits>

#include "lowp_common.h"

namespace copo {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));

constexpr int LOWP_ROWS = 16, LOWP_THREADS = 256, LOWP_PAD = 8;      // rows per workgroup; pad of an LDS tile row, in elements
constexpr float kLowpLog2Pi = 1.8378770664093453f;

__device__ __forceinline__ float lowp_tanh_fast(float x) {
#pragma clang fp contract(fast)
    const float x2 = x * x;
    const float p = x * (1.0f + x2 * (-0.33333334f + x2 * (0.13333334f + x2 * (-0.053968254f + x2 * 0.021869488f))));
    const float r = 1.0f - 2.0f * __frcp_rn(__expf(2.0f * x) + 1.0f);
    return fabsf(x) < 0.3f ? p : r;
}

// ---- pack: one workgroup of 64 threads per (output unit, layer, member) ------------------------------------------------------------
__global__ void __launch_bounds__(64) lowp_pack_kernel(copo_ppo_cfg c, const float* theta, int64_t member_stride, int32_t fmt, uint8_t* packed,
                                                       int64_t packed_stride) {
    const int H = c.hidden, K1 = c.pol.in_dim, layer = blockIdx.y + 1, u = blockIdx.x, lane = threadIdx.x;
    if (layer == 3 && u >= 4) return;
    const LowpLay L(H, K1, fmt);
    const float* th = theta + (size_t)blockIdx.z * member_stride;
    uint8_t* img = packed + (size_t)blockIdx.z * packed_stride;
    const int K = layer == 1 ? K1 : H, KP = layer == 1 ? L.K1P : H;
    const float* w = th + (layer == 1 ? c.pol.w1 : layer == 2 ? c.pol.w2 : c.pol.w3) + (size_t)u * K;
    const float bias = th[(layer == 1 ? c.pol.b1 : layer == 2 ? c.pol.b2 : c.pol.b3) + u];
    float amax = 0.0f;
    for (int k = lane; k < K; k += 64) amax = fmaxf(amax, fabsf(w[k]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    const float s = fmt == COPO_LOWP_E4M3 ? e4m3_row_scale(amax) : 1.0f;
    if (layer == 3) {
        float* q3 = reinterpret_cast<float*>(img + L.q3()) + (size_t)u * H;
        for (int k = lane; k < H; k += 64) q3[k] = lowp_round(fmt, w[k] / s);
    } else if (fmt == COPO_LOWP_E4M3) {
        uint8_t* q = img + (layer == 1 ? L.q1 : L.q2) + (size_t)u * KP;
        for (int k = lane; k < KP; k += 64) q[k] = k < K ? e4m3_encode(w[k] / s) : (uint8_t)0;
    } else {
        uint16_t* q = reinterpret_cast<uint16_t*>(img + (layer == 1 ? L.q1 : L.q2)) + (size_t)u * KP;
        for (int k = lane; k < KP; k += 64) q[k] = k < K ? bf16_encode(w[k]) : (uint16_t)0;
    }
    if (lane == 0) {
        reinterpret_cast<float*>(img + L.s(layer))[u] = s;
        // bfloat16: the learner's bfloat16 operand mode rounds its biases too, and the two describe one function; e4m3 keeps them fp32
        reinterpret_cast<float*>(img + L.b(layer))[u] = fmt == COPO_LOWP_E4M3 ? bias : lowp_round(COPO_LOWP_BF16, bias);
    }
}

hipError_t launch_lowp_pack(const copo_ppo_cfg& c, const float* theta, int64_t member_stride, int32_t n_members, int32_t fmt, uint8_t* packed,
                            int64_t packed_stride, hipStream_t stream) {
    hipLaunchKernelGGL(lowp_pack_kernel, dim3(c.hidden, 3, n_members), dim3(64), 0, stream, c, theta, member_stride, fmt, packed, packed_stride);
    return hipGetLastError();
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
template <bool FP8> struct LowpFmt;
template <> struct LowpFmt<false> {
    typedef uint16_t E;
    typedef uint4 Frag;      // 8 elements
    static __device__ __forceinline__ E enc(float x) { return bf16_encode(x); }
    static __device__ __forceinline__ float dec(E h) { return bf16_decode(h); }
    static __device__ __forceinline__ Frag pack8(const float* v) {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = (uint32_t)bf16_encode(v[2 * j]) | ((uint32_t)bf16_encode(v[2 * j + 1]) << 16);
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
    static __device__ __forceinline__ v4f mfma(const Frag& a, const Frag& b, v4f acc) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), acc, 0, 0, 0);
    }
};
template <> struct LowpFmt<true> {
    typedef uint8_t E;
    typedef uint2 Frag;
    static __device__ __forceinline__ E enc(float x) { return e4m3_encode(x); }
    static __device__ __forceinline__ float dec(E h) { return e4m3_decode(h); }
    static __device__ __forceinline__ Frag pack8(const float* v) {
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j >> 2] |= (uint32_t)e4m3_encode(v[j]) << (8 * (j & 3));
        return make_uint2(w[0], w[1]);
    }
    static __device__ __forceinline__ v4f mfma(const Frag& a, const Frag& b, v4f acc) {
        return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(__builtin_bit_cast(long, a), __builtin_bit_cast(long, b), acc, 0, 0, 0);
    }
};

// One hidden layer of the tile: acc[t] += tile [16][K] x q [H][K]^T on the 16 columns (wave NT + t) 16 .. + 16.  Lane l holds row l & 15 of
// the tile (A) and column l & 15 of the weights (B), both at k = k0 + 8 (l >> 4) .. + 8: one aligned LDS read and one aligned global load.
template <int NT, bool FP8>
__device__ __forceinline__ void lowp_layer(const typename LowpFmt<FP8>::E* tile, int TS, const uint8_t* q, int K, int wave, int lane, v4f* acc) {
    typedef LowpFmt<FP8> F;
    typedef typename F::Frag Frag;
    typedef typename F::E E;
    const int ln = lane & 15, lj = lane >> 4;
    const E* ap = tile + ln * TS + 8 * lj;
    const E* bp = reinterpret_cast<const E*>(q) + (size_t)(wave * NT * 16 + ln) * K + 8 * lj;
    if constexpr (FP8) {
        // The fp8 instruction does not add its 32 products in fp32: among the eight k of ONE lane the products are aligned to the
        // largest and what lies far below it is dropped (measured: DESIGN.md section 8t), while the four lane groups and C are added
        // to fp32 width.  So each issue gets one k per lane group -- the other seven bytes of A zero, B as loaded -- with C = 0, and
        // the eight partial sums of four exact products are added in fp32 on the lanes, in k order.
#pragma unroll 1
        for (int k0 = 0; k0 < K; k0 += 32) {
            const Frag a = *reinterpret_cast<const Frag*>(ap + k0);
            Frag a1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a1[j] = j < 4 ? make_uint2(a.x & (0xffu << (8 * j)), 0u) : make_uint2(0u, a.y & (0xffu << (8 * (j - 4))));
            Frag b[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) b[t] = *reinterpret_cast<const Frag*>(bp + (size_t)t * 16 * K + k0);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[t] += F::mfma(a1[j], b[t], v4f{0.f, 0.f, 0.f, 0.f});
                __builtin_amdgcn_sched_barrier(0);      // one tile's eight partial sums in flight, not all NT tiles'
            }
        }
    } else {
        for (int k0 = 0; k0 < K; k0 += 32) {
            const Frag a = *reinterpret_cast<const Frag*>(ap + k0);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const Frag b = *reinterpret_cast<const Frag*>(bp + (size_t)t * 16 * K + k0);
                acc[t] = F::mfma(a, b, acc[t]);
            }
        }
    }
}

// scale, bias, tanh, round and store of a layer's accumulators (D: row 4 (l >> 4) + reg, column l & 15) into the next tile
template <int NT, bool FP8>
__device__ __forceinline__ void lowp_store(const v4f* acc, const float* sv, const float* bv, typename LowpFmt<FP8>::E* out, int TS, int wave, int lane) {
    typedef LowpFmt<FP8> F;
    const int ln = lane & 15, lj = lane >> 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = (wave * NT + t) * 16 + ln;
        const float s = sv[col], b = bv[col];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            // bfloat16: the linear output is a bfloat16 tensor, as in the learner's bfloat16 operand mode (s = 1 there)
            const float pre = FP8 ? s * acc[t][rr] + b : bf16_decode(bf16_encode(acc[t][rr] + b));
            out[(4 * lj + rr) * TS + col] = F::enc(lowp_tanh_fast(pre));
        }
    }
}

// mlp_fwd_kernel's epilogue from the four distribution inputs on, text and contraction mode
__device__ __forceinline__ void lowp_sample(const LowpFwdArgs& a, int64_t m, const float* out) {
#pragma clang fp contract(fast)
    if (a.dist_inputs) *reinterpret_cast<float4*>(a.dist_inputs + (size_t)m * 4) = make_float4(out[0], out[1], out[2], out[3]);
    if (a.eps) {
        float act[2], lp = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float sd = expf(out[2 + j]);
            act[j] = out[j] + sd * a.eps[(size_t)m * 2 + j];
            const float z = (act[j] - out[j]) / sd;
            lp += -0.5f * z * z - out[2 + j] - 0.5f * kLowpLog2Pi;
        }
        a.action[(size_t)m * 2] = act[0];
        a.action[(size_t)m * 2 + 1] = act[1];
        a.logp[m] = lp;
        if (a.clipped) {
            a.clipped[(size_t)m * 2] = fminf(fmaxf(act[0], -1.0f), 1.0f);
            a.clipped[(size_t)m * 2 + 1] = fminf(fmaxf(act[1], -1.0f), 1.0f);
        }
    }
}

// NT: 16-column tiles per wave, hidden = 64 NT, four waves.  Grid ceil(cap / 16) x n_members.
template <int NT, bool FP8>
__global__ void __launch_bounds__(LOWP_THREADS) lowp_fwd_kernel(LowpFwdArgs a) {
    typedef LowpFmt<FP8> F;
    typedef typename F::E E;
    extern __shared__ uint4 lowp_lds[];
    constexpr int H = 64 * NT, HS = H + LOWP_PAD, TPR = LOWP_THREADS / LOWP_ROWS;
    const size_t k = blockIdx.y;
    const int64_t n = a.counts[k] < a.cap ? a.counts[k] : a.cap;      // (a list holds `cap` rows at the most)
    const int64_t m0 = (int64_t)blockIdx.x * LOWP_ROWS;
    if (m0 >= n) return;                                              // uniform over the workgroup, before any weight load
    const int64_t* rows = a.rows + k * (size_t)a.cap;
    // slot mm of the list: its row, or -1 where there is none (past the list, or an index outside [0, n_out))
    auto row_at = [&](int64_t mm) -> int64_t {
        if (mm >= n) return -1;
        const int64_t r = rows[mm];
        return r >= 0 && r < a.n_out ? r : -1;
    };
    const int K1 = a.in_dim, fmt = FP8 ? COPO_LOWP_E4M3 : COPO_LOWP_BF16;
    const LowpLay L(H, K1, fmt);
    const int K1P = L.K1P, XS = K1P + LOWP_PAD;
    const uint8_t* img = a.packed + k * (size_t)a.packed_stride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    E* xs = reinterpret_cast<E*>(lowp_lds);      // [16][XS]
    E* h1s = xs + LOWP_ROWS * XS;                // [16][HS]
    E* h2s = h1s + LOWP_ROWS * HS;               // [16][HS]
    // the tile's observation rows, rounded, eight columns (one A fragment) per thread and store; zero beyond in_dim and where there is no row
    const int nch = K1P >> 3;
    const bool vec = (K1 & 3) == 0 && (reinterpret_cast<uintptr_t>(a.obs_src) & 15) == 0;
    for (int i = tid; i < LOWP_ROWS * nch; i += LOWP_THREADS) {
        const int row = i / nch, kk = (i - row * nch) * 8;
        const int64_t r = row_at(m0 + row);
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (r >= 0) {
            const float* src = a.obs_src + (size_t)r * K1;
            if (vec) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    if (kk + 4 * h < K1) {
                        const float4 q = *reinterpret_cast<const float4*>(src + kk + 4 * h);
                        v[4 * h] = q.x; v[4 * h + 1] = q.y; v[4 * h + 2] = q.z; v[4 * h + 3] = q.w;
                    }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (kk + j < K1) v[j] = src[kk + j];
            }
        }
        *reinterpret_cast<typename F::Frag*>(xs + row * XS + kk) = F::pack8(v);
    }
    __syncthreads();
    v4f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
    lowp_layer<NT, FP8>(xs, XS, img + L.q1, K1P, wave, lane, acc);
    lowp_store<NT, FP8>(acc, reinterpret_cast<const float*>(img + L.s(1)), reinterpret_cast<const float*>(img + L.b(1)), h1s, HS, wave, lane);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
    lowp_layer<NT, FP8>(h1s, HS, img + L.q2, H, wave, lane, acc);
    lowp_store<NT, FP8>(acc, reinterpret_cast<const float*>(img + L.s(2)), reinterpret_cast<const float*>(img + L.b(2)), h2s, HS, wave, lane);
    __syncthreads();
    // heads on the lanes, fp32: TPR threads per row, each a strided share of the hidden units, a butterfly over them
    const int r = tid / TPR, part = tid % TPR;
    const int64_t m = row_at(m0 + r);
    const float* q3 = reinterpret_cast<const float*>(img + L.q3());
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = part; i < H; i += TPR) {
        const float h = F::dec(h2s[r * HS + i]);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] += h * q3[j * H + i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int o = 1; o < TPR; o <<= 1) out[j] += __shfl_xor(out[j], o);
    }
    if (part != 0 || m < 0) return;
    const float* s3 = reinterpret_cast<const float*>(img + L.s(3));
    const float* b3 = reinterpret_cast<const float*>(img + L.b(3));
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = FP8 ? s3[j] * out[j] + b3[j] : bf16_decode(bf16_encode(out[j] + b3[j]));
    lowp_sample(a, m, out);
}

size_t lowp_fwd_lds_bytes(int hidden, int in_dim, int fmt) {
    const LowpLay L(hidden, in_dim, fmt);
    return (size_t)LOWP_ROWS * ((L.K1P + LOWP_PAD) + 2 * (hidden + LOWP_PAD)) * L.esz;
}

template <int NT, bool FP8>
static hipError_t lowp_launch_one(int32_t n_members, const LowpFwdArgs& a, size_t lds, hipStream_t stream) {
    const dim3 grid((uint32_t)((a.cap + LOWP_ROWS - 1) / LOWP_ROWS), (uint32_t)n_members);
    hipLaunchKernelGGL((lowp_fwd_kernel<NT, FP8>), grid, dim3(LOWP_THREADS), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_lowp_forward(int hidden, int32_t fmt, int32_t n_members, const LowpFwdArgs& a, hipStream_t stream) {
    const size_t lds = lowp_fwd_lds_bytes(hidden, a.in_dim, fmt);
    const bool f8 = fmt == COPO_LOWP_E4M3;
    switch (hidden) {
        case 64: return f8 ? lowp_launch_one<1, true>(n_members, a, lds, stream) : lowp_launch_one<1, false>(n_members, a, lds, stream);
        case 128: return f8 ? lowp_launch_one<2, true>(n_members, a, lds, stream) : lowp_launch_one<2, false>(n_members, a, lds, stream);
        case 256: return f8 ? lowp_launch_one<4, true>(n_members, a, lds, stream) : lowp_launch_one<4, false>(n_members, a, lds, stream);
        case 512: return f8 ? lowp_launch_one<8, true>(n_members, a, lds, stream) : lowp_launch_one<8, false>(n_members, a, lds, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace copo
