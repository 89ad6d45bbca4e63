// The Gram tile under representation similarity (cka_kernels.hip) and linear probes (probe_kernels.hip, section 8x):
// one 64 x 64 tile of X_a^T X_b over the counted positions of a row list, fp32 on the matrix cores into a float64 plane.  Everything here
// is inlined into the kernel that uses it; no device call crosses a unit.
// ------------------------------------------------------------------------------------------------------------
// gram_tile, one workgroup of 256 threads.  With x_a[p], x_b[p] the 64 features at `base_a` / `base_b` + p * pos_stride and the COUNTED
// positions (gram_counted: p < count, the row's flags carry COPO_F_ACTED, rows_of < 0 or the row's seat is rows_of, and with a fold term
// fold[scene of the row] == f):
//     dst[i][j] += sum_p x_a[p][i] x_b[p][j]
// -- the shape of the weight-gradient GEMM (X^T Y, rows as the reduction dimension; learn_gemm.inc's gemm_bw_kernel), into float64.
// Wave w owns rows 16 w .. 16 w + 15 of the tile as four 16 x 16 accumulators of v_mfma_f32_16x16x4_f32 (fp32 operands: lane l supplies
// A[i = l & 15][k = l >> 4] = x_a[p0 + k][i] and B[k][j = l & 15] = x_b[p0 + k][j], so the reduction index of the instruction is the
// position).  The positions are walked in chunks of 32: plane r of R takes chunks r, r + R, r + 2 R, ... in ascending order, stages both
// operands of a chunk in LDS (128-bit loads, the next chunk's in flight while this one multiplies; rows of 80 floats, so the four position
// groups of a wave's read fall on disjoint banks), and after every fourth chunk of its own and at the end adds the fp32 partial to its
// float64 plane with a plain load-add-store and clears it.  Every accumulator element has one owner and one order: no atomics, and two runs
// of the same sequence of launches leave the same bits.  R is the caller's (a property of the plan).
// A position that is not counted contributes exact zeros: the OPERAND is replaced by zero when it is staged, whatever the workspace
// holds there (not-a-numbers included).
// With RIDERS (GramRiders) two more sums ride along on the same walk: where own_s, a fifth accumulator against a B operand of ones, whose
// every column is the row sum of x_a, added to s[0 .. 64) at the promote point; where own_n, the chunks' counted positions by ballot at the
// staging point, added to *n at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/copo_hip.h"

namespace copo {

typedef float gram_v4f __attribute__((ext_vector_type(4)));
constexpr int GRAM_TILE = 64;                                 // a workgroup owns a 64 x 64 tile
constexpr int GRAM_CHUNK = COPO_CKA_CHUNK;                    // positions staged through LDS at a time
constexpr int GRAM_PROMOTE_CHUNKS = COPO_CKA_PROMOTE_ROWS / COPO_CKA_CHUNK;      // fp32 partial -> float64 accumulator after so many chunks
constexpr int GRAM_STRIDE = 80;      // floats per staged position: 64 units + 16, so that positions p .. p + 3 start on banks 0 / 16 / 32 / 48

// *count clamped to [0, cap], and the chunks that many positions make
__device__ __forceinline__ int64_t gram_count(const int32_t* count, int64_t cap) {
    const int64_t listed = *count;
    return listed < 0 ? 0 : listed < cap ? listed : cap;
}
__device__ __forceinline__ int64_t gram_chunks(int64_t count) { return (count + GRAM_CHUNK - 1) / GRAM_CHUNK; }

// index into the upper triangle of an n x n table -> (a, b), a <= b, rows of the triangle one after the other: (0, 0) .. (0, n - 1), (1, 1) ..
__device__ __forceinline__ void gram_upper(int index, int n, int& ra, int& rb) {
    int a = 0;
    while (index >= n - a) {
        index -= n - a;
        ++a;
    }
    ra = a;
    rb = a + index;
}

// (by value: a reference to the kernel's argument struct would put the struct on the stack)
// FOLD: the fold term counts; without it fold, slots and f are never read.
template <bool FOLD>
struct GramMask {
    const int64_t* rows;
    const uint8_t* flags;
    const int32_t* seat;
    const uint8_t* fold;
    int64_t count, n_out;
    int32_t slots, rows_of, f;
};
template <bool FOLD>
__device__ __forceinline__ bool gram_counted(const GramMask<FOLD> m, int64_t p) {
    if (p >= m.count) return false;
    const int64_t r = m.rows[p];
    if (r < 0 || r >= m.n_out) return false;
    const bool ok = (m.flags[r] & COPO_F_ACTED) != 0 && (m.rows_of < 0 || m.seat[r] == m.rows_of);
    if constexpr (FOLD) return ok && m.fold[r / m.slots] == m.f;
    return ok;
}

struct GramRiders {
    double* s;        // [64]: the row sums of x_a, where own_s
    int64_t* n;       // [1]: the counted positions, where own_n
    bool own_s, own_n;
};

// `dst`: element (0, 0) of the tile in this plane, rows `ld` doubles apart.  Every thread of the workgroup calls it (it has barriers).
template <bool RIDERS, bool FOLD>
__device__ __forceinline__ void gram_tile(const float* base_a, const float* base_b, size_t pos_stride, const GramMask<FOLD> mask, int plane, int R,
                                          double* dst, size_t ld, const GramRiders rd = {}) {
    __shared__ float4 lds_a4[GRAM_CHUNK * GRAM_STRIDE / 4], lds_b4[GRAM_CHUNK * GRAM_STRIDE / 4];
    float* as = reinterpret_cast<float*>(lds_a4);
    float* bs = reinterpret_cast<float*>(lds_b4);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 15, lj = lane >> 4;
    const int64_t n_chunks = gram_chunks(mask.count);
    const int sp = tid >> 4, sc = (tid & 15) * 4;      // this thread stages positions sp and sp + 16 of a chunk, units sc .. sc + 3
    float4 reg[4];
    auto fetch = [&](int64_t chunk) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t p = chunk * GRAM_CHUNK + sp + 16 * h;
            const bool ok = gram_counted(mask, p);
            const size_t at = (size_t)(ok ? p : 0) * pos_stride + sc;
            const float4 va = *reinterpret_cast<const float4*>(base_a + at), vb = *reinterpret_cast<const float4*>(base_b + at);
            // the operand is masked, not the product (component by component: a select of two float4 objects goes through memory)
            reg[h] = make_float4(ok ? va.x : 0.f, ok ? va.y : 0.f, ok ? va.z : 0.f, ok ? va.w : 0.f);
            reg[2 + h] = make_float4(ok ? vb.x : 0.f, ok ? vb.y : 0.f, ok ? vb.z : 0.f, ok ? vb.w : 0.f);
        }
    };
    gram_v4f acc[4], accs = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = gram_v4f{0.f, 0.f, 0.f, 0.f};
    dst += (size_t)(16 * wave + 4 * lj) * ld + ln;
    double* s = RIDERS ? rd.s + 16 * wave + 4 * lj : nullptr;
    auto promote = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                double* at = dst + (size_t)rr * ld + 16 * t;
                *at = *at + (double)acc[t][rr];
            }
            acc[t] = gram_v4f{0.f, 0.f, 0.f, 0.f};
        }
        if (RIDERS && rd.own_s) {
            if (ln == 0) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) s[rr] = s[rr] + (double)accs[rr];
            }
            accs = gram_v4f{0.f, 0.f, 0.f, 0.f};
        }
    };
    int64_t n_local = 0;
    int since = 0;
    fetch(plane);
    for (int64_t c = plane; c < n_chunks; c += R) {
        __syncthreads();      // (the previous chunk's reads are done)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<float4*>(as + (sp + 16 * h) * GRAM_STRIDE + sc) = reg[h];
            *reinterpret_cast<float4*>(bs + (sp + 16 * h) * GRAM_STRIDE + sc) = reg[2 + h];
        }
        if (RIDERS && rd.own_n && wave == 0) n_local += __popcll(__ballot(lane < GRAM_CHUNK && gram_counted(mask, c * GRAM_CHUNK + lane)));
        __syncthreads();
        if (c + R < n_chunks) fetch(c + R);
#pragma unroll
        for (int ks = 0; ks < GRAM_CHUNK / 4; ++ks) {
            const float av = as[(4 * ks + lj) * GRAM_STRIDE + 16 * wave + ln];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bs[(4 * ks + lj) * GRAM_STRIDE + 16 * t + ln], acc[t], 0, 0, 0);
            if (RIDERS && rd.own_s) accs = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.0f, accs, 0, 0, 0);
        }
        if (++since == GRAM_PROMOTE_CHUNKS) {
            promote();
            since = 0;
        }
    }
    if (since) promote();
    if (RIDERS && rd.own_n && tid == 0) *rd.n = *rd.n + n_local;
}

}  // namespace copo
