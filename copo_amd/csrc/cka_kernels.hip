// Representation similarity of bank members (copo_cka_accumulate, copo_cka_finish; eval/similarity.py): linear CKA of
// the hidden activations that copo_hidden_obs_seats_f32 (learn_hidden.inc) keeps, over the rows a seated evaluation visits.
// ------------------------------------------------------------------------------------------------------------
// cka_gram_kernel, one launch per env step.  With h_m,l[p] the layer-l activations of panel member m at position p of the common row list
// and the COUNTED positions (p < count, the row's flags carry COPO_F_ACTED, rows_of < 0 or the row's seat is rows_of), for every member
// pair a <= b and both layers:
//     S[a,b,l][i][j] += sum_p h_a,l[p][i] h_b,l[p][j]      s[a,l][i] += sum_p h_a,l[p][i]      n += the counted positions
// -- the shape of the weight-gradient GEMM (X^T Y, rows as the reduction dimension; learn_gemm.inc's gemm_bw_kernel), over pairs of
// members and into float64.  Grid: (H / 64)^2 tiles x (pairs * 2 layers) x R planes, 256 threads.  A workgroup owns one 64 x 64 tile of
// one S[a,b,l] in one plane; wave w owns its rows 16 w .. 16 w + 15 as four 16 x 16 accumulators of v_mfma_f32_16x16x4_f32 (fp32 operands:
// lane l supplies A[i = l & 15][k = l >> 4] = h_a[p0 + k][i0 + i] and B[k][j = l & 15] = h_b[p0 + k][j0 + j], so the reduction index of
// the instruction is the position).  The positions are walked in chunks of 32: plane r takes chunks r, r + R, r + 2 R, ... in ascending
// order, stages both operands of a chunk in LDS (128-bit loads, the next chunk's in flight while this one multiplies; rows of 80 floats,
// so the four position groups of a wave's read fall on disjoint banks), and after every fourth chunk of its own and at the end adds the fp32
// partial to its float64 plane with a plain load-add-store and clears it.  Every accumulator element has one owner and one order: no
// atomics, and two runs of the same sequence of launches leave the same bits.  R is the caller's (a property of the plan).
// A position that is not counted contributes exact zeros: the OPERAND is replaced by zero when it is staged, whatever the workspace
// holds there (not-a-numbers included).
// s rides along: the workgroups of the pairs (a, a) in tile column 0 run a fifth accumulator against a B operand of ones, whose every
// column is the row sum.  n: workgroup (0, 0) of every plane counts its chunks' positions with a ballot.
// cka_finish_kernel: one workgroup per (pair, layer), float64 throughout: the planes summed in plane order, then
//     hsic[a,b,l] = || S - s_a s_b^T / n ||_F^2
// with a fixed-order tree over lanes (xor butterfly) and waves (in order); the means and variances of the units come from the diagonal
// pairs.  n < 2: zeros.
#include "cka_common.h"

namespace copo {

typedef float cka_v4f __attribute__((ext_vector_type(4)));
constexpr int CKA_STRIDE = 80;      // floats per staged position: 64 units + 16, so that positions p .. p + 3 start on banks 0 / 16 / 32 / 48

// (by value: a reference to the kernel's argument struct would put the struct on the stack)
struct CkaMask {
    const int64_t* rows;
    const uint8_t* flags;
    const int32_t* seat;
    int64_t count, n_out;
    int32_t rows_of;
};
__device__ __forceinline__ bool cka_counted(const CkaMask m, int64_t p) {
    if (p >= m.count) return false;
    const int64_t r = m.rows[p];
    if (r < 0 || r >= m.n_out) return false;
    return (m.flags[r] & COPO_F_ACTED) != 0 && (m.rows_of < 0 || m.seat[r] == m.rows_of);
}

// pair index -> (a, b), a <= b, rows of the upper triangle one after the other
__device__ __forceinline__ void cka_pair(int pair, int M, int& pa, int& pb) {
    int a = 0;
    while (pair >= M - a) {
        pair -= M - a;
        ++a;
    }
    pa = a;
    pb = a + pair;
}

__global__ __launch_bounds__(256) void cka_gram_kernel(CkaArgs a) {
    __shared__ float4 lds_a4[CKA_CHUNK * CKA_STRIDE / 4], lds_b4[CKA_CHUNK * CKA_STRIDE / 4];
    float* as = reinterpret_cast<float*>(lds_a4);
    float* bs = reinterpret_cast<float*>(lds_b4);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 15, lj = lane >> 4;
    const int H = a.H, nt = H / CKA_TILE, ti = blockIdx.x / nt, tj = blockIdx.x - ti * nt;
    const int pair = blockIdx.y >> 1, layer = blockIdx.y & 1, plane = blockIdx.z, P = a.M * (a.M + 1) / 2;
    int pa, pb;
    cka_pair(pair, a.M, pa, pb);
    const int64_t listed = *a.count, count = listed < 0 ? 0 : listed < a.cap ? listed : a.cap;
    const int64_t n_chunks = (count + CKA_CHUNK - 1) / CKA_CHUNK;
    if (plane >= n_chunks) return;      // (uniform over the workgroup: this plane has no chunk in this launch)
    const CkaMask mask{a.rows, a.flags, a.seat, count, a.n_out, a.rows_of};
    const int R = a.R, M = a.M;
    const int ma = a.panel[pa], mb = a.panel[pb];
    if (ma < 0 || ma >= a.K || mb < 0 || mb >= a.K) return;      // (uniform: a panel entry that names no member)
    const size_t pos_stride = (size_t)2 * H;
    const float* base_a = a.hidden + ((size_t)ma * a.cap * 2 + layer) * H + CKA_TILE * ti;
    const float* base_b = a.hidden + ((size_t)mb * a.cap * 2 + layer) * H + CKA_TILE * tj;
    const bool own_s = pa == pb && tj == 0, own_n = blockIdx.x == 0 && blockIdx.y == 0;
    const int sp = tid >> 4, sc = (tid & 15) * 4;      // this thread stages positions sp and sp + 16 of a chunk, units sc .. sc + 3
    float4 reg[4];
    auto fetch = [&](int64_t chunk) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t p = chunk * CKA_CHUNK + sp + 16 * h;
            const bool ok = cka_counted(mask, p);
            const size_t at = (size_t)(ok ? p : 0) * pos_stride + sc;
            const float4 va = *reinterpret_cast<const float4*>(base_a + at), vb = *reinterpret_cast<const float4*>(base_b + at);
            // the operand is masked, not the product (component by component: a select of two float4 objects goes through memory)
            reg[h] = make_float4(ok ? va.x : 0.f, ok ? va.y : 0.f, ok ? va.z : 0.f, ok ? va.w : 0.f);
            reg[2 + h] = make_float4(ok ? vb.x : 0.f, ok ? vb.y : 0.f, ok ? vb.z : 0.f, ok ? vb.w : 0.f);
        }
    };
    cka_v4f acc[4], accs = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = cka_v4f{0.f, 0.f, 0.f, 0.f};
    double* S = a.S + (((size_t)plane * P + pair) * 2 + layer) * H * H + (size_t)(CKA_TILE * ti + 16 * wave + 4 * lj) * H + CKA_TILE * tj + ln;
    double* s = a.s + (((size_t)plane * M + pa) * 2 + layer) * H + CKA_TILE * ti + 16 * wave + 4 * lj;
    auto promote = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                double* at = S + (size_t)rr * H + 16 * t;
                *at = *at + (double)acc[t][rr];
            }
            acc[t] = cka_v4f{0.f, 0.f, 0.f, 0.f};
        }
        if (own_s) {
            if (ln == 0) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) s[rr] = s[rr] + (double)accs[rr];
            }
            accs = cka_v4f{0.f, 0.f, 0.f, 0.f};
        }
    };
    int64_t n_local = 0;
    int since = 0;
    fetch(plane);
    for (int64_t c = plane; c < n_chunks; c += R) {
        __syncthreads();      // (the previous chunk's reads are done)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<float4*>(as + (sp + 16 * h) * CKA_STRIDE + sc) = reg[h];
            *reinterpret_cast<float4*>(bs + (sp + 16 * h) * CKA_STRIDE + sc) = reg[2 + h];
        }
        if (own_n && wave == 0) n_local += __popcll(__ballot(lane < CKA_CHUNK && cka_counted(mask, c * CKA_CHUNK + lane)));
        __syncthreads();
        if (c + R < n_chunks) fetch(c + R);
#pragma unroll
        for (int ks = 0; ks < CKA_CHUNK / 4; ++ks) {
            const float av = as[(4 * ks + lj) * CKA_STRIDE + 16 * wave + ln];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bs[(4 * ks + lj) * CKA_STRIDE + 16 * t + ln], acc[t], 0, 0, 0);
            if (own_s) accs = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.0f, accs, 0, 0, 0);
        }
        if (++since == CKA_PROMOTE_CHUNKS) {
            promote();
            since = 0;
        }
    }
    if (since) promote();
    if (own_n && tid == 0) a.n[plane] = a.n[plane] + n_local;
}

__global__ __launch_bounds__(256) void cka_finish_kernel(const double* __restrict__ S, const double* __restrict__ s, const int64_t* __restrict__ n_planes,
                                                         int M, int H, int R, double* __restrict__ hsic, int64_t* __restrict__ n_out,
                                                         double* __restrict__ mean, double* __restrict__ var) {
    __shared__ double sa[COPO_CKA_MAX_HIDDEN], sb[COPO_CKA_MAX_HIDDEN], wave_part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x, layer = blockIdx.y, P = M * (M + 1) / 2;
    int pa, pb;
    cka_pair(pair, M, pa, pb);
    int64_t n = 0;
    for (int r = 0; r < R; ++r) n += n_planes[r];
    const bool enough = n >= 2;
    const double dn = (double)n;
    for (int i = tid; i < H; i += 256) {
        double va = 0.0, vb = 0.0;
        for (int r = 0; r < R; ++r) {
            va = va + s[(((size_t)r * M + pa) * 2 + layer) * H + i];
            vb = vb + s[(((size_t)r * M + pb) * 2 + layer) * H + i];
        }
        sa[i] = va;
        sb[i] = vb;
    }
    __syncthreads();
    const size_t plane_stride = (size_t)P * 2 * H * H;
    const double* Sp = S + ((size_t)pair * 2 + layer) * H * H;
    double part = 0.0;
    if (enough) {
        for (int e = tid; e < H * H; e += 256) {
            const int i = e / H, j = e - i * H;
            double v = 0.0;
            for (int r = 0; r < R; ++r) v = v + Sp[(size_t)r * plane_stride + e];
            const double d = v - sa[i] * sb[j] / dn;
            part = part + d * d;
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) part = part + __shfl_xor(part, o);
    if (lane == 0) wave_part[wave] = part;
    __syncthreads();
    if (tid == 0) {
        const double total = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
        hsic[((size_t)pa * M + pb) * 2 + layer] = total;
        hsic[((size_t)pb * M + pa) * 2 + layer] = total;
        if (pair == 0 && layer == 0) *n_out = n;
    }
    if (pa == pb) {
        for (int i = tid; i < H; i += 256) {
            double d = 0.0;
            for (int r = 0; r < R; ++r) d = d + Sp[(size_t)r * plane_stride + (size_t)i * H + i];
            const double m = enough ? sa[i] / dn : 0.0;
            mean[((size_t)pa * 2 + layer) * H + i] = m;
            var[((size_t)pa * 2 + layer) * H + i] = enough ? d / dn - m * m : 0.0;
        }
    }
}

hipError_t launch_cka_accumulate(const CkaArgs& a, hipStream_t stream) {
    const int nt = a.H / CKA_TILE, P = a.M * (a.M + 1) / 2;
    hipLaunchKernelGGL(cka_gram_kernel, dim3(nt * nt, 2 * P, a.R), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cka_finish(const double* S, const double* s, const int64_t* n, int32_t M, int32_t H, int32_t R, double* hsic, int64_t* n_out,
                             double* mean, double* var, hipStream_t stream) {
    hipLaunchKernelGGL(cka_finish_kernel, dim3(M * (M + 1) / 2, 2), dim3(256), 0, stream, S, s, n, M, H, R, hsic, n_out, mean, var);
    return hipGetLastError();
}

}  // namespace copo
