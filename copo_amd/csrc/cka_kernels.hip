// Representation similarity of bank members (copo_cka_accumulate, copo_cka_finish; eval/similarity.py): linear CKA of
// the hidden activations that copo_hidden_obs_seats_f32 (learn_hidden.inc) keeps, over the rows a seated evaluation visits.
// ------------------------------------------------------------------------------------------------------------
// cka_gram_kernel, one launch per env step.  With h_m,l[p] the layer-l activations of panel member m at position p of the common row list
// and the COUNTED positions (gram_common.h, no fold term), for every member pair a <= b and both layers:
//     S[a,b,l][i][j] += sum_p h_a,l[p][i] h_b,l[p][j]      s[a,l][i] += sum_p h_a,l[p][i]      n += the counted positions
// Grid: (H / 64)^2 tiles x (pairs * 2 layers) x R planes, 256 threads.  A workgroup owns one 64 x 64 tile of one S[a,b,l] in one plane
// and is gram_tile (gram_common.h: the chunk walk, the staging, the matrix-core loop and the promotion to float64 are described there)
// with its operands taken from two members' activations.  Both riders of the tile are used: s by the workgroups of the pairs (a, a) in
// tile column 0, n by workgroup (0, 0) of every plane.
// cka_finish_kernel: one workgroup per (pair, layer), float64 throughout: the planes summed in plane order, then
//     hsic[a,b,l] = || S - s_a s_b^T / n ||_F^2
// with a fixed-order tree over lanes (xor butterfly) and waves (in order); the means and variances of the units come from the diagonal
// pairs.  n < 2: zeros.
#include "cka_common.h"
#include "gram_common.h"

namespace copo {

__global__ __launch_bounds__(256) void cka_gram_kernel(CkaArgs a) {
    const int H = a.H, nt = H / GRAM_TILE, ti = blockIdx.x / nt, tj = blockIdx.x - ti * nt;
    const int pair = blockIdx.y >> 1, layer = blockIdx.y & 1, plane = blockIdx.z, P = a.M * (a.M + 1) / 2;
    int pa, pb;
    gram_upper(pair, a.M, pa, pb);
    const int64_t count = gram_count(a.count, a.cap);
    if (plane >= gram_chunks(count)) return;      // (uniform over the workgroup: this plane has no chunk in this launch)
    const GramMask<false> mask{a.rows, a.flags, a.seat, nullptr, count, a.n_out, 0, a.rows_of, 0};
    const int M = a.M;
    const int ma = a.panel[pa], mb = a.panel[pb];
    if (ma < 0 || ma >= a.K || mb < 0 || mb >= a.K) return;      // (uniform: a panel entry that names no member)
    const float* base_a = a.hidden + ((size_t)ma * a.cap * 2 + layer) * H + GRAM_TILE * ti;
    const float* base_b = a.hidden + ((size_t)mb * a.cap * 2 + layer) * H + GRAM_TILE * tj;
    double* S = a.S + (((size_t)plane * P + pair) * 2 + layer) * H * H + (size_t)(GRAM_TILE * ti) * H + GRAM_TILE * tj;
    double* s = a.s + (((size_t)plane * M + pa) * 2 + layer) * H + GRAM_TILE * ti;
    const GramRiders riders{s, a.n + plane, pa == pb && tj == 0, blockIdx.x == 0 && blockIdx.y == 0};
    gram_tile<true>(base_a, base_b, (size_t)2 * H, mask, plane, a.R, S, (size_t)H, riders);
}

__global__ __launch_bounds__(256) void cka_finish_kernel(const double* __restrict__ S, const double* __restrict__ s, const int64_t* __restrict__ n_planes,
                                                         int M, int H, int R, double* __restrict__ hsic, int64_t* __restrict__ n_out,
                                                         double* __restrict__ mean, double* __restrict__ var) {
    __shared__ double sa[COPO_CKA_MAX_HIDDEN], sb[COPO_CKA_MAX_HIDDEN], wave_part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x, layer = blockIdx.y, P = M * (M + 1) / 2;
    int pa, pb;
    gram_upper(pair, M, pa, pb);
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
    const int nt = a.H / GRAM_TILE, P = a.M * (a.M + 1) / 2;
    hipLaunchKernelGGL(cka_gram_kernel, dim3(nt * nt, 2 * P, a.R), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cka_finish(const double* S, const double* s, const int64_t* n, int32_t M, int32_t H, int32_t R, double* hsic, int64_t* n_out,
                             double* mean, double* var, hipStream_t stream) {
    hipLaunchKernelGGL(cka_finish_kernel, dim3(M * (M + 1) / 2, 2), dim3(256), 0, stream, S, s, n, M, H, R, hsic, n_out, mean, var);
    return hipGetLastError();
}

}  // namespace copo
