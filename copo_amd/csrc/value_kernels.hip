// Value pass of a seated bank (copo_value_obs_seats_f32; eval/critics.py): value_obs_kernel, the value nets of
// every member on the rows of its seat list in one launch.  A unit of its own, as lowp_kernels.hip is: the learner's kernel table
// (learn_plan.inc) does not grow and none of the learner's kernels is compiled differently.  What it shares with learn_fused.hip it
// includes as it stands -- HT and opnd (learn_args.inc), tanh_fast (learn_gemm.inc), v4f, BRing and rowpass_k1p (learn_rowpass.inc),
// SeatHead / seat_row_at (learn_seat.inc) -- inside an unnamed namespace, so that the kernels and device variables those files define
// stay local to this unit, and under that unit's contraction mode, so that equal inputs give equal bits.
//
// Member k = blockIdx.y owns the list rows[k cap .. k cap + counts[k]) of [0, n_out); head h = blockIdx.z is value net val[h] of the
// member ("net = blockIdx.y" of the single-member kernel, moved to z).  Per listed row r:
//     h1 = tanh(W1 x + b1), h2 = tanh(W2 h1 + b2), values[r][h] = w3 . h2 + b3,   x = src[r] (val[h].in_dim wide)
// -- the bits copo_mlp_forward_rows_f32(first_net = 1, n_nets = heads) writes for member k alone on its gathered rows at the one-tile
// variant: the staging masks as mlp_fwd_kernel's (zero rows where the tile has none, zero columns beyond in_dim; 128-bit loads where the
// width and the address allow them, scalar loads otherwise), layers 1 and 2 are the one-tile forward body (a copy of mlp_fwd_kernel's on
// purpose, as jury_obs_kernel's is), the head repeats its summation order (TH / 16 threads per row, stride TH / 16, xor tree, bias
// last).  A tile row's sums read that row's LDS rows only, so the bits do not depend on which other rows share the tile.
// Always the 16-row tile; a workgroup past counts[k] leaves before any weight load; the last tile is masked; a row index outside
// [0, n_out) and rows in no list are not written.  No atomics, fixed summation order: two launches give the same bits.
// MAINTENANCE: this is the fourth copy of mlp_fwd_kernel's one-tile body (after adv_obs_kernel, jury_obs_kernel and hidden_obs_kernel).  Any
// change to that body, its staging masks or its head order in learn_rowpass.inc must be mirrored here, or the bit contract above (held by
// tests/test_gpu_critics.py) breaks.  Including the four files whole also gives this unit private copies of their profiling variables and
// of learn_gemm.inc's non-template kernel, none of which it launches; hence the unused-function suppression below.
#include <cstring>
#include <type_traits>

#include "sim_common.h"
#include "value_common.h"

#pragma clang fp contract(fast)
#pragma clang diagnostic ignored "-Wunused-function"      // (the included files define more than this unit launches)

namespace copo {
namespace {
#include "learn_args.inc"
#include "learn_gemm.inc"
#include "learn_rowpass.inc"
#include "learn_seat.inc"

constexpr int VALUE_LDS_CAP = 150 * 1024;      // the forward workgroups' ceiling in learn_fused.hip (gfx950: 160 KB per CU)

__device__ __host__ inline size_t value_lds_floats(int H, int k1p) { return (size_t)2 * HT * (H + 4) + (size_t)HT * (k1p + 4) + H; }

template <int NT, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) value_obs_kernel(ValueSeatArgs a) {
    extern __shared__ float4 value_lds[];
    constexpr int H = 16 * NT * WAVES, HP = H + 4, TH = 64 * WAVES, TPR = TH / HT;
    constexpr int DB = NT >= 8 ? 4 : (H / 16 >= 8 ? 8 : H / 16);
    const copo_ppo_cfg& c = a.c;
    const size_t k = blockIdx.y;
    const int hd = blockIdx.z;
    const int64_t n = a.counts[k] < a.cap ? a.counts[k] : a.cap;      // (a list holds `cap` rows at the most)
    const int64_t m0 = (int64_t)blockIdx.x * HT;
    if (m0 >= n) return;       // (uniform over the workgroup; nothing of the weights has been requested)
    const float* theta = a.theta + k * a.member_stride;
    const float* theta_t = a.theta_t + k * a.member_stride;
    const int64_t* rows = a.rows + k * (size_t)a.cap;
    const copo_net_layout L = c.val[hd];
    const float* src = a.src;
    // slot mm of the list: its row, or -1 where there is none (learn_seat.inc: past the list, or an index outside [0, n_out))
    SeatHead sh{};
    sh.n_out = a.n_out;
    const int K1 = L.in_dim, K1P = rowpass_k1p(K1), XP = K1P + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 15, lj = lane >> 4, cb = wave * (16 * NT);
    float* h1s = reinterpret_cast<float*>(value_lds);   // [HT][HP]
    float* h2s = h1s + HT * HP;                         // [HT][HP]
    float* xs = h2s + HT * HP;                          // [HT][XP]  the input rows, zero beyond K1
    float* w3s = xs + HT * XP;                          // [H]
    BRing<NT, DB, false> ring;
    ring.start(theta_t + L.w1, H, cb, ln, lj);
    if ((K1 & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int qn = K1P >> 2;
        for (int i = tid; i < HT * qn; i += TH) {
            const int row = i / qn, kk = (i - row * qn) * 4;
            const int64_t r = seat_row_at(sh, rows, n, m0 + row);
            const bool ok = r >= 0 && kk < K1;
            const float4 v = *reinterpret_cast<const float4*>(src + (size_t)(r < 0 ? 0 : r) * K1 + (kk < K1 ? kk : 0));
            *reinterpret_cast<float4*>(xs + row * XP + kk) = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        for (int i = tid; i < HT * K1P; i += TH) {
            const int row = i / K1P, kk = i - row * K1P;
            const int64_t r = seat_row_at(sh, rows, n, m0 + row);
            const bool ok = r >= 0 && kk < K1;
            const float v = src[(size_t)(r < 0 ? 0 : r) * K1 + (kk < K1 ? kk : 0)];
            xs[row * XP + kk] = ok ? v : 0.0f;
        }
    }
    for (int i = tid; i < H; i += TH) w3s[i] = theta[L.w3 + i];
    __syncthreads();
    v4f acc[1][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[0][t] = v4f{0.f, 0.f, 0.f, 0.f};
    ring.template run_tiles<1>(xs, XP, (K1 + 15) & ~15, ln, lj, acc);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = cb + NT * ln + t;
        const float bv = theta[L.b1 + col];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) h1s[(4 * lj + rr) * HP + col] = tanh_fast(acc[0][t][rr] + bv);
    }
    ring.start(theta_t + L.w2, H, cb, ln, lj);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[0][t] = v4f{0.f, 0.f, 0.f, 0.f};
    ring.template run_tiles<1>(h1s, HP, H, ln, lj, acc);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = cb + NT * ln + t;
        const float bv = theta[L.b2 + col];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) h2s[(4 * lj + rr) * HP + col] = tanh_fast(acc[0][t][rr] + bv);
    }
    __syncthreads();
    // ---- the head, in mlp_fwd_kernel's order: TPR threads per row, each a strided share of H, an xor tree, then the bias ----
    const int r = tid / TPR, part = tid % TPR;
    float out = 0.f;
    for (int i = part; i < H; i += TPR) out += h2s[r * HP + i] * w3s[i];
#pragma unroll
    for (int o = 1; o < TPR; o <<= 1) out += __shfl_xor(out, o);
    if (part != 0) return;
    const int64_t dst = seat_row_at(sh, rows, n, m0 + r);
    if (dst < 0) return;
    a.values[(size_t)dst * c.n_value_heads + hd] = out + theta[L.b3];
}

template <int NT, int WAVES>
hipError_t value_launch_one(const ValueSeatArgs& a, size_t lds, hipStream_t stream) {
    // the ceiling above the default 64 KB as an attribute, once per process and instantiation
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&value_obs_kernel<NT, WAVES>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, VALUE_LDS_CAP);
    if (attr != hipSuccess) return attr;
    const dim3 grid((uint32_t)((a.cap + HT - 1) / HT), (uint32_t)a.n_members, (uint32_t)a.c.n_value_heads);
    hipLaunchKernelGGL((value_obs_kernel<NT, WAVES>), grid, dim3(64 * WAVES), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

size_t value_seats_lds_bytes(const copo_ppo_cfg& c) {
    const int H = c.hidden;
    if (H != 64 && H != 128 && H != 256 && H != 512) return 0;
    int kmax = 1;
    for (int h = 0; h < c.n_value_heads && h < 3; ++h) kmax = c.val[h].in_dim > kmax ? c.val[h].in_dim : kmax;
    return value_lds_floats(H, rowpass_k1p(kmax)) * sizeof(float);
}

hipError_t launch_value_seats(const ValueSeatArgs& a, hipStream_t stream) {
    const size_t lds = value_seats_lds_bytes(a.c);
    if (lds == 0 || lds > (size_t)VALUE_LDS_CAP) return hipErrorInvalidValue;
    switch (a.c.hidden) {      // hidden = 16 NT WAVES, the four shapes of the learner's forward
        case 64: return value_launch_one<1, 4>(a, lds, stream);
        case 128: return value_launch_one<2, 4>(a, lds, stream);
        case 256: return value_launch_one<2, 8>(a, lds, stream);
        case 512: return value_launch_one<4, 8>(a, lds, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace copo
