// Part of learn_fused.hip: the jury pass of a seated bank -- every JUDGE's distribution parameters on rows that another member may drive
// (copo_jury_obs_seats_f32; eval/jury.py, DESIGN.md section 8r).  The third mode of the bank's forward: the dense bank gives a member its
// own rows, seat mode gives a row to one member (its outputs land at row r of shared [n_out] arrays), here a row may stand in the lists
// of many members and every member's outputs land in a plane of their own.
// ------------------------------------------------------------------------------------------------------------
// Judge j = blockIdx.y owns the list rows[j cap .. j cap + counts[j]) of [0, n_out); a row may appear in several judges' lists, once per
// list.  Per listed row r, with o the TRUE row obs_src[r] and member j's parameters:
//     h1 = tanh(W1 o + b1), h2 = tanh(W2 h1 + b2), verdict[r][j][0..4) = W3 h2 + b3 = mu_steer, mu_throttle, logstd_steer, logstd_throttle
// -- the bits copo_mlp_forward_seats_f32 writes to dist_inputs[r] when member j's list holds r: the prologue is learn_seat.inc's (same
// masking: zero rows where the tile has none), layers 1 and 2 are the one-tile forward body (a copy of mlp_fwd_kernel's on purpose, as
// adv_obs_kernel's is: see there), and the heads repeat mlp_fwd_kernel's summation order (TH / 16 threads per row, stride TH / 16, xor
// tree, bias last).  A tile row's sums read that row's LDS rows only, so the bits do not depend on which other rows share the tile.
// Launch shape of seat mode: grid ceil(cap / 16) x n_members, always the 16-row tile; a workgroup past counts[j] leaves at once, before
// any weight load; the last tile is masked; entries no list names are not written.  No sampling, no eps, no atomics, fixed summation
// order: two launches give the same bits.  SeatHead's group / level fields are unused here (zero).
// LDS: h1 and h2 tiles [16][H + 4], the input tile [16][k1p + 4], all four rows of W3 (seat_stage brings the two mean rows, the two
// log-std rows follow them).
// ------------------------------------------------------------------------------------------------------------
struct JuryArgs {
    SeatHead h;
    float* verdict;           // [n_out][n_members][4]
};

__device__ __host__ inline size_t jury_lds_floats(int H, int k1p) { return (size_t)2 * HT * (H + 4) + (size_t)HT * (k1p + 4) + 4 * H; }

template <int NT, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) jury_obs_kernel(JuryArgs a) {
    extern __shared__ float4 jury_lds[];
    constexpr int H = 16 * NT * WAVES, HP = H + 4, TH = 64 * WAVES, TPR = TH / HT;
    constexpr int DB = NT >= 8 ? 4 : (H / 16 >= 8 ? 8 : H / 16);
    const SeatHead& hd = a.h;
    const copo_ppo_cfg& c = hd.c;
    const size_t k = blockIdx.y;
    const int64_t n = hd.counts[k] < hd.cap ? hd.counts[k] : hd.cap;      // (a list holds `cap` rows at the most)
    const int64_t m0 = (int64_t)blockIdx.x * HT;
    if (m0 >= n) return;       // (uniform over the workgroup; nothing of the weights has been requested)
    const float* theta = hd.theta + k * hd.member_stride;
    const float* theta_t = hd.theta_t + k * hd.member_stride;
    const int64_t* rows = hd.rows + k * (size_t)hd.cap;
    const copo_net_layout L = c.pol;
    const int K1 = L.in_dim, K1P = rowpass_k1p(K1), XP = K1P + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 15, lj = lane >> 4, cb = wave * (16 * NT);
    float* h1s = reinterpret_cast<float*>(jury_lds);    // [HT][HP]
    float* h2s = h1s + HT * HP;                         // [HT][HP]
    float* xs = h2s + HT * HP;                          // [HT][XP]  the true observation rows, zero beyond K1
    float* w3s = xs + HT * XP;                          // [4][H]
    BRing<NT, DB, false> ring;
    ring.start(theta_t + L.w1, H, cb, ln, lj);
    seat_stage<TH>(hd, rows, n, m0, theta, H, xs, w3s, tid);
    for (int i = tid; i < 2 * H; i += TH) w3s[2 * H + i] = theta[L.w3 + 2 * H + i];      // the two log-std rows behind the mean rows
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
    // ---- heads, in mlp_fwd_kernel's order: TPR threads per row, each a strided share of H, an xor tree, then the bias ----
    const int r = tid / TPR, part = tid % TPR;
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = part; i < H; i += TPR) {
        const float h = h2s[r * HP + i];
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] += h * w3s[j * H + i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int o = 1; o < TPR; o <<= 1) out[j] += __shfl_xor(out[j], o);
    }
    if (part != 0) return;
    const int64_t dst = seat_row_at(hd, rows, n, m0 + r);
    if (dst < 0) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = out[j] + theta[L.b3 + j];
    *reinterpret_cast<float4*>(a.verdict + ((size_t)dst * hd.n_members + k) * 4) = make_float4(out[0], out[1], out[2], out[3]);
}
