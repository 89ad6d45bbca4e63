// Part of learn_fused.hip: the hidden-layer pass of a seated bank -- both tanh layers of every JUDGE on the rows of its list, kept
// instead of discarded (copo_hidden_obs_seats_f32; eval/similarity.py, DESIGN.md section 8w).  The fourth mode of the bank's forward, in
// the jury's launch shape: the jury pass (learn_jury.inc) ends in the four head outputs of a row, this one ends one step earlier.
// ------------------------------------------------------------------------------------------------------------
// Judge j = blockIdx.y owns the list rows[j cap .. j cap + counts[j]) of [0, n_out), as in the jury pass.  Per listed row r at position
// p of the list, with o the TRUE row obs_src[r] and member j's parameters:
//     h1 = tanh(W1 o + b1) -> hidden[j][p][0][0..H),   h2 = tanh(W2 h1 + b2) -> hidden[j][p][1][0..H)
// -- the bits jury_obs_kernel holds in its h1s / h2s tiles for that judge and row: the prologue is learn_seat.inc's (same masking), and
// layers 1 and 2 are the one-tile forward body, a copy of jury_obs_kernel's (itself a copy of mlp_fwd_kernel's) on purpose, statement
// by statement up to the barrier behind the h2 tile.  A tile row's sums read that row's LDS rows only, so the bits do not depend on
// which other rows share the tile.  No heads: verdict[row][judge] is the jury pass's to write.
// The workspace is indexed by POSITION, not by row: hidden fp32 [n_members][cap][2][H], unit fastest -- what the Gram kernel
// (cka_kernels.hip) stages with 128-bit loads, sixteen lanes on 256 consecutive bytes of one position.
// Launch shape of seat mode: grid ceil(cap / 16) x n_members, always the 16-row tile; a workgroup past counts[j] leaves at once, before
// any weight load; positions at or past counts[j] -- the masked rows of a last, partial tile among them -- and positions whose row index
// lies outside [0, n_out) are not written.  No sampling, no atomics, fixed summation order: two launches give the same bits.
// LDS: h1 and h2 tiles [16][H + 4], the input tile [16][k1p + 4], the two mean rows of W3 (seat_stage brings them; unused here).
// ------------------------------------------------------------------------------------------------------------
struct HiddenArgs {
    SeatHead h;
    float* hidden;            // [n_members][cap][2][H]
};

__device__ __host__ inline size_t hidden_lds_floats(int H, int k1p) { return (size_t)2 * HT * (H + 4) + (size_t)HT * (k1p + 4) + 2 * H; }

template <int NT, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) hidden_obs_kernel(HiddenArgs a) {
    extern __shared__ float4 hidden_lds[];
    constexpr int H = 16 * NT * WAVES, HP = H + 4, TH = 64 * WAVES;
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
    float* h1s = reinterpret_cast<float*>(hidden_lds);    // [HT][HP]
    float* h2s = h1s + HT * HP;                           // [HT][HP]
    float* xs = h2s + HT * HP;                            // [HT][XP]  the true observation rows, zero beyond K1
    float* w3s = xs + HT * XP;                            // [2][H]
    BRing<NT, DB, false> ring;
    ring.start(theta_t + L.w1, H, cb, ln, lj);
    seat_stage<TH>(hd, rows, n, m0, theta, H, xs, w3s, tid);
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
    // ---- both tiles out, 128 bits per thread and store: [position][layer][unit].  A position without a row is skipped. ----
    constexpr int Q = H / 4;
    for (int i = tid; i < HT * 2 * Q; i += TH) {
        const int row = i / (2 * Q), rem = i - row * (2 * Q), layer = rem / Q, u = (rem - layer * Q) * 4;
        if (seat_row_at(hd, rows, n, m0 + row) < 0) continue;
        const float4 v = *reinterpret_cast<const float4*>((layer ? h2s : h1s) + row * HP + u);
        *reinterpret_cast<float4*>(a.hidden + (((k * (size_t)hd.cap + (size_t)(m0 + row)) * 2 + layer) * H + u)) = v;
    }
}
