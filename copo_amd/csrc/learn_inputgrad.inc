// Part of learn_fused.hip: the policy net differentiated with respect to its INPUT, for a seated bank (copo_adv_obs_seats_f32;
// eval/adversary.py, DESIGN.md section 8m).  The learner's backward pass stops at the layer-1 weight gradient -- training never needs
// dJ/d obs -- so this is the one kernel here that carries a gradient down to the observation row.
// ------------------------------------------------------------------------------------------------------------
// Per row of member k's list, with the row's level (eps, steer, throttle) = levels[level_of[group[row / n_slots]][k]]:
//     h1 = tanh(W1 o + b1), h2 = tanh(W2 h1 + b2)                  forward, as mlp_fwd_kernel (W1 / W2 from the transposed mirror)
//     u2 = (1 - h2^2) (steer W3[0] + throttle W3[1])               seed: d J / d z2, J = steer mu_0 + throttle mu_1
//     u1 = (u2 W2) (1 - h1^2)                                      W2 as stored, [out][in] = [k][n]
//     g  = u1 W1                                                   W1 as stored, [H][in_dim] = [k][n], n padded to 16-column tiles
//     obs_seen[j] = clamp(o[j] + eps sign(g[j]), 0, 1) on columns [col_lo, col_hi), o[j] elsewhere; grad = g (optional)
// Launch shape of seat mode: grid ceil(cap / 16) x n_members, the member owns its row list, a workgroup past counts[k] leaves before
// its first barrier, the last tile is masked.  Always the 16-row tile.  h1 / h2 stay in LDS; u2 overwrites h2 and u1 overwrites h1 in
// place (element by element, by the thread that owns the element), so the backward half needs no LDS of its own; the last GEMM's
// accumulators go straight to obs_seen / grad (16 lanes write 16 adjacent columns of a row).
// Modes of a row (selected per ROW: one tile can hold rows of several levels):
//     ADV_SKIP   no row here (past the member's count, or an index outside [0, n_out)): nothing is written
//     ADV_COPY   level index outside [0, L), group outside [0, G), steer == throttle == 0, or eps == 0 without a `grad` output:
//                obs_seen = o bit for bit (no arithmetic), grad = 0
//     ADV_GRAD   the gradient is needed: for the perturbation (eps != 0) or for `grad` alone (eps == 0: obs_seen = o bit for bit)
// A tile without an ADV_GRAD row copies and leaves before the GEMMs (uniform over the workgroup).  No atomics, fixed summation order.
// The argument head and the tile prologue (row and level look-up, the staging of the true rows and of W3) are learn_seat.inc's, shared
// with pgd_obs_kernel, cert_obs_kernel and lin_obs_kernel; the resource report of all sixteen instantiations is what it was with a copy each.
// The forward body is a copy of mlp_fwd_kernel's on purpose: a __device__ body shared with it changed the register allocation of the
// hidden-512 forward kernels (see there).
// ------------------------------------------------------------------------------------------------------------
struct AdvArgs {
    SeatHead h;               // levels [n_levels][4]: eps, steer, throttle, 0
    float* obs_seen;          // [n_out][in_dim]
    float* grad;              // [n_out][in_dim] or NULL
};

constexpr int ADV_SKIP = 0, ADV_COPY = 1, ADV_GRAD = 2;
__device__ __host__ inline size_t adv_lds_floats(int H, int k1p) { return (size_t)2 * HT * (H + 4) + (size_t)HT * (k1p + 4) + 2 * H; }

template <int NT, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) adv_obs_kernel(AdvArgs a) {
    extern __shared__ float4 adv_lds[];
    __shared__ int64_t dst_s[HT];          // where a tile row's outputs go
    __shared__ float lvl_s[HT][4];         // eps, steer, throttle of the row's level
    __shared__ int mode_s[HT];
    constexpr int H = 16 * NT * WAVES, HP = H + 4, TH = 64 * WAVES;
    constexpr int DB = NT >= 8 ? 4 : (H / 16 >= 8 ? 8 : H / 16);
    const SeatHead& hd = a.h;
    const copo_ppo_cfg& c = hd.c;
    const size_t k = blockIdx.y;
    const int64_t n = hd.counts[k] < hd.cap ? hd.counts[k] : hd.cap;      // (a list holds `cap` rows at the most)
    const int64_t m0 = (int64_t)blockIdx.x * HT;
    if (m0 >= n) return;
    const float* theta = hd.theta + k * hd.member_stride;
    const float* theta_t = hd.theta_t + k * hd.member_stride;
    const int64_t* rows = hd.rows + k * (size_t)hd.cap;
    const copo_net_layout L = c.pol;
    const int K1 = L.in_dim, K1P = rowpass_k1p(K1), XP = K1P + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 15, lj = lane >> 4, cb = wave * (16 * NT);
    float* h1s = reinterpret_cast<float*>(adv_lds);     // [HT][HP]  h1, then u1
    float* h2s = h1s + HT * HP;                         // [HT][HP]  h2, then u2
    float* xs = h2s + HT * HP;                          // [HT][XP]  the true observation rows, zero beyond K1
    float* w3s = xs + HT * XP;                          // [2][H]    the two mean rows of W3
    BRing<NT, DB, false> ring;
    ring.start(theta_t + L.w1, H, cb, ln, lj);
    if (tid < HT) {
        const int64_t r = seat_row_at(hd, rows, n, m0 + tid);
        int mode = r < 0 ? ADV_SKIP : ADV_COPY;
        float e = 0.0f, s = 0.0f, t = 0.0f;
        if (r >= 0) {
            const int lv = seat_level_at(hd, k, r);
            if (lv >= 0) {
                e = hd.levels[4 * lv]; s = hd.levels[4 * lv + 1]; t = hd.levels[4 * lv + 2];
                if ((s != 0.0f || t != 0.0f) && (e != 0.0f || a.grad)) mode = ADV_GRAD;
            }
        }
        dst_s[tid] = r < 0 ? 0 : r;
        mode_s[tid] = mode;
        lvl_s[tid][0] = e; lvl_s[tid][1] = mode == ADV_GRAD ? s : 0.0f; lvl_s[tid][2] = mode == ADV_GRAD ? t : 0.0f; lvl_s[tid][3] = 0.0f;
    }
    seat_stage<TH>(hd, rows, n, m0, theta, H, xs, w3s, tid);
    __syncthreads();
    bool any = false;          // (the same sixteen words for every thread: uniform)
#pragma unroll
    for (int i = 0; i < HT; ++i) any = any || mode_s[i] == ADV_GRAD;
    if (!any) {                // every row passes through: copy, no GEMM
        for (int i = tid; i < HT * K1; i += TH) {
            const int row = i / K1, col = i - row * K1;
            if (mode_s[row] == ADV_SKIP) continue;
            const size_t at = (size_t)dst_s[row] * K1 + col;
            a.obs_seen[at] = xs[row * XP + col];
            if (a.grad) a.grad[at] = 0.0f;
        }
        return;
    }
    v4f acc[1][NT];
    // ---- forward: layers 1 and 2 (the heads are not needed: J's gradient starts at W3) ----
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
    ring.start(theta + L.w2, H, cb, ln, lj);       // W2 as stored: the B operand of u2 W2, requested under the seed below
    __syncthreads();
    // ---- seed: u2 = (1 - h2^2) (steer W3[0] + throttle W3[1]), in place of h2; rows without a gradient get zeros ----
    for (int i = tid; i < HT * H; i += TH) {
        const int row = i / H, col = i - row * H;
        const float h = h2s[row * HP + col];
        h2s[row * HP + col] = (1.0f - h * h) * (lvl_s[row][1] * w3s[col] + lvl_s[row][2] * w3s[H + col]);
    }
    __syncthreads();
    // ---- u1 = (u2 W2) (1 - h1^2), in place of h1 ----
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[0][t] = v4f{0.f, 0.f, 0.f, 0.f};
    ring.template run_tiles<1>(h2s, HP, H, ln, lj, acc);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = cb + NT * ln + t;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const float h = h1s[(4 * lj + rr) * HP + col];
            h1s[(4 * lj + rr) * HP + col] = acc[0][t][rr] * (1.0f - h * h);
        }
    }
    __syncthreads();
    // ---- g = u1 W1 with W1 as stored: 16-column tiles of the input, dealt to the waves; lane group lj takes k = 16 s + 4 lj + {0..3}
    // of every step, 16 lanes read 16 adjacent floats of a weight row.  Columns beyond in_dim read the last column and are not stored.
    const int ntile = (K1 + 15) >> 4;
    for (int tile = wave; tile < ntile; tile += WAVES) {
        const int col = 16 * tile + ln;
        const float* wp = theta + L.w1 + (size_t)(4 * lj) * K1 + (col < K1 ? col : K1 - 1);
        const float* arow = h1s + ln * HP + 4 * lj;
        v4f g = {0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < H / 16; s0 += 4) {       // four steps' loads in flight (H / 16 is a multiple of 4)
            float b[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) b[u][e] = wp[(size_t)(16 * (s0 + u) + e) * K1];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 a4 = *reinterpret_cast<const float4*>(arow + 16 * (s0 + u));
                const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) g = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], b[u][e], g, 0, 0, 0);
            }
        }
        if (col >= K1) continue;
        const bool lidar = col >= hd.col_lo && col < hd.col_hi;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int i = 4 * lj + rr, mode = mode_s[i];
            if (mode == ADV_SKIP) continue;
            const size_t at = (size_t)dst_s[i] * K1 + col;
            const float o = xs[i * XP + col], gv = mode == ADV_GRAD ? g[rr] : 0.0f, e = lvl_s[i][0];
            float seen = o;
            if (mode == ADV_GRAD && lidar && e != 0.0f) {
                const float sg = gv > 0.0f ? 1.0f : gv < 0.0f ? -1.0f : 0.0f;
                seen = fminf(fmaxf(o + e * sg, 0.0f), 1.0f);
            }
            a.obs_seen[at] = seen;
            if (a.grad) a.grad[at] = gv;
        }
    }
}
