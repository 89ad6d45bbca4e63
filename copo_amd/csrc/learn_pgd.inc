// Part of learn_fused.hip: the iterated form of learn_inputgrad.inc -- projected gradient descent (PGD) on the LiDAR block of the
// observation of a seated bank, the whole iteration resident in one workgroup (copo_pgd_obs_seats_f32; eval/pgd.py, DESIGN.md
// section 8n).  adv_obs_kernel cannot be chained to get this: each of its launches projects around its INPUT, not around the true row.
// ------------------------------------------------------------------------------------------------------------
// Per row r of member k's list, level = levels[level_of[group[r / n_slots]][k]] = eight words: eps, steer, throttle, alpha (f32),
// iters, flags (i32; bit 0 RANDOM_START, bit 1 UNTARGETED), two zeros.  it = min(iters, max_iters).
//     x_0 = o; with RANDOM_START on the columns [col_lo, col_hi): x_0[j] = clamp(o[j] + eps u, 0, 1), u = 2 uniform01(h) - 1 (exact),
//           h = hash_rng(seed, r, tick[r], j - col_lo, 40)                      (sim_math.h; stream 40)
//     for i < it:  g_i = W1^T (d1 * W2^T (d2 * W3[:2]^T c)) at x_i, as adv_obs_kernel; c = (steer, throttle), or, UNTARGETED,
//           c = mu(x_i) - mu(o) (J = 1/2 |mu(x) - mu(o)|^2; mu(o) from one clean forward pass of the tile, run only if it holds such a row)
//           y = x_i[j] + alpha sign(g_i[j]); y = min(max(y, o[j] - eps), o[j] + eps); x_{i+1}[j] = min(max(y, 0), 1)   on the columns
//     obs_seen = x_it; every other column is o[j] bit for bit.  Sums and products one rounding each (__fadd_rn / __fmul_rn).
// tick (int32 [n_out] or NULL = 0): the thread that looks a listed valid row up reads tick[r] and writes tick[r] + 1 back, at every
// level; a row sits in one member's list at the most (the seat plan's contract), so nothing races.
// trace (float [max_iters][n_out][in_dim] or NULL): g_i of every attacked row for i < it, zeros for later iterations and for listed
// rows that pass through.
// Launch shape, prologue (learn_seat.inc) and modes are adv_obs_kernel's: grid ceil(cap / 16) x n_members, 16-row tile, a workgroup past counts[k]
// leaves before its first barrier, the last tile is masked, modes per ROW:
//     PGD_SKIP    no row here: nothing is written
//     PGD_COPY    level or group out of range, eps == 0, it <= 0, or targeted with steer == throttle == 0: obs_seen = o, no arithmetic
//     PGD_ATTACK  the row iterates
// A tile without a PGD_ATTACK row copies and leaves.  New against adv_obs_kernel: a second input tile xp holds the iterate (xs keeps
// the true rows for the projection), layer 1 reads xp, the workgroup loops to the largest `it` of its tile (read from LDS: uniform),
// a row past its own `it` is masked out of seed, trace and update, the last GEMM's accumulators update xp in place of going to
// global memory, and obs_seen is stored once behind the loop.  The clean pass of an untargeted tile is iteration -1 of the same
// loop body on xs.  The head means are 32 dot products of length H per pass: eight lanes each, every lane a strided partial in
// ascending order, then a three-level xor tree -- a fixed order.  No atomics: two launches from the same tick give the same bits.
// The forward body is a copy of mlp_fwd_kernel's, as adv_obs_kernel's is (see there).
// ------------------------------------------------------------------------------------------------------------
struct PgdArgs {
    SeatHead h;               // levels [n_levels][8]: eps, steer, throttle, alpha, iters (i32), flags (i32), 0, 0
    float* obs_seen;          // [n_out][in_dim]
    float* trace;             // [max_iters][n_out][in_dim] or NULL
    uint64_t seed;
    int32_t* tick;            // [n_out] or NULL
    int32_t max_iters;
};

constexpr int PGD_SKIP = 0, PGD_COPY = 1, PGD_ATTACK = 2;
constexpr int PGD_RANDOM_START = 1, PGD_UNTARGETED = 2, PGD_MAX_ITERS = 16, PGD_LEVEL_WORDS = 8;
constexpr uint32_t PGD_STREAM = 40;            // the simulator draws on streams 1..4 and 16, the faults on 32..37
__device__ __host__ inline size_t pgd_lds_floats(int H, int k1p) { return adv_lds_floats(H, k1p) + (size_t)HT * (k1p + 4); }

template <int NT, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) pgd_obs_kernel(PgdArgs a) {
    extern __shared__ float4 pgd_lds[];
    __shared__ int64_t dst_s[HT];          // where a tile row's outputs go
    __shared__ float lvl_s[HT][4];         // eps, steer, throttle, alpha of the row's level
    __shared__ float c_s[HT][2];           // the seed's coefficients: (steer, throttle), or mu(x_i) - mu(o)
    __shared__ float mu0_s[HT][2];         // mu(o) of an untargeted tile
    __shared__ int mode_s[HT], it_s[HT], flag_s[HT], tick_s[HT];
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
    float* h1s = reinterpret_cast<float*>(pgd_lds);     // [HT][HP]  h1, then u1
    float* h2s = h1s + HT * HP;                         // [HT][HP]  h2, then u2
    float* xs = h2s + HT * HP;                          // [HT][XP]  the true observation rows, zero beyond K1
    float* w3s = xs + HT * XP;                          // [2][H]    the two mean rows of W3
    float* xp = w3s + 2 * H;                            // [HT][XP]  the iterate
    if (tid < HT) {
        const int64_t r = seat_row_at(hd, rows, n, m0 + tid);
        int mode = r < 0 ? PGD_SKIP : PGD_COPY, it = 0, flags = 0, tk = 0;
        float e = 0.0f, s = 0.0f, t = 0.0f, al = 0.0f;
        if (r >= 0) {
            if (a.tick) {
                tk = a.tick[r];
                a.tick[r] = tk + 1;
            }
            const int lv = seat_level_at(hd, k, r);
            if (lv >= 0) {
                const float* w = hd.levels + (size_t)PGD_LEVEL_WORDS * lv;
                e = w[0]; s = w[1]; t = w[2]; al = w[3];
                it = __float_as_int(w[4]); flags = __float_as_int(w[5]);
                it = it < a.max_iters ? it : a.max_iters;
                if (e != 0.0f && it > 0 && ((flags & PGD_UNTARGETED) || s != 0.0f || t != 0.0f)) mode = PGD_ATTACK;
            }
        }
        dst_s[tid] = r < 0 ? 0 : r;
        mode_s[tid] = mode;
        it_s[tid] = mode == PGD_ATTACK ? it : 0;
        flag_s[tid] = mode == PGD_ATTACK ? flags : 0;
        tick_s[tid] = tk;
        lvl_s[tid][0] = e; lvl_s[tid][1] = s; lvl_s[tid][2] = t; lvl_s[tid][3] = al;
        const bool aimed = mode == PGD_ATTACK && !(flags & PGD_UNTARGETED);
        c_s[tid][0] = aimed ? s : 0.0f; c_s[tid][1] = aimed ? t : 0.0f;
        mu0_s[tid][0] = 0.0f; mu0_s[tid][1] = 0.0f;
    }
    seat_stage<TH>(hd, rows, n, m0, theta, H, xs, w3s, tid);
    __syncthreads();
    int itmax = 0;             // (the same sixteen words for every thread: uniform)
    bool any_unt = false;
#pragma unroll
    for (int i = 0; i < HT; ++i) {
        itmax = it_s[i] > itmax ? it_s[i] : itmax;
        any_unt = any_unt || (flag_s[i] & PGD_UNTARGETED);
    }
    // obs_seen of the tile's rows from `src`, once; the trace's iterations from `from` on are zeros
    auto store_rows = [&](const float* src, int from) {
        for (int i = tid; i < HT * K1; i += TH) {
            const int row = i / K1, col = i - row * K1;
            if (mode_s[row] == PGD_SKIP) continue;
            const size_t at = (size_t)dst_s[row] * K1 + col;
            a.obs_seen[at] = src[row * XP + col];
            if (a.trace)
                for (int j = from; j < a.max_iters; ++j) a.trace[(size_t)j * hd.n_out * K1 + at] = 0.0f;
        }
    };
    if (itmax <= 0) {          // every row passes through: copy, no GEMM
        store_rows(xs, 0);
        return;
    }
    // ---- start: x_0 = o, a uniform draw inside the budget on the LiDAR columns of the rows that ask for one ----
    for (int i = tid; i < HT * K1P; i += TH) {
        const int row = i / K1P, kk = i - row * K1P;
        float v = xs[row * XP + kk];
        if ((flag_s[row] & PGD_RANDOM_START) && kk >= hd.col_lo && kk < hd.col_hi) {      // (flags are zero off the attacked rows)
            const uint32_t h = hash_rng(a.seed, (uint32_t)dst_s[row], (uint32_t)tick_s[row], (uint32_t)(kk - hd.col_lo), PGD_STREAM);
            const float u = __fadd_rn(__fmul_rn(2.0f, uniform01(h)), -1.0f);
            v = fminf(fmaxf(__fadd_rn(v, __fmul_rn(lvl_s[row][0], u)), 0.0f), 1.0f);
        }
        xp[row * XP + kk] = v;
    }
    __syncthreads();
    v4f acc[1][NT];
    const float* const theta0 = theta;
    const float* const theta_t0 = theta_t;
    for (int it = any_unt ? -1 : 0; it < itmax; ++it) {          // -1: the clean pass, mu(o) of the true rows
        // the weights' addresses are made opaque per iteration: every load of the body is loop-invariant, and hoisted out of the loop
        // (the optimiser does so in the copy of the loop it makes for trace == NULL) they cost hundreds of registers and spill
        const float* theta = theta0;
        const float* theta_t = theta_t0;
        asm volatile("" : "+s"(theta), "+s"(theta_t));
        BRing<NT, DB, false> ring;          // requested per pass: a ring carried round the loop is copied at the back edge and spills
        ring.start(theta_t + L.w1, H, cb, ln, lj);
        const float* in = it < 0 ? xs : xp;
        // ---- forward: layers 1 and 2 ----
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[0][t] = v4f{0.f, 0.f, 0.f, 0.f};
        ring.template run_tiles<1>(in, XP, (K1 + 15) & ~15, ln, lj, acc);
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
        // W2 as stored: the B operand of u2 W2, requested under the seed below (the clean pass ends at the means)
        if (it >= 0) ring.start(theta + L.w2, H, cb, ln, lj);
        __syncthreads();
        if (any_unt) {
            // ---- the two action means of every row: eight lanes per dot product, ascending strided partials, xor tree ----
            if (tid < 16 * HT) {
                const int row = tid >> 4, j = (tid >> 3) & 1, q = tid & 7;
                float s = 0.0f;
                for (int col = q; col < H; col += 8) s += h2s[row * HP + col] * w3s[j * H + col];
                s += __shfl_xor(s, 4);
                s += __shfl_xor(s, 2);
                s += __shfl_xor(s, 1);
                const float mu = s + theta[L.b3 + j];
                if (q == 0) {
                    if (it < 0) mu0_s[row][j] = mu;
                    else if (flag_s[row] & PGD_UNTARGETED) c_s[row][j] = mu - mu0_s[row][j];
                }
            }
            __syncthreads();
            if (it < 0) continue;
        }
        // ---- seed: u2 = (1 - h2^2) (c_0 W3[0] + c_1 W3[1]), in place of h2; rows that do not iterate (any more) get zeros ----
        for (int i = tid; i < HT * H; i += TH) {
            const int row = i / H, col = i - row * H;
            const float h = h2s[row * HP + col];
            const bool on = it < it_s[row];
            const float c0 = on ? c_s[row][0] : 0.0f, c1 = on ? c_s[row][1] : 0.0f;
            h2s[row * HP + col] = (1.0f - h * h) * (c0 * w3s[col] + c1 * w3s[H + col]);
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
        // ---- g = u1 W1 with W1 as stored, as adv_obs_kernel; the accumulators step and project the iterate in xp ----
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
                const int i = 4 * lj + rr;
                if (mode_s[i] == PGD_SKIP) continue;
                const bool on = it < it_s[i];
                const float gv = on ? g[rr] : 0.0f;
                if (a.trace) a.trace[((size_t)it * hd.n_out + dst_s[i]) * K1 + col] = gv;
                if (on && lidar) {
                    const float x = xp[i * XP + col], o = xs[i * XP + col], e = lvl_s[i][0], al = lvl_s[i][3];
                    const float sg = gv > 0.0f ? 1.0f : gv < 0.0f ? -1.0f : 0.0f;
                    float y = __fadd_rn(x, __fmul_rn(al, sg));
                    y = fminf(fmaxf(y, __fadd_rn(o, -e)), __fadd_rn(o, e));
                    xp[i * XP + col] = fminf(fmaxf(y, 0.0f), 1.0f);
                }
            }
        }
        __syncthreads();          // xp is layer 1's operand, h1s its output
    }
    store_rows(xp, itmax);
}
