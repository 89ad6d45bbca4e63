// Part of learn_fused.hip: input attribution of a seated bank by integrated gradients (IG) -- which observation columns a policy's two
// action means rest on, in units of action (copo_ig_obs_seats_f32; eval/attribution.py, DESIGN.md section 8v).  It composes three of its
// neighbours: learn_inputgrad.inc's backward pass down to the whole observation row, learn_pgd.inc's tile that stays resident while
// forward and backward run many times, and both action heads per pass as learn_linbound.inc carries them.
// ------------------------------------------------------------------------------------------------------------
// Per row r of member k's list, level = levels[level_of[group[r / n_slots]][k]] = four words: m (i32, the quadrature points), flags
// (i32, reserved, 0), two zeros; mm = min(m, max_points).  base [n_levels][in_dim] (f32) is the level's baseline row; a NaN entry means
// "this column keeps the row's own value".  With o the TRUE row, b[j] = isnan(base[j]) ? o[j] : base[j] and d = o - b (rounded once):
//     x_s   = b + ((s - 1/2) / mm) d                       s = 1 .. mm (midpoint rule); quotient, product and sum rounded once each
//     G_a   = sum_s d mu_a / d x at x_s                    a = 0 (steer), 1 (throttle); s ascending, one rounding per add (G = g at s = 1)
//     attr_a[j] = (d[j] G_a[j]) / mm                       product and quotient rounded once each; exactly 0.0 where d[j] == 0
//     gap_a = (mu_a(o) - mu_a(b)) - sum_j attr_a[j]        j ascending from 0.0, one rounding per add: the quadrature residual
// d mu_a / d x = W1^T (d1 * W2^T (d2 * W3[a])) as adv_obs_kernel computes it for the seed (steer, throttle) = e_a: forward from the
// transposed mirror, backward on the weights as stored.
// Outputs: attr [n_out][2][in_dim]; heads [n_out][8] = mu_0(o), mu_1(o), mu_0(b), mu_1(b), gap_0, gap_1, valid (1.0 / 0.0), mm as bits.
// Launch shape, prologue (learn_seat.inc) and the way modes are chosen per ROW are adv_obs_kernel's: grid ceil(cap / 16) x n_members,
// 16-row tile, a workgroup past counts[k] leaves before its first barrier, the last tile is masked:
//     IG_SKIP   no row here: nothing is written
//     IG_ZERO   level or group out of range, or mm <= 0: attr = 0, heads = 0 (valid = 0)
//     IG_ATTR   the row is attributed
// A tile without an IG_ATTR row writes its zeros and leaves before the GEMMs.
// The loop: pass -2 is the forward of the true rows (xs) up to the means, pass -1 that of the baseline rows (xb), passes 0 .. mmax - 1
// (mmax: the largest mm of the tile, read from LDS: uniform) build the tile's points in xp, run layers 1 and 2 ONCE and then the two
// heads' backward passes one after the other.  The heads are run in sequence, not stacked against one weight stream: a head's seed and
// its u1 live in a third hidden tile `us`, so that h1 / h2 survive for the second head -- three hidden tiles, three input tiles and the
// running sum G [2][16][in] are 142 KB of LDS at hidden 512 with a 128-column input; stacking needs a fourth hidden tile, 174 KB, which
// a compute unit does not have.  G stays in LDS across the passes: element (head, row, column) is owned by one lane of the last GEMM.
// A row past its own mm is masked out of the seed and of the sum.  The means are reduced in pgd_obs_kernel's fixed lane order.  No
// atomics: two launches give the same bits.  The forward body is a copy of mlp_fwd_kernel's, as adv_obs_kernel's is (see there).
// ------------------------------------------------------------------------------------------------------------
struct IgArgs {
    SeatHead h;               // levels [n_levels][4]: m (i32), flags (i32, 0), 0, 0
    float* attr;              // [n_out][2][in_dim]
    float* heads;             // [n_out][8]
    const float* base;        // [n_levels][in_dim], NaN = keep the row's own value
    int32_t max_points;
};

constexpr int IG_SKIP = 0, IG_ZERO = 1, IG_ATTR = 2;
constexpr int IG_MAX_POINTS = 32, IG_LEVEL_WORDS = 4, IG_HEAD_WORDS = 8;
__device__ __host__ inline size_t ig_lds_floats(int H, int k1p) { return (size_t)3 * HT * (H + 4) + (size_t)5 * HT * (k1p + 4) + 2 * H; }

template <int NT, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) ig_obs_kernel(IgArgs a) {
    extern __shared__ float4 ig_lds[];
    __shared__ int64_t dst_s[HT];          // where a tile row's outputs go
    __shared__ float mu_s[HT][4];          // mu_0(o), mu_1(o), mu_0(b), mu_1(b)
    __shared__ int mode_s[HT], m_s[HT], lv_s[HT];
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
    float* h1s = reinterpret_cast<float*>(ig_lds);      // [HT][HP]  h1 of the pass
    float* h2s = h1s + HT * HP;                         // [HT][HP]  h2 of the pass
    float* us = h2s + HT * HP;                          // [HT][HP]  a head's u2, then its u1
    float* xs = us + HT * HP;                           // [HT][XP]  the true observation rows, zero beyond K1
    float* w3s = xs + HT * XP;                          // [2][H]    the two mean rows of W3
    float* xb = w3s + 2 * H;                            // [HT][XP]  the baseline rows b
    float* xp = xb + HT * XP;                           // [HT][XP]  the points x_s of the pass
    float* gs = xp + HT * XP;                           // [2][HT][XP]  G, at the end attr
    if (tid < HT) {
        const int64_t r = seat_row_at(hd, rows, n, m0 + tid);
        int mode = r < 0 ? IG_SKIP : IG_ZERO, mm = 0, lv = 0;
        if (r >= 0) {
            lv = seat_level_at(hd, k, r);
            if (lv >= 0) {
                mm = __float_as_int(hd.levels[(size_t)IG_LEVEL_WORDS * lv]);
                mm = mm < a.max_points ? mm : a.max_points;
                if (mm > 0) mode = IG_ATTR;
            }
        }
        dst_s[tid] = r < 0 ? 0 : r;
        mode_s[tid] = mode;
        m_s[tid] = mode == IG_ATTR ? mm : 0;
        lv_s[tid] = mode == IG_ATTR ? lv : 0;
        mu_s[tid][0] = 0.0f; mu_s[tid][1] = 0.0f; mu_s[tid][2] = 0.0f; mu_s[tid][3] = 0.0f;
    }
    seat_stage<TH>(hd, rows, n, m0, theta, H, xs, w3s, tid);
    __syncthreads();
    int mmax = 0;              // (the same sixteen words for every thread: uniform)
#pragma unroll
    for (int i = 0; i < HT; ++i) mmax = m_s[i] > mmax ? m_s[i] : mmax;
    if (mmax <= 0) {           // nothing to attribute: zeros, no GEMM
        for (int i = tid; i < HT * 2 * K1; i += TH) {
            const int row = i / (2 * K1);
            if (mode_s[row] != IG_SKIP) a.attr[(size_t)dst_s[row] * 2 * K1 + (i - row * 2 * K1)] = 0.0f;
        }
        for (int i = tid; i < HT * IG_HEAD_WORDS; i += TH)
            if (mode_s[i / IG_HEAD_WORDS] != IG_SKIP) a.heads[(size_t)dst_s[i / IG_HEAD_WORDS] * IG_HEAD_WORDS + (i % IG_HEAD_WORDS)] = 0.0f;
        return;
    }
    // ---- the baseline rows: the level's row where it is a number, the row's own value where it is NaN (and on rows not attributed) ----
    for (int i = tid; i < HT * K1P; i += TH) {
        const int row = i / K1P, kk = i - row * K1P;
        float v = xs[row * XP + kk];
        if (mode_s[row] == IG_ATTR && kk < K1) {
            const float bv = a.base[(size_t)lv_s[row] * K1 + kk];
            v = bv != bv ? v : bv;
        }
        xb[row * XP + kk] = v;
    }
    v4f acc[1][NT];
    const float* const theta0 = theta;
    const float* const theta_t0 = theta_t;
    for (int p = -2; p < mmax; ++p) {          // -2: mu(o), -1: mu(b), then the point s = p + 1
        // the weights' addresses are made opaque per pass and the ring is requested per pass, as in pgd_obs_kernel (see there)
        const float* theta = theta0;
        const float* theta_t = theta_t0;
        asm volatile("" : "+s"(theta), "+s"(theta_t));
        BRing<NT, DB, false> ring;
        ring.start(theta_t + L.w1, H, cb, ln, lj);
        if (p >= 0) {
            for (int i = tid; i < HT * K1P; i += TH) {
                const int row = i / K1P, kk = i - row * K1P;
                const float b = xb[row * XP + kk], d = __fsub_rn(xs[row * XP + kk], b);
                const int mm = m_s[row] > 0 ? m_s[row] : 1;
                const float cs = __fdiv_rn((float)(p + 1) - 0.5f, (float)mm);
                xp[row * XP + kk] = __fadd_rn(b, __fmul_rn(cs, d));
            }
        }
        __syncthreads();          // xb (first pass) / xp are layer 1's operand
        const float* in = p == -2 ? xs : p == -1 ? xb : xp;
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
        __syncthreads();
        if (p < 0) {
            // ---- the two action means of every row: eight lanes per dot product, ascending strided partials, xor tree ----
            if (tid < 16 * HT) {
                const int row = tid >> 4, j = (tid >> 3) & 1, q = tid & 7;
                float s = 0.0f;
                for (int col = q; col < H; col += 8) s += h2s[row * HP + col] * w3s[j * H + col];
                s += __shfl_xor(s, 4);
                s += __shfl_xor(s, 2);
                s += __shfl_xor(s, 1);
                if (q == 0) mu_s[row][2 * (p + 2) + j] = s + theta[L.b3 + j];
            }
            __syncthreads();          // (h2s is written again by the next pass)
            continue;
        }
        for (int hh = 0; hh < 2; ++hh) {
            const float* th = theta0;
            asm volatile("" : "+s"(th));
            ring.start(th + L.w2, H, cb, ln, lj);       // W2 as stored: the B operand of u2 W2, requested under the seed below
            // ---- seed: u2 = (1 - h2^2) W3[hh]; rows that are not attributed (any more) get zeros ----
            for (int i = tid; i < HT * H; i += TH) {
                const int row = i / H, col = i - row * H;
                const float h = h2s[row * HP + col];
                us[row * HP + col] = p < m_s[row] ? (1.0f - h * h) * w3s[hh * H + col] : 0.0f;
            }
            __syncthreads();
            // ---- u1 = (u2 W2) (1 - h1^2), in place of u2 once every wave has read it ----
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[0][t] = v4f{0.f, 0.f, 0.f, 0.f};
            ring.template run_tiles<1>(us, HP, H, ln, lj, acc);
            __syncthreads();
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int col = cb + NT * ln + t;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const float h = h1s[(4 * lj + rr) * HP + col];
                    us[(4 * lj + rr) * HP + col] = acc[0][t][rr] * (1.0f - h * h);
                }
            }
            __syncthreads();
            // ---- g = u1 W1 with W1 as stored, as adv_obs_kernel; the accumulators go into G ----
            const int ntile = (K1 + 15) >> 4;
            for (int tile = wave; tile < ntile; tile += WAVES) {
                const int col = 16 * tile + ln;
                const float* wp = th + L.w1 + (size_t)(4 * lj) * K1 + (col < K1 ? col : K1 - 1);
                const float* arow = us + ln * HP + 4 * lj;
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
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int i = 4 * lj + rr;
                    if (p >= m_s[i]) continue;
                    float* at = gs + (hh * HT + i) * XP + col;
                    *at = p == 0 ? g[rr] : __fadd_rn(*at, g[rr]);
                }
            }
            __syncthreads();          // `us` is the next seed's, h1s / h2s / xp the next pass's
        }
    }
    // ---- attr = d G / mm in place of G and out; exactly 0.0 where d == 0 and on rows that are not attributed ----
    for (int i = tid; i < 2 * HT * K1; i += TH) {
        const int row = i / (2 * K1), rem = i - row * 2 * K1, hh = rem / K1, col = rem - hh * K1;
        float v = 0.0f;
        if (mode_s[row] == IG_ATTR) {
            const float d = __fsub_rn(xs[row * XP + col], xb[row * XP + col]);
            if (d != 0.0f) v = __fdiv_rn(__fmul_rn(d, gs[(hh * HT + row) * XP + col]), (float)m_s[row]);
        }
        gs[(hh * HT + row) * XP + col] = v;
        if (mode_s[row] != IG_SKIP) a.attr[(size_t)dst_s[row] * 2 * K1 + rem] = v;
    }
    __syncthreads();
    // ---- the residual of a (row, head): one thread, columns ascending; head 0's thread writes the row's other words ----
    if (tid < 2 * HT) {
        const int row = tid >> 1, hh = tid & 1;
        if (mode_s[row] != IG_SKIP) {
            float* out = a.heads + (size_t)dst_s[row] * IG_HEAD_WORDS;
            const bool on = mode_s[row] == IG_ATTR;
            float sum = 0.0f;
            if (on)
                for (int col = 0; col < K1; ++col) sum = __fadd_rn(sum, gs[(hh * HT + row) * XP + col]);
            out[4 + hh] = on ? __fsub_rn(__fsub_rn(mu_s[row][hh], mu_s[row][2 + hh]), sum) : 0.0f;
            out[hh] = on ? mu_s[row][hh] : 0.0f;
            out[2 + hh] = on ? mu_s[row][2 + hh] : 0.0f;
            out[6 + hh] = !on ? 0.0f : hh == 0 ? 1.0f : __int_as_float(m_s[row]);
        }
    }
}
