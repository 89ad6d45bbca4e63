// Part of learn_fused.hip: linear bound propagation through the policy net of a seated bank -- for every listed row a box that holds the
// two action MEANS under every perturbation of its LiDAR block inside an L-infinity budget, from ONE linear relaxation per tanh unit
// carried backward from each mean to the input box, intersected with the interval box of the same pass (copo_lin_obs_seats_f32;
// eval/certify.py method="linear", DESIGN.md section 8p).  learn_certify.inc is the interval pass alone.
// ------------------------------------------------------------------------------------------------------------
// Rows, levels, the input box (c0, r0) and the output words are learn_certify.inc's.  Per certified row:
//     forward, layer i = 1, 2:  zc = W_i c_{i-1} + b_i, zr = |W_i| r_{i-1};  l = zc - zr, u = zc + zr (exact for the box at layer 1);
//                               tl = tanh(l), tu = max(tanh(u), tl);  c_i = (tl + tu) / 2, r_i = (tu - tl) / 2
//     a unit on [l, u]:         lam = max(min(1 - tl^2, 1 - tu^2), 0), betaL = tl - lam l, betaU = tu - lam u:
//                               lam z + betaL <= tanh z <= lam z + betaU on [l, u] (tanh' is unimodal: smallest at an end).  One slope for
//                               both sides, so the upper and the lower bound of a head share their backward coefficients: one pass per head
//     backward, head a = 0, 1:  v2 = W3[a], g2 = v2 lam2;  v1 = W2^T g2, g1 = v1 lam1;  v0 = W1^T g1
//                               base = b3[a] + g2 . b2 + g1 . b1 + v0 . c0, rad = |v0| . r0
//                               hiL = base + v2+ . betaU2 + v2- . betaL2 + v1+ . betaU1 + v1- . betaL1 + rad
//                               loL = base + v2+ . betaL2 + v2- . betaU2 + v1+ . betaL1 + v1- . betaU1 - rad
//     interval box:             loI = (mc - mr), hiI = (mc + mr) with mc = W3[a] . c2 + b3[a], mr = |W3[a]| . r2
//     per axis:                 lo = max(loL, loI), hi = min(hiL, hiI); lo > hi (rounding only, e.g. eps = 0): (loI, hiI); then pad (__fadd_rn)
//     bounds[r] = lo_0, hi_0, lo_1, hi_1, mu_0(o), mu_1(o), 1.0, eps;  parts[r] (optional) = loL_0, hiL_0, loL_1, hiL_1, loI_0, hiI_0, loI_1,
//     hiI_1 before the pad.  Invalid listed rows: eight zeros in both; rows in no list are never written.
// Launch shape, prologue (learn_seat.inc), masking, per-row modes and the three-tile forward are cert_obs_kernel's (the forward copied, as its
// body is mlp_fwd_kernel's).
// LDS is cert_obs_kernel's too -- three input tiles, three h1 tiles, the two mean rows of W3 -- at every hidden width, 512 included: layer
// 1's (l, u) are NOT kept across layer 2.  Where the backward pass needs them, the layer-1 GEMM of the centre and radius tiles (K = in_dim,
// the cheapest GEMM of the kernel) runs again, behind the W2 pass, into accumulators whose layout is that of v1: lam1 / beta1 are formed
// on the lanes.  The dead h1 tiles carry the backward operands: g2 of the two heads replaces the clean and the centre tile behind layer
// 2, g1 replaces g2 behind the W2 pass; both heads are stacked against ONE stream of W2 as stored and ONE of W1 as stored
// (adv_obs_kernel's backward half with two A tiles).  The last GEMM's accumulators meet c0 / r0, still in LDS.
// Every sum over units is a lane's ascending columns, a four-level xor tree over the sixteen lanes of a row, then the waves in wave order
// by one thread per row: no atomics, a fixed order -- two launches give the same bits.
// ------------------------------------------------------------------------------------------------------------
struct LinArgs {
    SeatHead h;               // levels [n_levels][4]: eps, delta_steer, delta_throttle, 0
    float* bounds;            // [n_out][8]
    float* parts;             // [n_out][8] or NULL
    float pad;
};

// a wave's share of a row's sums, per head a: behind layer 2  [6 a + 0..5] = mu, mc, mr, g2 . b2, hi-side v2 . beta2, lo-side v2 . beta2;
// behind the W2 pass [12 + 3 a + 0..2] = g1 . b1, hi-side v1 . beta1, lo-side v1 . beta1;  behind the W1 pass [18 + 2 a + 0..1] = v0 . c0, |v0| . r0
constexpr int LIN_P2 = 12, LIN_P1 = 6, LIN_P0 = 4, LIN_PARTS = LIN_P2 + LIN_P1 + LIN_P0;
__device__ __host__ inline size_t lin_lds_floats(int H, int k1p) { return cert_lds_floats(H, k1p); }

// lam, betaL, betaU of one unit from its pre-activation interval [zc - zr, zc + zr]; also its post-activation ends
struct LinUnit { float tl, tu, lam, bl, bu; };
__device__ __forceinline__ LinUnit lin_relax(float zc, float zr) {
    LinUnit q;
    const float l = zc - zr, u = zc + zr;
    q.tl = tanh_fast(l);
    q.tu = fmaxf(tanh_fast(u), q.tl);
    q.lam = fmaxf(fminf(1.0f - q.tl * q.tl, 1.0f - q.tu * q.tu), 0.0f);
    q.bl = q.tl - q.lam * l;
    q.bu = q.tu - q.lam * u;
    return q;
}

template <int NP>
__device__ __forceinline__ void lin_row_sums(float (*part)[NP], float* dst, int ln, int lj) {      // dst: this wave's [HT][LIN_PARTS] at its slot
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            float s = part[rr][q];
            s += __shfl_xor(s, 8);
            s += __shfl_xor(s, 4);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 1);
            if (ln == 0) dst[(4 * lj + rr) * LIN_PARTS + q] = s;
        }
}

template <int NT, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) lin_obs_kernel(LinArgs a) {
    extern __shared__ float4 lin_lds[];
    __shared__ int64_t dst_s[HT];                  // where a tile row's outputs go
    __shared__ float eps_s[HT];
    __shared__ int mode_s[HT];
    __shared__ float part_s[WAVES][HT][LIN_PARTS];
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
    float* h1s = reinterpret_cast<float*>(lin_lds);     // [3][HT][HP]  h1 of the true row, centre and radius; then g2 / g1 of the two heads in [0], [1]
    float* xs = h1s + CERT_PASSES * HT * HP;            // [3][HT][XP]  the true rows (zero beyond K1), c0, r0
    float* w3s = xs + CERT_PASSES * HT * XP;            // [2][H]       the two mean rows of W3
    BRing<NT, DB, false> ring;
    ring.start(theta_t + L.w1, H, cb, ln, lj);
    if (tid < HT) {
        const int64_t r = seat_row_at(hd, rows, n, m0 + tid);
        int mode = r < 0 ? CERT_SKIP : CERT_ZERO;
        float e = 0.0f;
        if (r >= 0) {
            const int lv = seat_level_at(hd, k, r);
            if (lv >= 0) {
                e = hd.levels[4 * lv];
                mode = CERT_RUN;
            }
        }
        dst_s[tid] = r < 0 ? 0 : r;
        mode_s[tid] = mode;
        eps_s[tid] = mode == CERT_RUN ? e : 0.0f;
    }
    seat_stage<TH>(hd, rows, n, m0, theta, H, xs, w3s, tid);
    __syncthreads();
    bool any = false;          // (the same sixteen words for every thread: uniform)
#pragma unroll
    for (int i = 0; i < HT; ++i) any = any || mode_s[i] == CERT_RUN;
    if (!any) {                // every listed row is invalid: zeros, no GEMM
        for (int i = tid; i < HT * CERT_WORDS; i += TH) {
            const int row = i / CERT_WORDS;
            if (mode_s[row] == CERT_SKIP) continue;
            const size_t at = (size_t)dst_s[row] * CERT_WORDS + (i - row * CERT_WORDS);
            a.bounds[at] = 0.0f;
            if (a.parts) a.parts[at] = 0.0f;
        }
        return;
    }
    // ---- the input box: centre and radius tiles behind the true rows (rows that are not certified run at eps = 0) ----
    for (int i = tid; i < HT * K1P; i += TH) {
        const int row = i / K1P, kk = i - row * K1P;
        const float o = xs[row * XP + kk], e = eps_s[row];
        float c0 = o, r0 = 0.0f;
        if (kk >= hd.col_lo && kk < hd.col_hi) {
            const float lo = fmaxf(__fadd_rn(o, -e), 0.0f), hi = fminf(__fadd_rn(o, e), 1.0f);
            c0 = __fmul_rn(0.5f, __fadd_rn(lo, hi));
            r0 = __fmul_rn(0.5f, __fadd_rn(hi, -lo));
        }
        xs[(HT + row) * XP + kk] = c0;
        xs[(2 * HT + row) * XP + kk] = r0;
    }
    __syncthreads();
    const int k1r = (K1 + 15) & ~15;
    v4f acc[CERT_PASSES][NT];
    // ---- layer 1 on the three tiles ----
#pragma unroll
    for (int p = 0; p < CERT_PASSES; ++p)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[p][t] = v4f{0.f, 0.f, 0.f, 0.f};
    ring.template run_tiles_abs<CERT_PASSES, 4u>(xs, XP, k1r, ln, lj, acc);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = cb + NT * ln + t;
        const float bv = theta[L.b1 + col];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int row = 4 * lj + rr;
            const float zc = acc[1][t][rr] + bv, zr = acc[2][t][rr];
            const float l = tanh_fast(zc - zr), u = fmaxf(tanh_fast(zc + zr), l);
            h1s[row * HP + col] = tanh_fast(acc[0][t][rr] + bv);
            h1s[(HT + row) * HP + col] = 0.5f * (l + u);
            h1s[(2 * HT + row) * HP + col] = 0.5f * (u - l);
        }
    }
    ring.start(theta_t + L.w2, H, cb, ln, lj);
    __syncthreads();
    // ---- layer 2; its output stays on the lanes ----
#pragma unroll
    for (int p = 0; p < CERT_PASSES; ++p)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[p][t] = v4f{0.f, 0.f, 0.f, 0.f};
    ring.template run_tiles_abs<CERT_PASSES, 4u>(h1s, HP, H, ln, lj, acc);
    // the second ring and the early requests below need registers that NT = 4 does not have (they spilled): there every request waits
    // until the previous ring is dead
    constexpr bool EARLY = NT < 4;
    if constexpr (EARLY) ring.start(theta + L.w2, H, cb, ln, lj);       // W2 as stored: the B operand of g2 W2, requested under the epilogue below
    __syncthreads();                               // every wave is done with the h1 tiles: g2 may replace them
    {
        float part[4][LIN_P2];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int q = 0; q < LIN_P2; ++q) part[rr][q] = 0.0f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = cb + NT * ln + t;
            const float bv = theta[L.b2 + col];
            const float w[2] = {w3s[col], w3s[H + col]};
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const LinUnit q = lin_relax(acc[1][t][rr] + bv, acc[2][t][rr]);
                const float h = tanh_fast(acc[0][t][rr] + bv), cc = 0.5f * (q.tl + q.tu), rd = 0.5f * (q.tu - q.tl);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float g = w[j] * q.lam;
                    part[rr][6 * j + 0] += h * w[j];
                    part[rr][6 * j + 1] += cc * w[j];
                    part[rr][6 * j + 2] += rd * fabsf(w[j]);
                    part[rr][6 * j + 3] += g * bv;
                    part[rr][6 * j + 4] += w[j] * (w[j] > 0.0f ? q.bu : q.bl);
                    part[rr][6 * j + 5] += w[j] * (w[j] > 0.0f ? q.bl : q.bu);
                    h1s[(j * HT + 4 * lj + rr) * HP + col] = g;
                }
            }
        }
        lin_row_sums<LIN_P2>(part, &part_s[wave][0][0], ln, lj);
    }
    if constexpr (!EARLY) ring.start(theta + L.w2, H, cb, ln, lj);
    BRing<NT, DB, false> ring1;                    // W1^T again, for layer 1's intervals: requested in front of the W2 pass
    if constexpr (EARLY) ring1.start(theta_t + L.w1, H, cb, ln, lj);
    __syncthreads();
    // ---- v1 = g2 W2, the two heads stacked against one stream of W2 as stored ----
    v4f vac[2][NT];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t) vac[j][t] = v4f{0.f, 0.f, 0.f, 0.f};
    ring.template run_tiles<2>(h1s, HP, H, ln, lj, vac);
    if constexpr (!EARLY) ring1.start(theta_t + L.w1, H, cb, ln, lj);
    __syncthreads();                              // every wave is done with g2: g1 may replace it
    // ---- layer 1's (zc, zr) again on the lanes that hold v1 (the centre and radius tiles: the instruction sequence of the first run) ----
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[p][t] = v4f{0.f, 0.f, 0.f, 0.f};
    ring1.template run_tiles_abs<2, 2u>(xs + HT * XP, XP, k1r, ln, lj, acc);
    {
        float part[4][LIN_P1];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int q = 0; q < LIN_P1; ++q) part[rr][q] = 0.0f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = cb + NT * ln + t;
            const float bv = theta[L.b1 + col];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const LinUnit q = lin_relax(acc[0][t][rr] + bv, acc[1][t][rr]);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float v = vac[j][t][rr], g = v * q.lam;
                    part[rr][3 * j + 0] += g * bv;
                    part[rr][3 * j + 1] += v * (v > 0.0f ? q.bu : q.bl);
                    part[rr][3 * j + 2] += v * (v > 0.0f ? q.bl : q.bu);
                    h1s[(j * HT + 4 * lj + rr) * HP + col] = g;
                }
            }
        }
        lin_row_sums<LIN_P1>(part, &part_s[wave][0][LIN_P2], ln, lj);
    }
    __syncthreads();
    // ---- v0 = g1 W1 with W1 as stored, as adv_obs_kernel's last GEMM with two A tiles: 16-column tiles of the input dealt to the waves.
    // Columns beyond in_dim read the last column and meet c0 = r0 = 0.  A wave's tiles add up in ascending order.
    {
        float part[4][LIN_P0];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int q = 0; q < LIN_P0; ++q) part[rr][q] = 0.0f;
        const int ntile = (K1 + 15) >> 4;
        for (int tile = wave; tile < ntile; tile += WAVES) {
            const int col = 16 * tile + ln;
            const float* wp = theta + L.w1 + (size_t)(4 * lj) * K1 + (col < K1 ? col : K1 - 1);
            const float* arow = h1s + ln * HP + 4 * lj;
            v4f g[2] = {v4f{0.f, 0.f, 0.f, 0.f}, v4f{0.f, 0.f, 0.f, 0.f}};
            for (int s0 = 0; s0 < H / 16; s0 += 4) {       // four steps' loads in flight (H / 16 is a multiple of 4)
                float b[4][4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int e = 0; e < 4; ++e) b[u][e] = wp[(size_t)(16 * (s0 + u) + e) * K1];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const float4 a4 = *reinterpret_cast<const float4*>(arow + j * HT * HP + 16 * (s0 + u));
                        const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) g[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], b[u][e], g[j], 0, 0, 0);
                    }
                }
            }
            const bool in = col < K1;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int row = 4 * lj + rr;
                const float c0 = in ? xs[(HT + row) * XP + col] : 0.0f, r0 = in ? xs[(2 * HT + row) * XP + col] : 0.0f;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    part[rr][2 * j + 0] += g[j][rr] * c0;
                    part[rr][2 * j + 1] += fabsf(g[j][rr]) * r0;
                }
            }
        }
        lin_row_sums<LIN_P0>(part, &part_s[wave][0][LIN_P2 + LIN_P1], ln, lj);
    }
    __syncthreads();
    if (tid < HT && mode_s[tid] != CERT_SKIP) {
        float* out = a.bounds + (size_t)dst_s[tid] * CERT_WORDS;
        float* pout = a.parts ? a.parts + (size_t)dst_s[tid] * CERT_WORDS : nullptr;
        if (mode_s[tid] == CERT_ZERO) {
#pragma unroll
            for (int q = 0; q < CERT_WORDS; ++q) {
                out[q] = 0.0f;
                if (pout) pout[q] = 0.0f;
            }
        } else {
            float s[LIN_PARTS];
#pragma unroll
            for (int q = 0; q < LIN_PARTS; ++q) {
                s[q] = 0.0f;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) s[q] += part_s[w][tid][q];
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float b3 = theta[L.b3 + j];
                const float mc = s[6 * j + 1] + b3, mr = s[6 * j + 2];
                const float loI = __fadd_rn(mc, -mr), hiI = __fadd_rn(mc, mr);
                const float base = ((b3 + s[6 * j + 3]) + s[LIN_P2 + 3 * j]) + s[LIN_P2 + LIN_P1 + 2 * j], rad = s[LIN_P2 + LIN_P1 + 2 * j + 1];
                const float hiL = __fadd_rn(__fadd_rn(__fadd_rn(base, s[6 * j + 4]), s[LIN_P2 + 3 * j + 1]), rad);
                const float loL = __fadd_rn(__fadd_rn(__fadd_rn(base, s[6 * j + 5]), s[LIN_P2 + 3 * j + 2]), -rad);
                float lo = loL > loI ? loL : loI, hi = hiL < hiI ? hiL : hiI;
                if (lo > hi) { lo = loI; hi = hiI; }
                out[2 * j] = __fadd_rn(lo, -a.pad);
                out[2 * j + 1] = __fadd_rn(hi, a.pad);
                out[4 + j] = s[6 * j] + b3;
                if (pout) {
                    pout[2 * j] = loL; pout[2 * j + 1] = hiL;
                    pout[4 + 2 * j] = loI; pout[4 + 2 * j + 1] = hiI;
                }
            }
            out[6] = 1.0f;
            out[7] = eps_s[tid];
        }
    }
}
