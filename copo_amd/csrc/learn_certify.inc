// Part of learn_fused.hip: interval bound propagation (IBP) through the policy net of a seated bank -- for every listed row a box that
// holds the two action MEANS under every perturbation of its LiDAR block inside an L-infinity budget (copo_cert_obs_seats_f32;
// eval/certify.py, DESIGN.md section 8o).  learn_inputgrad.inc and learn_pgd.inc bound the worst case from below; this is the other side.
// ------------------------------------------------------------------------------------------------------------
// Per row r of member k's list, level = levels[level_of[group[r / n_slots]][k]] = four f32 words: eps >= 0, delta_steer,
// delta_throttle, 0 (the deltas are the fold's, copo_certify_tally; the kernel reads eps only).  With o the TRUE row:
//     lo[j] = max(o[j] - eps, 0), hi[j] = min(o[j] + eps, 1) on the columns [col_lo, col_hi), lo = hi = o[j] elsewhere
//     c0 = (lo + hi) / 2, r0 = (hi - lo) / 2
//     layer i = 1, 2:  zc = W_i c_{i-1} + b_i, zr = |W_i| r_{i-1};  l = tanh(zc - zr), u = max(tanh(zc + zr), l)   (tanh_fast is not
//                      monotone to the last ulp where it changes its formula);  c_i = (l + u) / 2, r_i = (u - l) / 2
//     heads a = 0, 1:  mc = W3[a] . c2 + b3[a], mr = |W3[a]| . r2;  lo_a = (mc - mr) - pad, hi_a = (mc + mr) + pad   (__fadd_rn each)
//     clean:           mu_a(o), the forward pass on the true row, in the same launch
//     bounds[r] = lo_0, hi_0, lo_1, hi_1, mu_0(o), mu_1(o), 1.0, eps
// A listed row whose level index or group is out of range gets eight zeros (valid = 0); rows in no list are never written.
// Launch shape, prologue (learn_seat.inc) and masking are adv_obs_kernel's: grid ceil(cap / 16) x n_members, 16-row tile, a workgroup past counts[k]
// leaves before its first barrier, the last tile is masked, modes per ROW:
//     CERT_SKIP   no row here: nothing is written
//     CERT_ZERO   level or group out of range: eight zeros
//     CERT_RUN    the row is certified
// A tile without a CERT_RUN row writes its zeros and leaves (uniform over the workgroup).  New against adv_obs_kernel: three stacked A
// tiles -- clean, centre, radius -- run against ONE weight stream (BRing::run_tiles_abs: the radius tile multiplies by fabsf of the
// fragment in registers); a layer's epilogue turns (zc, zr) into (c, r) on the lanes, as the accumulator layouts of the stacked tiles
// coincide; layer 2's output is not materialised: every lane multiplies its post-tanh accumulators by W3 / |W3| of its columns in
// ascending order, a four-level xor tree sums the sixteen lanes of a row, and the waves hand their partials over through LDS to one
// thread per row, which adds them in wave order -- a fixed order, no atomics: two launches give the same bits.  The clean and the centre
// pass run the same instruction sequence, so at eps = 0 (c0 = o exactly, a zero radius) lo_a == hi_a == mu_a(o) in bits for pad = 0.
// LDS: three input tiles [16][k1p + 4], three h1 tiles [16][H + 4], the two mean rows of W3.
// The forward body is a copy of mlp_fwd_kernel's, as adv_obs_kernel's is (see there).
// ------------------------------------------------------------------------------------------------------------
struct CertArgs {
    SeatHead h;               // levels [n_levels][4]: eps, delta_steer, delta_throttle, 0
    float* bounds;            // [n_out][8]
    float pad;
};

constexpr int CERT_SKIP = 0, CERT_ZERO = 1, CERT_RUN = 2;
constexpr int CERT_WORDS = 8, CERT_PASSES = 3;          // passes: the clean row, the centre and the radius of the box
__device__ __host__ inline size_t cert_lds_floats(int H, int k1p) { return (size_t)CERT_PASSES * HT * (H + 4 + k1p + 4) + 2 * H; }

template <int NT, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) cert_obs_kernel(CertArgs a) {
    extern __shared__ float4 cert_lds[];
    __shared__ int64_t dst_s[HT];                  // where a tile row's outputs go
    __shared__ float eps_s[HT];
    __shared__ int mode_s[HT];
    __shared__ float part_s[WAVES][HT][6];         // a wave's share of a row's head sums: clean 0 / 1, centre 0 / 1, radius 0 / 1
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
    float* h1s = reinterpret_cast<float*>(cert_lds);    // [3][HT][HP]  h1 of the true row, centre and radius behind layer 1
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
            if (mode_s[row] != CERT_SKIP) a.bounds[(size_t)dst_s[row] * CERT_WORDS + (i - row * CERT_WORDS)] = 0.0f;
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
    v4f acc[CERT_PASSES][NT];
    // ---- layer 1 on the three tiles ----
#pragma unroll
    for (int p = 0; p < CERT_PASSES; ++p)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[p][t] = v4f{0.f, 0.f, 0.f, 0.f};
    ring.template run_tiles_abs<CERT_PASSES, 4u>(xs, XP, (K1 + 15) & ~15, ln, lj, acc);
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
    float part[4][6];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int q = 0; q < 6; ++q) part[rr][q] = 0.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = cb + NT * ln + t;
        const float bv = theta[L.b2 + col];
        const float w0 = w3s[col], w1 = w3s[H + col], a0 = fabsf(w0), a1 = fabsf(w1);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const float zc = acc[1][t][rr] + bv, zr = acc[2][t][rr];
            const float l = tanh_fast(zc - zr), u = fmaxf(tanh_fast(zc + zr), l);
            const float h = tanh_fast(acc[0][t][rr] + bv), cc = 0.5f * (l + u), rd = 0.5f * (u - l);
            part[rr][0] += h * w0; part[rr][1] += h * w1;
            part[rr][2] += cc * w0; part[rr][3] += cc * w1;
            part[rr][4] += rd * a0; part[rr][5] += rd * a1;
        }
    }
    // ---- heads: the sixteen lanes of a row by an xor tree, the waves through LDS in wave order ----
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            float s = part[rr][q];
            s += __shfl_xor(s, 8);
            s += __shfl_xor(s, 4);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 1);
            if (ln == 0) part_s[wave][4 * lj + rr][q] = s;
        }
    __syncthreads();
    if (tid < HT && mode_s[tid] != CERT_SKIP) {
        float* out = a.bounds + (size_t)dst_s[tid] * CERT_WORDS;
        if (mode_s[tid] == CERT_ZERO) {
#pragma unroll
            for (int q = 0; q < CERT_WORDS; ++q) out[q] = 0.0f;
        } else {
            float s[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                s[q] = 0.0f;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) s[q] += part_s[w][tid][q];
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float b3 = theta[L.b3 + j];
                const float mc = s[2 + j] + b3, mr = s[4 + j];
                out[2 * j] = __fadd_rn(__fadd_rn(mc, -mr), -a.pad);
                out[2 * j + 1] = __fadd_rn(__fadd_rn(mc, mr), a.pad);
                out[4 + j] = s[j] + b3;
            }
            out[6] = 1.0f;
            out[7] = eps_s[tid];
        }
    }
}
