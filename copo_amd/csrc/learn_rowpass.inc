// Part of learn_fused.hip: the row-pass kernel (both layers + heads + activation gradients of 16 rows) and its
// forward-only sibling.
// ------------------------------------------------------------------------------------------------------------
// row pass: everything of an SGD step that is LOCAL TO A ROW of the minibatch -- both layer forwards, the heads
// with the loss gradients, and the activation gradients back to layer 1 -- in one kernel, one workgroup per 16 rows
// and net.  h1 / h2 / dz2 tiles stay in LDS between the phases; the weights stream from L2 straight into the MFMA
// B operands (v_mfma_f32_16x16x4_f32: lane l supplies A[l & 15][k] and B[k][l & 15] with k = l >> 4, so lane group
// l >> 4 owns one quarter of K and walks it with float4 loads).  Only the weight gradients (sums over rows)
// need the second kernel.  Replaces F1, F2, H, B2x: an SGD step is then three launches.
// ------------------------------------------------------------------------------------------------------------
typedef float v4f __attribute__((ext_vector_type(4)));

// acc[t] += A[16 x K] * W^T for the 16 output columns cb + 16 t + (l & 15); W rows are k-contiguous (forward).
// K is walked in steps of 32: lane group j = l >> 4 takes k = 32 s + 8 j + {0..7}, so the four lane groups of a row
// read one whole 128-byte line per step (every line of W is touched exactly once per workgroup).
// The weights were rewritten by the previous kernel (Adam), so the first touch of every line misses the XCD's L2:
// a ring of D steps of B operands is kept in flight (D x 8 x NT VGPRs) to cover that latency with MFMA work.
// kp = K rounded up to a multiple of 32 D; As rows hold zeros beyond K, so the over-read of W is harmless.
template <int NT, int D>
__device__ __forceinline__ void rowgemm_fwd(const float* As, int astride, const float* W, int wstride, int kp, int cb, int ln,
                                            int lj, v4f* acc) {
    const float* arow = As + ln * astride + 8 * lj;
    const float* wrow[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) wrow[t] = W + (size_t)(cb + 16 * t + ln) * wstride + 8 * lj;
    const int ns = kp >> 5;                    // multiple of D
    v4f b[D][2][NT];
#pragma unroll
    for (int u = 0; u < D; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            b[u][0][t] = *reinterpret_cast<const v4f*>(wrow[t] + 32 * u);
            b[u][1][t] = *reinterpret_cast<const v4f*>(wrow[t] + 32 * u + 4);
        }
    for (int s0 = 0; s0 < ns; s0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int s = s0 + u;
            const float4 a0 = *reinterpret_cast<const float4*>(arow + 32 * s), a1 = *reinterpret_cast<const float4*>(arow + 32 * s + 4);
            const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                // keep each quad one 128-bit register tuple: without this the optimiser splits the ring's float4
                // loads into dword loads, and the 6-bit vmcnt counter saturates long before the ring is in flight
                asm volatile("" : "+v"(b[u][0][t]), "+v"(b[u][1][t]));
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], b[u][e >> 2][t][e & 3], acc[t], 0, 0, 0);
            }
            const int sn = s + D < ns ? s + D : ns - 1;     // refill this slot (clamped: unconditional loads)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                b[u][0][t] = *reinterpret_cast<const v4f*>(wrow[t] + 32 * sn);
                b[u][1][t] = *reinterpret_cast<const v4f*>(wrow[t] + 32 * sn + 4);
            }
        }
    }
}

// acc[t] += A[16 x K] * W for output columns cb + NT (l & 15) + t; W is [K][wstride] (backward: W2 as stored).
// Tile t of a wave holds the columns {cb + NT i + t}: a lane's NT tiles are NT adjacent columns, so its B values of one
// k are one contiguous load (float4 for NT = 4) and 16 lanes read 16 NT contiguous floats.  Steps of 16 k (lane
// group j takes k = 16 s + 4 j + {0..3}); ring of D steps in flight.
typedef float v2f __attribute__((ext_vector_type(2)));
template <int N> struct ColVec;                 // N adjacent columns of one k as one load
template <> struct ColVec<1> { typedef float T; static __device__ __forceinline__ float get(const float& v, int) { return v; } };
template <> struct ColVec<2> { typedef v2f T; static __device__ __forceinline__ float get(const v2f& v, int i) { return v[i]; } };
template <> struct ColVec<4> { typedef v4f T; static __device__ __forceinline__ float get(const v4f& v, int i) { return v[i]; } };

// Ring of D steps of B operands for the [K][wstride]-layout GEMM.  `start` issues the first D steps' loads and can be
// called long before `run` (the loads depend only on the weights): the L2-missing first touch of the weights then
// overlaps whatever the workgroup does in between (input gather, the previous layer's epilogue, the heads).
template <int NT, int D, bool BF = false>       // BF: operands rounded to bfloat16 at use (the weights stay fp32 in memory)
struct BRing {
    static constexpr int VW = NT >= 4 ? 4 : NT, NV = NT / VW;     // vector width of a load, loads per k
    typedef typename ColVec<VW>::T vec_t;
    vec_t b[D][4][NV];
    const float* wcol;
    int wstride;
    __device__ __forceinline__ void start(const float* W, int wstride_, int cb, int ln, int lj) {
        wstride = wstride_;
        wcol = W + (size_t)(4 * lj) * wstride + cb + NT * ln;
#pragma unroll
        for (int u = 0; u < D; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int q = 0; q < NV; ++q) b[u][e][q] = *reinterpret_cast<const vec_t*>(wcol + (size_t)(16 * u + e) * wstride + VW * q);
    }
    // acc[t] += A[16 x k] * W for output columns cb + NT (l & 15) + t; k a multiple of 16
    // REFILL = false: the whole K range (<= 16 D) is what `start` requested -- no loads inside, so the compiler counts the
    // outstanding loads exactly (with refills and a run-time trip count it falls back to vmcnt(0) at the first use, which
    // also waits for every younger load of the OTHER rings: 2-3 us of cold misses in front of layer 1)
    // K = 32 D exactly, in two halves with static trip counts (exact load counting): half 0 consumes the D requested steps
    // and refills every slot with step u + D, half 1 consumes those.  The caller may request another ring's loads between
    // the halves: they then queue BEHIND the refills instead of in front of them.
    template <int HALF>
    __device__ __forceinline__ void run_half(const float* As, int astride, int ln, int lj, v4f* acc) {
        const float* arow = As + ln * astride + 4 * lj;
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int s = HALF * D + u;
            const float4 a4 = *reinterpret_cast<const float4*>(arow + 16 * s);
            const float av[4] = {a4.x, a4.y, a4.z, a4.w};
            if constexpr (VW > 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int q = 0; q < NV; ++q) asm volatile("" : "+v"(b[u][e][q]));
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], opnd<BF>(ColVec<VW>::get(b[u][e][t / VW], t % VW)), acc[t], 0, 0, 0);
            if constexpr (HALF == 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int q = 0; q < NV; ++q) b[u][e][q] = *reinterpret_cast<const vec_t*>(wcol + (size_t)(16 * (u + D) + e) * wstride + VW * q);
            }
        }
    }

    // Layer-1 flavour of run<false> that hands its slots over: after slot u is consumed (or skipped: k < 16 D) it is loaded
    // with step s2 + u of ANOTHER matrix in the same column layout (`wcol2`, `wstride2` of that matrix's ring).  The loads
    // are unconditional and sit at static positions, so they are counted exactly; run_half<1> consumes them later.
    __device__ __forceinline__ void run_handoff(const float* As, int astride, int k, int ln, int lj, v4f* acc,
                                                const float* wcol2, int wstride2, int s2) {
        const float* arow = As + ln * astride + 4 * lj;
        const int ns = k >> 4;
#pragma unroll
        for (int u = 0; u < D; ++u) {
            if (u < ns) {
                const float4 a4 = *reinterpret_cast<const float4*>(arow + 16 * u);
                const float av[4] = {a4.x, a4.y, a4.z, a4.w};
                if constexpr (VW > 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int q = 0; q < NV; ++q) asm volatile("" : "+v"(b[u][e][q]));
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], opnd<BF>(ColVec<VW>::get(b[u][e][t / VW], t % VW)), acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int q = 0; q < NV; ++q) b[u][e][q] = *reinterpret_cast<const vec_t*>(wcol2 + (size_t)(16 * (s2 + u) + e) * wstride2 + VW * q);
        }
    }

    // RT stacked 16-row tiles of A against the same weight rows (forward-only kernel with 16 RT rows per workgroup): every loaded
    // row feeds RT MFMAs per column tile; per row tile the instruction sequence is that of run<true>, so the results are the same bits
    template <int RT>
    __device__ __forceinline__ void run_tiles(const float* As, int astride, int k, int ln, int lj, v4f (*acc)[NT]) {
        const float* arow = As + ln * astride + 4 * lj;
        const int ns = k >> 4;
        for (int s0 = 0; s0 < ns; s0 += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int s = s0 + u;
                if (s >= ns) break;
                float av[RT][4];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const float4 a4 = *reinterpret_cast<const float4*>(arow + (size_t)rt * 16 * astride + 16 * s);
                    av[rt][0] = a4.x; av[rt][1] = a4.y; av[rt][2] = a4.z; av[rt][3] = a4.w;
                }
                if constexpr (VW > 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int q = 0; q < NV; ++q) asm volatile("" : "+v"(b[u][e][q]));
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < NT; ++t)
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
                            acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][e], opnd<BF>(ColVec<VW>::get(b[u][e][t / VW], t % VW)), acc[rt][t], 0, 0, 0);
                const int sn = s + D < ns ? s + D : ns - 1;
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int q = 0; q < NV; ++q) b[u][e][q] = *reinterpret_cast<const vec_t*>(wcol + (size_t)(16 * sn + e) * wstride + VW * q);
            }
        }
    }

    // run_tiles whose row tiles named by the bit mask ABS multiply by |W|: the B fragment a step holds feeds every row tile, the
    // masked ones through fabsf of the value in its register (interval propagation, learn_certify.inc: centre and radius of a box
    // against one weight stream).  Per unmasked row tile the instruction sequence is run_tiles', so those results are the same bits.
    template <int RT, unsigned ABS>
    __device__ __forceinline__ void run_tiles_abs(const float* As, int astride, int k, int ln, int lj, v4f (*acc)[NT]) {
        const float* arow = As + ln * astride + 4 * lj;
        const int ns = k >> 4;
        for (int s0 = 0; s0 < ns; s0 += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int s = s0 + u;
                if (s >= ns) break;
                float av[RT][4];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const float4 a4 = *reinterpret_cast<const float4*>(arow + (size_t)rt * 16 * astride + 16 * s);
                    av[rt][0] = a4.x; av[rt][1] = a4.y; av[rt][2] = a4.z; av[rt][3] = a4.w;
                }
                if constexpr (VW > 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int q = 0; q < NV; ++q) asm volatile("" : "+v"(b[u][e][q]));
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const float bv = opnd<BF>(ColVec<VW>::get(b[u][e][t / VW], t % VW));
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
                            acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][e], (ABS >> rt) & 1u ? fabsf(bv) : bv, acc[rt][t], 0, 0, 0);
                    }
                const int sn = s + D < ns ? s + D : ns - 1;
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int q = 0; q < NV; ++q) b[u][e][q] = *reinterpret_cast<const vec_t*>(wcol + (size_t)(16 * sn + e) * wstride + VW * q);
            }
        }
    }

    template <bool REFILL = true>
    __device__ __forceinline__ void run(const float* As, int astride, int k, int ln, int lj, v4f* acc) {
        const float* arow = As + ln * astride + 4 * lj;
        const int ns = k >> 4;
        if constexpr (!REFILL) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                if (u >= ns) break;
                const float4 a4 = *reinterpret_cast<const float4*>(arow + 16 * u);
                const float av[4] = {a4.x, a4.y, a4.z, a4.w};
                if constexpr (VW > 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int q = 0; q < NV; ++q) asm volatile("" : "+v"(b[u][e][q]));
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], opnd<BF>(ColVec<VW>::get(b[u][e][t / VW], t % VW)), acc[t], 0, 0, 0);
            }
            return;
        }
        for (int s0 = 0; s0 < ns; s0 += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int s = s0 + u;
                if (s >= ns) break;          // k need not fill the last ring turn (layer 1: 96 of 128 for a 92-wide input)
                const float4 a4 = *reinterpret_cast<const float4*>(arow + 16 * s);
                const float av[4] = {a4.x, a4.y, a4.z, a4.w};
                if constexpr (VW > 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int q = 0; q < NV; ++q) asm volatile("" : "+v"(b[u][e][q]));      // one register tuple per load (see rowgemm_fwd)
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], opnd<BF>(ColVec<VW>::get(b[u][e][t / VW], t % VW)), acc[t], 0, 0, 0);
                const int sn = s + D < ns ? s + D : ns - 1;
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int q = 0; q < NV; ++q) b[u][e][q] = *reinterpret_cast<const vec_t*>(wcol + (size_t)(16 * sn + e) * wstride + VW * q);
            }
        }
    }
};

template <int NT, int D>
__device__ __forceinline__ void rowgemm_bwd(const float* As, int astride, const float* W, int wstride, int k, int cb, int ln,
                                            int lj, v4f* acc) {
    BRing<NT, D> r;
    r.start(W, wstride, cb, ln, lj);
    r.run(As, astride, k, ln, lj, acc);
}

constexpr int RP_D1 = 4;      // prefetch ring depth of the layer-1 GEMM (its K is padded to 32 * RP_D1)
__device__ __host__ inline int rowpass_k1p(int in_dim) { return (in_dim + 32 * RP_D1 - 1) / (32 * RP_D1) * (32 * RP_D1); }
__device__ __host__ inline size_t rowpass_lds_floats(int H, int k1p) {
    return (size_t)HT * (k1p + 4) + (size_t)3 * HT * (H + 4) + 4 * H + HT * 4 + HT * 8;
}

#define RP_STAMP(i) do { if ((a.dbg & 256) && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) g_rp_stamps[i] = wall_clock64(); } while (0)

// hidden = 16 * NT * WAVES: every wave owns NT column tiles of 16.  Two waves per SIMD (WAVES = 8) overlap one
// wave's epilogue / load stalls with the other's MFMAs; the MFMA work per SIMD is the same.
// TW: a.theta_t holds W1 / W2 transposed ([in][out]), so the forward B operands are read like the backward ones --
// 16 lanes per 64 NT contiguous bytes -- instead of one row per lane (the strided pattern costs ~2x in the TA).
// HO (hand-over, chosen by the launcher when every net's input is at most 16 DB columns wide and layer 2 is two ring turns):
// layer 1 runs without loads of its own and refills its slots with the second half of W2^T (BRing::run_handoff).
// RT: minibatch rows per workgroup, 16 or 8.  The MFMA tile is 16 rows tall either way (LDS tiles keep 16 rows; rows >= RT hold
// don't-care values that only reach accumulator rows nobody stores) -- 8-row tiles double the workgroup count where 16-row
// tiles leave half of the compute units without one (512 rows x 4 nets = 128 workgroups on 256 CUs): the wasted MFMA rows are
// free on a latency-bound kernel, and everything that is proportional to the rows (input gather, heads, dz2, epilogues) halves.
template <int NT, int WAVES, bool TW, bool BF = false, bool HO = false, int RT = HT>
__global__ void __launch_bounds__(64 * WAVES) rowpass_kernel(FusedArgs a) {
    static_assert(TW || !BF, "bfloat16 operands go through the transposed-mirror path");
    static_assert(RT == 8 || RT == HT, "row tiles of 8 or 16");
    extern __shared__ float4 rowpass_lds[];
    constexpr int H = 16 * NT * WAVES, HP = H + 4, TH = 64 * WAVES, TPR = TH / RT;      // TPR: threads per row (heads)
    static_assert(TPR <= 64, "a row's head threads must sit in one wave (shuffle reduction)");
    constexpr int DF = NT >= 8 ? 2 : 4, DF2 = H / 32 < DF ? H / 32 : DF;                // prefetch ring depths
    constexpr int DB = NT >= 8 ? 4 : (H / 16 >= 8 ? 8 : H / 16);
    static_assert(H % (32 * DF2) == 0 && (H / 16) % DB == 0, "ring depths must divide the step counts");
    const copo_ppo_cfg& c = a.c;
    int g, tile;          // all row tiles of a net on the same XCDs: its weights are read through one or two L2s
    xcd_tile(tile, g);
    const int m0 = tile * RT;
    const copo_net_layout L = net_of(a, g);
    const float* theta = theta_of(a, g);
    const int mode = mode_of(a, g);
    const bool policy = is_policy(a, g);
    const int K1 = L.in_dim, OD = L.out_dim, K1P = rowpass_k1p(K1), XP = K1P + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 15, lj = lane >> 4, cb = wave * (16 * NT);
    float* xs = reinterpret_cast<float*>(rowpass_lds);      // [HT][XP]   gathered input rows, zero beyond K1
    float* h1s = xs + HT * XP;                               // [HT][HP]
    float* h2s = h1s + HT * HP;                              // [HT][HP]
    float* dzs = h2s + HT * HP;                              // [HT][HP]   dz2
    float* w3s = dzs + HT * HP;                              // [4][H]
    float* douts = w3s + 4 * H;                              // [HT][4]
    float* sts = douts + HT * 4;                             // [HT][8]    per-row loss statistics
    // the first kernel of an SGD step advances the Adam step counter (its only reader is the fold at the end)
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) first_kernel_duties(a);
    if ((a.dbg & 2048) && threadIdx.x == 0) g_wg_times[0][(blockIdx.x + blockIdx.y * gridDim.x) & 1023][0] = wall_clock64();
    RP_STAMP(0);
    // TW: the first ring of layer-1 weights is requested before anything else
    constexpr bool EARLY = NT <= 2;          // two rings in flight fit the register file only for narrow waves
    // EARLY: the layer-2 ring is requested right after the layer-1 ring, so both cold misses (the weights were rewritten by
    // the previous step's Adam) overlap the prologue; layer 1 then runs without any load in its loop (exact load counting)
    constexpr bool HANDOFF = HO;
    static_assert(!HO || (TW && EARLY && H / 16 == 2 * DB), "hand-over: two ring turns of layer 2, narrow waves");
    // bfloat16-operand mode: the transposed mirror already holds rounded weights (its writers round), so only the ring that
    // reads W2 as stored (the fp32 master) rounds at use
    BRing<NT, DB, false> ring1, ring2;
    BRing<NT, DB, BF> ring3;
    if (TW) ring1.start(a.theta_t + L.w1, H, cb, ln, lj);
    if (TW && EARLY) ring2.start(a.theta_t + L.w2, H, cb, ln, lj);
    // biases of this lane's columns: requested now (the parameters were rewritten by the previous step's Adam, so the
    // first touch misses L2) instead of after each layer's GEMM, where the miss sat on the critical path
    float b1v[NT], b2v[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = TW ? cb + NT * ln + t : cb + 16 * t + ln;
        b1v[t] = opnd<BF>(theta[L.b1 + col]);
        b2v[t] = opnd<BF>(theta[L.b2 + col]);
    }
    float b3v[4];        // head biases: same reason (their load sat between the head dot products and the loss terms)
#pragma unroll
    for (int j = 0; j < 4; ++j) b3v[j] = opnd<BF>(theta[L.b3 + (j < OD ? j : 0)]);
    const int64_t kb = kb_of(a, g);
    // head bookkeeping: TPR threads per row; the dependent loads (k -> row index -> pack row) are issued here and
    // consumed after both layers
    const int r = tid / TPR, part = tid % TPR, m = m0 + r;
    const bool rok = m < c.mb;
    float wgt = 0.0f;
    RowIn ri;
    if (part == 0) {
        const int64_t prow = src_row(a, kb, rok ? m : 0);
        wgt = rok ? a.w[kb * c.mb + m] / a.denom[kb] : 0.0f;
        ri = load_row_in(a, g, mode, policy, a.pack_src + (size_t)prow * c.pack_width);
    }
    {   // input tile: rows gathered through the minibatch table, float4 per thread, zeros beyond K1 / mb
        const float* src = src_of(a, g);
        if ((K1 & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const int qn = K1P >> 2;
            for (int i = tid; i < RT * qn; i += TH) {
                const int row = i / qn, k = (i - row * qn) * 4;
                const bool ok = (m0 + row < c.mb) && (k < K1);
                const int64_t ridx = src_row(a, kb, m0 + row < c.mb ? m0 + row : 0);
                float4 v = *reinterpret_cast<const float4*>(src + (size_t)ridx * K1 + (k < K1 ? k : 0));
                if (BF) v = make_float4(bf16r(v.x), bf16r(v.y), bf16r(v.z), bf16r(v.w));
                *reinterpret_cast<float4*>(xs + row * XP + k) = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {      // rows that are not 16-byte aligned (e.g. the 91-dim observation): element-wise gather
            for (int i = tid; i < RT * K1P; i += TH) {
                const int row = i / K1P, k = i - row * K1P;
                const bool ok = (m0 + row < c.mb) && (k < K1);
                const int64_t ridx = src_row(a, kb, m0 + row < c.mb ? m0 + row : 0);
                const float v = opnd<BF>(src[(size_t)ridx * K1 + (k < K1 ? k : 0)]);
                xs[row * XP + k] = ok ? v : 0.0f;
            }
        }
        for (int i = tid; i < OD * H; i += TH) w3s[i] = opnd<BF>(theta[L.w3 + i]);
    }
    __syncthreads();
    RP_STAMP(1);
    v4f acc[NT];
    // ---- layer 1 ----
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
    if (TW) {
        const int k1 = (K1 + 15) & ~15;
        // HANDOFF: the layer-1 input (<= 16 DB columns, checked by the launcher) was requested whole by `start`: no load of W1
        // in the loop, and every slot is handed over to the SECOND half of W2^T as soon as layer 1 is done with it -- those
        // loads then have layer 1 and the first half of layer 2 to arrive
        if constexpr (HANDOFF) ring1.run_handoff(xs, XP, k1, ln, lj, acc, ring2.wcol, ring2.wstride, DB);
        else if (EARLY && k1 <= 16 * DB) ring1.template run<false>(xs, XP, k1, ln, lj, acc);      // (uniform)
        else ring1.template run<true>(xs, XP, k1, ln, lj, acc);
    } else if (!(a.dbg & 1)) rowgemm_fwd<NT, DF>(xs, XP, theta + L.w1, K1, K1P, cb, ln, lj, acc);
    {
        float* h1g = a.ws + ws_h1(a, g);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = TW ? cb + NT * ln + t : cb + 16 * t + ln;      // tile -> column map of the GEMM flavour used
            const float bv = b1v[t];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = 4 * lj + rr;
                const float y = opnd<BF>(tanh_fast(opnd<BF>(acc[t][rr] + bv)));    // BF: linear output and tanh output are bfloat16 tensors
                h1s[i * HP + col] = y;
                if (i < RT && m0 + i < c.mb) store_next(&h1g[(size_t)(m0 + i) * H + col], y);
            }
        }
    }
    __syncthreads();
    RP_STAMP(2);
    // ---- layer 2 ----
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
    if (TW) {
        // W2 as stored (ring3) feeds the activation-gradient GEMM below; it is requested where its loads do not sit in
        // front of layer 2's own refills in the (in-order) load queue
        if constexpr (!EARLY) {
            ring2.start(a.theta_t + L.w2, H, cb, ln, lj);
            ring2.run(h1s, HP, H, ln, lj, acc);
        } else if constexpr (H / 16 == 2 * DB) {
            if constexpr (HANDOFF) {      // the second half of W2^T is in ring1's slots (run_handoff)
                ring2.template run<false>(h1s, HP, 16 * DB, ln, lj, acc);
                ring3.start(theta + L.w2, H, cb, ln, lj);
                ring1.template run_half<1>(h1s, HP, ln, lj, acc);
            } else {
                ring2.template run_half<0>(h1s, HP, ln, lj, acc);
                ring3.start(theta + L.w2, H, cb, ln, lj);
                ring2.template run_half<1>(h1s, HP, ln, lj, acc);
            }
        } else {
            static_assert(EARLY ? (H / 16 == DB || H / 16 == 2 * DB) : true, "layer-2 steps: one or two ring turns");
            ring3.start(theta + L.w2, H, cb, ln, lj);
            ring2.template run<false>(h1s, HP, H, ln, lj, acc);
        }
    } else if (!(a.dbg & 2)) rowgemm_fwd<NT, DF2>(h1s, HP, theta + L.w2, H, H, cb, ln, lj, acc);
    {
        float* h2g = a.ws + ws_h2(a, g);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = TW ? cb + NT * ln + t : cb + 16 * t + ln;
            const float bv = b2v[t];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = 4 * lj + rr;
                const float y = opnd<BF>(tanh_fast(opnd<BF>(acc[t][rr] + bv)));
                h2s[i * HP + col] = y;
                if (i < RT && m0 + i < c.mb) store_next(&h2g[(size_t)(m0 + i) * H + col], y);
            }
        }
    }
    __syncthreads();
    RP_STAMP(3);
    // ---- heads, loss terms, d(loss)/d(outputs) ----
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = part; i < H; i += TPR) {
        const float h = h2s[r * HP + i];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < OD) out[j] += h * w3s[j * H + i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int o = 1; o < TPR; o <<= 1) out[j] += __shfl_xor(out[j], o);
    }
    if (part == 0) {
        float st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        float dout[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = opnd<BF>(out[j] + b3v[j]);
        if (rok && !(a.dbg & 8)) head_row_terms(a, g, mode, policy, ri, wgt, out, dout, st);
        if (BF) {           // the loss is fp32; its gradient enters the bfloat16 graph rounded
#pragma unroll
            for (int j = 0; j < 4; ++j) dout[j] = bf16r(dout[j]);
        }
        *reinterpret_cast<float4*>(douts + r * 4) = make_float4(dout[0], dout[1], dout[2], dout[3]);
        if (rok) *reinterpret_cast<float4*>(a.ws + ws_dout(a, g) + (size_t)m * 4) = make_float4(dout[0], dout[1], dout[2], dout[3]);
        *reinterpret_cast<float4*>(sts + r * 8) = make_float4(st[0], st[1], st[2], st[3]);
        *reinterpret_cast<float4*>(sts + r * 8 + 4) = make_float4(st[4], st[5], st[6], st[7]);
    }
    __syncthreads();
    RP_STAMP(4);
    if (tid < 8) {       // per-tile partial of the statistics, rows in a fixed order
        float sv = 0.0f;
#pragma unroll
        for (int rr = 0; rr < RT; ++rr) sv += sts[rr * 8 + tid];
        a.ws[ws_stats_at(a, g * a.stat_tiles + tile) + tid] = sv;
    }
    // ---- dz2 = (dout W3) * (1 - h2^2) ----
    {
        float* dz2g = a.ws + ws_dz2(a, g);
        const int nr = (c.mb - m0 < RT) ? c.mb - m0 : RT;
        for (int i = tid; i < H; i += TH) {
            float wc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) wc[j] = (j < OD) ? w3s[j * H + i] : 0.0f;
#pragma unroll
            for (int rr = 0; rr < RT; ++rr) {
                const float4 d = *reinterpret_cast<const float4*>(douts + rr * 4);
                const float h = h2s[rr * HP + i];
                const float v = opnd<BF>(opnd<BF>((d.x * wc[0] + d.y * wc[1]) + (d.z * wc[2] + d.w * wc[3])) * (1.0f - h * h));
                dzs[rr * HP + i] = v;
                if (rr < nr) store_next(&dz2g[(size_t)(m0 + rr) * H + i], v);
            }
        }
    }
    __syncthreads();
    RP_STAMP(5);
    // ---- dz1 = (dz2 W2) * (1 - h1^2) ----
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
    if (TW) {
        if (!EARLY) ring3.start(theta + L.w2, H, cb, ln, lj);
        ring3.run(dzs, HP, H, ln, lj, acc);
    }
    else if (!(a.dbg & 4)) rowgemm_bwd<NT, DB>(dzs, HP, theta + L.w2, H, H, cb, ln, lj, acc);
    {
        float* dz1g = a.ws + ws_dz1(a, g);
        // tile t of rowgemm_bwd holds the columns cb + NT * ln + t: a lane stores NT adjacent columns per row
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int i = 4 * lj + rr;
            if (i < RT && m0 + i < c.mb) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int col = cb + NT * ln + t;
                    const float h = h1s[i * HP + col];
                    store_next(&dz1g[(size_t)(m0 + i) * H + col], opnd<BF>(opnd<BF>(acc[t][rr]) * (1.0f - h * h)));
                }
            }
        }
    }
    RP_STAMP(9);
    // EXPERIMENT (profiling builds): the hand-over a merged row pass + weight-gradient kernel would need here.
    //   4096: release fence by every workgroup + arrive + wait for all + acquire fence      8192: the fence alone
    if (a.dbg & (4096 | 8192)) {
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence();
            if (a.dbg & 4096) {
                const unsigned int nwg = gridDim.x * gridDim.y;
                const unsigned int t = atomicAdd(&g_rp_bar, 1u);
                const unsigned int target = (t / nwg + 1u) * nwg;
                while ((int)(__hip_atomic_load(&g_rp_bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) __builtin_amdgcn_s_sleep(2);
                __threadfence();
            }
        }
        __syncthreads();
    }
    if ((a.dbg & 2048) && threadIdx.x == 0) g_wg_times[0][(blockIdx.x + blockIdx.y * gridDim.x) & 1023][1] = wall_clock64();
}

// ------------------------------------------------------------------------------------------------------------
// row pass on 8-row tiles with v_mfma_f32_4x4x1_16B_f32 (the production shape: 512 rows x 4 nets = 256 workgroups, one per
// compute unit).  The 16 x 16 x 4 tile of rowpass_kernel is 16 rows tall, so with 8 rows per workgroup half of every MFMA
// is wasted; the 4 x 4 x 1 instruction with its A operand broadcast from one block to all sixteen (cbsz = 4, abid = b) is a
// 4-row x 64-column outer product: lane = output column, four rows per instruction, two instructions per k for the eight
// rows -- no wasted rows, half the MFMA cycles per workgroup (scripts/micro/mfma4x4_probe.hip pins the operand layout).
// Work split: wave w owns the 64 columns of group w % (H / 64) and one of R8_KS parts of every K range (w / (H / 64)); the
// parts' accumulators meet in LDS after each GEMM (each wave finishes 8 / R8_KS of the eight rows).  R8_KS waves per SIMD,
// because a lane gets ONE k of its column per load (every matrix is read as [k][column]: W1^T / W2^T from the transposed
// mirror, W2 as stored for the activation gradients; one coalesced 256-byte row per k and wave) and the 6-bit load counter
// caps a wave at 63 loads in flight: four waves x 32 k = 128 k per SIMD = ~1000 cycles of MFMA work cover an L2 round trip
// (two waves per SIMD: SGD step 33.0 us, see profiles/).
// ONE stream of B rows: the rows a wave needs from the three matrices form one sequence in the order of use, walked by one
// ring of R8_D registers -- the prefetch runs ahead across the layer boundaries, so the cold first touch of the next layer's
// weights (rewritten by the previous step's Adam) happens under the current layer's MFMAs.
// The A operand of lanes 0..7 is row (lane & 7) of the LDS tile, four k per ds_read_b128.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum_f32_to_lane63(float v) {
#define COPO_FSUM_STEP(ctrl, rmask) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rmask, 0xf, false));
    COPO_FSUM_STEP(0x111, 0xf)   // row_shr:1
    COPO_FSUM_STEP(0x112, 0xf)   // row_shr:2
    COPO_FSUM_STEP(0x114, 0xf)   // row_shr:4
    COPO_FSUM_STEP(0x118, 0xf)   // row_shr:8
    COPO_FSUM_STEP(0x142, 0xa)   // row_bcast:15 -> rows 1, 3
    COPO_FSUM_STEP(0x143, 0xc)   // row_bcast:31 -> rows 2, 3
#undef COPO_FSUM_STEP
    return v;
}

constexpr int R8 = 8;          // rows per workgroup
constexpr int R8_D = 32;       // k-steps of B operands in flight per wave
constexpr int R8_KS = 4;       // waves that share a K range (= waves per SIMD): 4 x 32 k in flight per SIMD
__device__ __host__ inline int rowpass8_k1p(int in_dim) { return (in_dim + R8_KS * R8_D - 1) / (R8_KS * R8_D) * (R8_KS * R8_D); }      // every K part: whole ring turns
__device__ __host__ inline size_t rowpass8_lds_floats(int H, int k1p) {
    return (size_t)R8 * (k1p + 4) + (size_t)3 * R8 * (H + 4) + 4 * H + R8 * 4 + R8 * 8 + (size_t)R8_KS * R8 * H;
}

// the B-operand stream of one wave: segment 0 = rows [k0a, k0a + na) of matrix A (rows beyond its last valid one read as zero: the A
// operand holds zeros there), then nb rows from kb of matrices B and C.
// Addressing: raw buffer loads.  The row number is uniform, so a global load needs a 64-bit scalar address per row -- six scalar
// instructions per k (add, clamp, sign-extend, shift, add, add-with-carry; 1 036 per wave of the round-4 kernel, MORE than its vector
// instructions), and a SIMD issues one scalar instruction per four cycles: 4 waves x 6 = 96 cycles per k against 64 cycles of MFMA.
// With a buffer descriptor per matrix the row goes into the 12-bit immediate (G rows per vector offset, one v_add per G loads), the
// range check of the descriptor replaces the clamp, and what is left on the scalar unit is the choice of the descriptor per ring turn.
template <int HS>           // row length of all three matrices (floats)
struct Stream8 {
    static constexpr int RB = HS * 4;                                           // row bytes
    static constexpr int G = (4096 / RB) < R8_D ? (4096 / RB) : R8_D;            // rows per vector offset: immediates up to 4095
    static_assert(G >= 1 && R8_D % G == 0, "row groups tile the ring");
    float b[R8_D];
    __amdgpu_buffer_rsrc_t ra, rb, rc;      // segment 0 (valid rows only: beyond them a load returns 0), segments 1, 2
    int col4, seg0, seg1, ka0, kb0, q;      // col4: the lane's column, bytes; q: rows consumed so far; seg0 / seg1: ends of segments 0 / 1
    // the R8_D rows from stream position qb on (qb a multiple of R8_D; segments are whole ring turns, so a turn never
    // straddles two matrices): descriptor and first row, uniform per turn
    __device__ __forceinline__ void turn(int qb, int total, __amdgpu_buffer_rsrc_t& r, int& k) const {
        if (qb >= total) qb = total - R8_D;          // past the end of the stream: re-read the last turn (never consumed)
        if (qb < seg0) { r = ra; k = ka0 + qb; }
        else if (qb < seg1) { r = rb; k = kb0 + (qb - seg0); }
        else { r = rc; k = kb0 + (qb - seg1); }
    }
    // vector offsets of a turn's row groups (opaque to the optimiser: it would otherwise fold column | row into 32 separate registers
    // instead of one register per group + the instruction's immediate)
    struct Turn { int vg[R8_D / G]; };
    __device__ __forceinline__ Turn offsets(int k) const {
        Turn t;
#pragma unroll
        for (int g = 0; g < R8_D / G; ++g) {
            t.vg[g] = col4 + (k + g * G) * RB;
            asm volatile("" : "+v"(t.vg[g]));
        }
        return t;
    }
    __device__ __forceinline__ float row(__amdgpu_buffer_rsrc_t r, const Turn& t, int u) const {      // row u of the turn
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, t.vg[u / G] + (u % G) * RB, 0, 0));
    }
    __device__ __forceinline__ void start(const float* wa_, const float* wb_, const float* wc_, int col_, int ka0_, int na,
                                          int ka_valid, int kb0_, int nb, int total) {
        ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wa_), 0, ka_valid * RB, 0x00020000);
        rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wb_), 0, HS * RB, 0x00020000);
        rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wc_), 0, HS * RB, 0x00020000);
        col4 = col_ * 4;
        seg0 = na; seg1 = na + nb; ka0 = ka0_; kb0 = kb0_;
        q = 0;
        __amdgpu_buffer_rsrc_t r; int k;
        turn(0, total, r, k);
        const Turn t = offsets(k);
#pragma unroll
        for (int u = 0; u < R8_D; ++u) b[u] = row(r, t, u);
    }
    // c0 / c1 += A[rows 0..3 / 4..7][ka + i] * (next n rows of the stream), n a multiple of R8_D; `total`: rows of the whole stream
    // BF: rows of segment 2 (W2 as stored, the fp32 master) are rounded to bfloat16 at use; the mirror's rows already are
    template <bool BF = false>
    __device__ __forceinline__ void run(const float* As, int astride, int ka, int n, int total, int lane, v4f& c0, v4f& c1) {
        const float* arow = As + (lane & 7) * astride + ka;
        for (int s0 = 0; s0 < n; s0 += R8_D) {
            __amdgpu_buffer_rsrc_t r; int k;
            turn(q + s0 + R8_D, total, r, k);
            const Turn t = offsets(k);
            const bool rnd = BF && q + s0 >= seg1;          // (uniform per turn)
#pragma unroll
            for (int u4 = 0; u4 < R8_D; u4 += 4) {
                const float4 a4 = *reinterpret_cast<const float4*>(arow + s0 + u4);
                const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int u = u4 + e;
                    const float bv = rnd ? bf16r(b[u]) : b[u];
                    c0 = __builtin_amdgcn_mfma_f32_4x4x1f32(av[e], bv, c0, 4, 0, 0);
                    c1 = __builtin_amdgcn_mfma_f32_4x4x1f32(av[e], bv, c1, 4, 1, 0);
                    b[u] = row(r, t, u);       // refill: unconditional, counted exactly
                }
            }
        }
        q += n;
    }
};

template <int CG, bool BF = false>          // column groups of 64: H = 64 CG, R8_KS CG waves; BF: bfloat16-operand mode (as rowpass_kernel)
__global__ void __launch_bounds__(64 * R8_KS * CG) rowpass8_kernel(FusedArgs a) {
    extern __shared__ float4 rowpass_lds[];
    constexpr int KS = R8_KS, RW = R8 / KS;                  // rows a wave finishes after the K parts met
    constexpr int H = 64 * CG, HP = H + 4, TH = 64 * KS * CG, TPR = 64;      // heads: the first 8 waves' worth of threads, one wave per row
    static_assert(TH >= R8 * TPR && R8 % KS == 0, "eight head waves; the K parts share the rows evenly");
    const copo_ppo_cfg& c = a.c;
    int g, tile;
    xcd_tile(tile, g);
    const int m0 = tile * R8;
    const copo_net_layout L = net_of(a, g);
    const float* theta = theta_of(a, g);
    const int mode = mode_of(a, g);
    const bool policy = is_policy(a, g);
    const int K1 = L.in_dim, OD = L.out_dim, K1P = rowpass8_k1p(K1), XP = K1P + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (scalar: the stream's row numbers stay on the SALU)
    const int kh = wave / CG, col = (wave % CG) * 64 + lane;
    float* xs = reinterpret_cast<float*>(rowpass_lds);      // [8][XP]   gathered input rows, zero beyond K1
    float* h1s = xs + R8 * XP;                               // [8][HP]
    float* h2s = h1s + R8 * HP;                              // [8][HP]
    float* dzs = h2s + R8 * HP;                              // [8][HP]   dz2
    float* w3s = dzs + R8 * HP;                              // [4][H]
    float* douts = w3s + 4 * H;                              // [8][4]
    float* sts = douts + R8 * 4;                             // [8][8]
    float* xch = sts + R8 * 8;                               // [KS][8][H] every K part's partial sums of the eight rows
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) first_kernel_duties(a);
    if ((a.dbg & 2048) && threadIdx.x == 0) g_wg_times[0][(blockIdx.x + blockIdx.y * gridDim.x) & 1023][0] = wall_clock64();
    RP_STAMP(0);
    Stream8<H> st8;
    const int total = K1P / KS + 2 * (H / KS);               // rows of this wave's stream: its part of each K range
    st8.start(a.theta_t + L.w1, a.theta_t + L.w2, theta + L.w2, col, kh * (K1P / KS), K1P / KS, K1, kh * (H / KS), H / KS, total);
    const float b1v = opnd<BF>(theta[L.b1 + col]), b2v = opnd<BF>(theta[L.b2 + col]);
    float b3v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b3v[j] = opnd<BF>(theta[L.b3 + (j < OD ? j : 0)]);
    const int64_t kb = kb_of(a, g);
    const int r = tid / TPR, part = tid % TPR, m = m0 + r;        // (threads beyond the eight head waves: r >= 8, no head work)
    const bool rok = r < R8 && m < c.mb;
    float wgt = 0.0f;
    RowIn ri;
    if (part >= 62 && r < R8) {      // (lane 62 too: the policy's two action dimensions are evaluated side by side on lanes 62 / 63)
        const int64_t prow = src_row(a, kb, rok ? m : 0);
        wgt = rok ? a.w[kb * c.mb + m] / a.denom[kb] : 0.0f;
        ri = load_row_in(a, g, mode, policy, a.pack_src + (size_t)prow * c.pack_width);
    }
    {
        const float* src = src_of(a, g);
        if ((K1 & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const int qn = K1P >> 2;
            for (int i = tid; i < R8 * qn; i += TH) {
                const int row = i / qn, k = (i - row * qn) * 4;
                const bool ok = (m0 + row < c.mb) && (k < K1);
                const int64_t ridx = src_row(a, kb, m0 + row < c.mb ? m0 + row : 0);
                float4 v = *reinterpret_cast<const float4*>(src + (size_t)ridx * K1 + (k < K1 ? k : 0));
                if (BF) v = make_float4(bf16r(v.x), bf16r(v.y), bf16r(v.z), bf16r(v.w));
                *reinterpret_cast<float4*>(xs + row * XP + k) = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
            for (int i = tid; i < R8 * K1P; i += TH) {
                const int row = i / K1P, k = i - row * K1P;
                const bool ok = (m0 + row < c.mb) && (k < K1);
                const int64_t ridx = src_row(a, kb, m0 + row < c.mb ? m0 + row : 0);
                const float v = opnd<BF>(src[(size_t)ridx * K1 + (k < K1 ? k : 0)]);
                xs[row * XP + k] = ok ? v : 0.0f;
            }
        }
        for (int i = tid; i < OD * H; i += TH) w3s[i] = opnd<BF>(theta[L.w3 + i]);
    }
    __syncthreads();
    RP_STAMP(1);
    // every K part publishes its partial sums of the eight rows; this wave then finishes rows RW kh .. RW kh + RW - 1 of its
    // columns, adding the parts in a fixed order
    auto meet = [&](const v4f& c0, const v4f& c1, float* z) {
        float* mine = xch + (size_t)kh * R8 * H + col;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mine[i * H] = c0[i];
            mine[(4 + i) * H] = c1[i];
        }
        __syncthreads();
#pragma unroll
        for (int ii = 0; ii < RW; ++ii) {
            const float* src = xch + (size_t)(RW * kh + ii) * H + col;
            float sum = src[0];
#pragma unroll
            for (int p = 1; p < KS; ++p) sum += src[(size_t)p * R8 * H];
            z[ii] = sum;
        }
    };
    v4f c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
    // ---- layer 1 ----
    st8.template run<BF>(xs, XP, kh * (K1P / KS), K1P / KS, total, lane, c0, c1);
    {
        float z[RW];
        meet(c0, c1, z);
        float* h1g = a.ws + ws_h1(a, g);
#pragma unroll
        for (int ii = 0; ii < RW; ++ii) {
            const int i = RW * kh + ii;
            const float y = opnd<BF>(tanh_fast(opnd<BF>(z[ii] + b1v)));
            h1s[i * HP + col] = y;
            if (m0 + i < c.mb) store_next(&h1g[(size_t)(m0 + i) * H + col], y);
        }
    }
    __syncthreads();
    RP_STAMP(2);
    // ---- layer 2 ----
    c0 = v4f{0.f, 0.f, 0.f, 0.f}; c1 = v4f{0.f, 0.f, 0.f, 0.f};
    st8.template run<BF>(h1s, HP, kh * (H / KS), H / KS, total, lane, c0, c1);
    {
        float z[RW];
        meet(c0, c1, z);
        float* h2g = a.ws + ws_h2(a, g);
#pragma unroll
        for (int ii = 0; ii < RW; ++ii) {
            const int i = RW * kh + ii;
            const float y = opnd<BF>(tanh_fast(opnd<BF>(z[ii] + b2v)));
            h2s[i * HP + col] = y;
            if (m0 + i < c.mb) store_next(&h2g[(size_t)(m0 + i) * H + col], y);
        }
    }
    __syncthreads();
    RP_STAMP(3);
    // ---- heads, loss terms, d(loss)/d(outputs) ----
    if (r < R8) {        // (wave-uniform: a wave per row)
        float out[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = part; i < H; i += TPR) {
            const float h = h2s[r * HP + i];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < OD) out[j] += h * w3s[j * H + i];
        }
        // sums over the row's wave on the DPP network (the total lands in lane 63, which owns the row's head terms): an
        // xor-shuffle ladder is 24 ds_bpermute round trips here
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = wave_sum_f32_to_lane63(out[j]);
        if (policy && mode == COPO_HEAD_PPO && OD == 4) {
            // PPO policy head (algo_copo.py:311-424): the per-dimension chains (exp, two or three IEEE divisions each) of the two action
            // dimensions run on lanes 62 / 63 side by side instead of one after the other on lane 63 -- that single-lane chain was
            // ~1 us of every SGD step (the policy net's workgroups end the launch).  Every float operation and every sum order is that
            // of head_row_terms (0 + x == x for the accumulators it starts at zero), so the results are the same bits.
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = opnd<BF>(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(out[j]), 63)) + b3v[j]);      // (uniform)
            if (part >= 62) {
                const int j = part - 62;
                auto other = [](float v) {      // the partner lane's value: quad_perm [1, 0, 3, 2]
                    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));
                };
                float dmu_w = 0.0f, dls_w = 0.0f, st0 = 0.0f, st1 = 0.0f, st3 = 0.0f, st4 = 0.0f, st7 = 0.0f;
                const bool live = rok && !(a.dbg & 8);
                {
                    const copo_ppo_cfg& cc = a.c;
                    const float mu = j == 0 ? o[0] : o[1], ls = j == 0 ? o[2] : o[3];
                    const float sig = expf(ls);
                    const float z = ((j == 0 ? ri.act0 : ri.act1) - mu) / sig;
                    const float t = -0.5f * z * z - ls - 0.5f * kLog2Pi;
                    const float e = ls + 0.5f + 0.5f * kLog2Pi;
                    const float t_o = other(t), e_o = other(e);
                    const float logp = (0.0f + (j == 0 ? t : t_o)) + (j == 0 ? t_o : t);
                    const float ent = (0.0f + (j == 0 ? e : e_o)) + (j == 0 ? e_o : e);
                    const float adv = ri.adv;
                    const float ratio = expf(logp - ri.logp);
                    const float s1 = adv * ratio;
                    const float rc = fminf(fmaxf(ratio, 1.0f - cc.clip_param), 1.0f + cc.clip_param);
                    const float s2 = adv * rc;
                    const float surr = fminf(s1, s2);
                    const bool inside = (ratio >= 1.0f - cc.clip_param) && (ratio <= 1.0f + cc.clip_param);
                    const float dsurr_dratio = (inside || s1 < s2) ? adv : 0.0f;
                    const float dlogp = -dsurr_dratio * ratio;
                    float dmu = 0.0f, dls = 0.0f, kl = 0.0f;
                    if (cc.use_kl) {
                        const float mup = j == 0 ? ri.dist0 : ri.dist1, lsp = j == 0 ? ri.dist2 : ri.dist3;
                        const float sp = expf(lsp), dm = mup - mu;
                        const float q = (sp * sp + dm * dm) / (sig * sig);
                        const float k = ls - lsp + 0.5f * q - 0.5f;
                        const float k_o = other(k);
                        kl = (0.0f + (j == 0 ? k : k_o)) + (j == 0 ? k_o : k);
                        dmu += ri.klc * (-dm / (sig * sig));
                        dls += ri.klc * (1.0f - q);
                    }
                    dmu += dlogp * z / sig;
                    dls += dlogp * (z * z - 1.0f);
                    dls += -cc.entropy_coeff;
                    dmu_w = wgt * dmu;
                    dls_w = wgt * dls;
                    st1 = wgt * (-surr);
                    st3 = wgt * kl;
                    st4 = wgt * ent;
                    st0 = st1 + ((cc.use_kl ? ri.klc * st3 : 0.0f) - cc.entropy_coeff * st4);
                    st7 = wgt * adv;
                }
                if (!live) dmu_w = dls_w = st0 = st1 = st3 = st4 = st7 = 0.0f;
                if (BF) { dmu_w = bf16r(dmu_w); dls_w = bf16r(dls_w); }
                douts[r * 4 + j] = dmu_w;
                douts[r * 4 + 2 + j] = dls_w;
                if (rok) {
                    float* dg = a.ws + ws_dout(a, g) + (size_t)m * 4;
                    dg[j] = dmu_w;
                    dg[2 + j] = dls_w;
                }
                if (j == 1) {
                    *reinterpret_cast<float4*>(sts + r * 8) = make_float4(st0, st1, 0.0f, st3);
                    *reinterpret_cast<float4*>(sts + r * 8 + 4) = make_float4(st4, 0.0f, 0.0f, st7);
                }
            }
        } else if (part == 63) {
            float st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            float dout[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = opnd<BF>(out[j] + b3v[j]);
            if (rok && !(a.dbg & 8)) head_row_terms(a, g, mode, policy, ri, wgt, out, dout, st);
            if (BF) {           // the loss is fp32; its gradient enters the bfloat16 graph rounded
#pragma unroll
                for (int j = 0; j < 4; ++j) dout[j] = bf16r(dout[j]);
            }
            *reinterpret_cast<float4*>(douts + r * 4) = make_float4(dout[0], dout[1], dout[2], dout[3]);
            if (rok) *reinterpret_cast<float4*>(a.ws + ws_dout(a, g) + (size_t)m * 4) = make_float4(dout[0], dout[1], dout[2], dout[3]);
            *reinterpret_cast<float4*>(sts + r * 8) = make_float4(st[0], st[1], st[2], st[3]);
            *reinterpret_cast<float4*>(sts + r * 8 + 4) = make_float4(st[4], st[5], st[6], st[7]);
        }
    }
    __syncthreads();
    RP_STAMP(4);
    if (tid < 8) {       // per-tile partial of the statistics, rows in a fixed order
        float sv = 0.0f;
#pragma unroll
        for (int rr = 0; rr < R8; ++rr) sv += sts[rr * 8 + tid];
        a.ws[ws_stats_at(a, g * a.stat_tiles + tile) + tid] = sv;
    }
    // ---- dz2 = (dout W3) * (1 - h2^2): this thread's column, its RW rows ----
    {
        float* dz2g = a.ws + ws_dz2(a, g);
        float wc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wc[j] = (j < OD) ? w3s[j * H + col] : 0.0f;
#pragma unroll
        for (int ii = 0; ii < RW; ++ii) {
            const int rr = RW * kh + ii;
            const float4 d = *reinterpret_cast<const float4*>(douts + rr * 4);
            const float h = h2s[rr * HP + col];
            const float v = opnd<BF>(opnd<BF>((d.x * wc[0] + d.y * wc[1]) + (d.z * wc[2] + d.w * wc[3])) * (1.0f - h * h));
            dzs[rr * HP + col] = v;
            if (m0 + rr < c.mb) store_next(&dz2g[(size_t)(m0 + rr) * H + col], v);
        }
    }
    __syncthreads();
    RP_STAMP(5);
    // ---- dz1 = (dz2 W2) * (1 - h1^2) ----
    c0 = v4f{0.f, 0.f, 0.f, 0.f}; c1 = v4f{0.f, 0.f, 0.f, 0.f};
    st8.template run<BF>(dzs, HP, kh * (H / KS), H / KS, total, lane, c0, c1);
    {
        float z[RW];
        meet(c0, c1, z);
        float* dz1g = a.ws + ws_dz1(a, g);
#pragma unroll
        for (int ii = 0; ii < RW; ++ii) {
            const int i = RW * kh + ii;
            if (m0 + i < c.mb) {
                const float h = h1s[i * HP + col];
                store_next(&dz1g[(size_t)(m0 + i) * H + col], opnd<BF>(opnd<BF>(z[ii]) * (1.0f - h * h)));
            }
        }
    }
    RP_STAMP(9);
    if ((a.dbg & 2048) && threadIdx.x == 0) g_wg_times[0][(blockIdx.x + blockIdx.y * gridDim.x) & 1023][1] = wall_clock64();
}

// ------------------------------------------------------------------------------------------------------------
// forward-only pass of the same nets for rollouts and the dense postprocess: 16 dense rows per workgroup and net,
// both layers through the transposed weight mirror (see rowpass_kernel), heads on the vector ALUs.  Net 0 (policy)
// can sample: action = mean + exp(log_std) * eps, its log-probability and the clipped action the simulator takes.
// ------------------------------------------------------------------------------------------------------------
struct FwdArgs {
    copo_ppo_cfg c;
    const float* theta;
    const float* theta_t;
    const float* obs_src;     // [n_rows][pol.in_dim]
    const float* cc_src;      // [n_rows][val.in_dim] (value nets)
    int64_t n_rows;
    int32_t first_net, n_nets;
    float* values;            // [n_nets][n_rows]: output 0 of value nets (slot of a policy net unused)
    float* dist_inputs;       // policy: [n_rows][4] or NULL
    const float* eps;         // policy: [n_rows][2] standard normal draws, or NULL = no sampling
    float* action;            // [n_rows][2]
    float* logp;              // [n_rows]
    float* clipped;           // [n_rows][2] or NULL
    const int64_t* rows;      // NULL: row m of the launch is row m of the sources / outputs; else rows[m] (n_out of them exist)
    int64_t n_out;            // rows of the sources / outputs (= n_rows without a row list)
};

// A bank of K policies (copo_mlp_forward_bank_f32, the BANK instantiations of mlp_fwd_kernel): blockIdx.y is the member, which owns rows
// [y R, (y + 1) R) of the sources and the outputs, R = n_rows = n_out, and the parameters `member_stride` floats into theta / theta_t
// per member.  Tiles are counted per member, so no tile spans two members and a member's last tile is masked as the last tile of a
// launch of its R rows alone.  Policy net only (first_net = 0, n_nets = 1), no row list, no values.
// SEAT mode (copo_mlp_forward_seats_f32, `counts` given): member y owns the row list rows[y cap .. y cap + counts[y]) instead of a slice,
// cap = n_rows of the launch; sources and outputs are the shared [n_out] arrays, read and written at the listed rows only.  A workgroup
// whose first row is past counts[y] leaves before its first barrier (the test is uniform over the workgroup); from there on the
// member's list is the row list of a single-member launch of counts[y] rows, last tile masked alike.
struct FwdBankArgs : FwdArgs {
    int64_t member_stride;
    const int32_t* counts;    // [n_members] on the device, or NULL: the dense bank
};

// RT: 16-row tiles per workgroup.  RT = 2 (launcher: hidden 256, enough rows to fill the chip) halves the weight bytes a row costs and
// the number of workgroup prologues / epilogues per row; the input rows share LDS with the second hidden layer (dead after layer 1).
// BANK: the prologue below moves the member's parameters, sources and outputs into `a`; everything after it is the one body.  (A
// __device__ function shared by two __global__s changed the register allocation of the single-member hidden-512 kernels, 168 -> 196
// VGPRs; a template parameter leaves the BANK = false instantiations as they were.)
template <int NT, int WAVES, bool BF = false, int RT = 1, bool BANK = false>
__global__ void __launch_bounds__(64 * WAVES, RT > 1 ? 4 : 1) mlp_fwd_kernel(std::conditional_t<BANK, FwdBankArgs, FwdArgs> a) {      // (RT = 2: four waves per SIMD = two workgroups per CU)
    extern __shared__ float4 fwd_lds[];
    constexpr int H = 16 * NT * WAVES, HP = H + 4, TH = 64 * WAVES, RWS = HT * RT, TPR = TH / RWS;
    constexpr int DB = NT >= 8 ? 4 : (H / 16 >= 8 ? 8 : H / 16);
    const copo_ppo_cfg& c = a.c;
    const int g = BANK ? 0 : a.first_net + blockIdx.y;
    if constexpr (BANK) {
        const size_t k = blockIdx.y, r0 = k * (size_t)a.n_rows;
        a.theta += k * a.member_stride;
        a.theta_t += k * a.member_stride;
        if (a.counts) {       // seat mode: the member's row list takes the slice's place
            const int64_t n = a.counts[k] < a.n_rows ? a.counts[k] : a.n_rows;      // (a list holds `cap` rows at the most)
            if ((int64_t)blockIdx.x * RWS >= n) return;
            a.rows += r0;
            a.n_rows = n;
        } else {
            a.obs_src += r0 * c.pol.in_dim;
            if (a.dist_inputs) a.dist_inputs += r0 * 4;
            if (a.eps) { a.eps += r0 * 2; a.action += r0 * 2; a.logp += r0; }
            if (a.clipped) a.clipped += r0 * 2;
        }
    }
    const int64_t m0 = (int64_t)blockIdx.x * RWS;
    const copo_net_layout L = g == 0 ? c.pol : c.val[g - 1];
    const float* src = g == 0 ? a.obs_src : a.cc_src;
    auto row_at = [&](int64_t mm) -> int64_t { return mm < a.n_rows ? (a.rows ? a.rows[mm] : mm) : 0; };
    const int K1 = L.in_dim, OD = L.out_dim, K1P = rowpass_k1p(K1), XP = K1P + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 15, lj = lane >> 4, cb = wave * (16 * NT);
    float* h1s = reinterpret_cast<float*>(fwd_lds);    // [RWS][HP]
    float* h2s = h1s + RWS * HP;                        // [RWS][HP]
    float* xs = RT > 1 ? h2s : h2s + RWS * HP;          // [RWS][XP]  (RT > 1: inside h2s -- XP <= HP is checked by the launcher)
    float* w3s = (RT > 1 ? h2s + RWS * HP : xs + RWS * XP);      // [4][H]
    BRing<NT, DB, false> ring;         // (bfloat16-operand mode: the mirror holds rounded weights)
    ring.start(a.theta_t + L.w1, H, cb, ln, lj);
    if ((K1 & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int qn = K1P >> 2;
        for (int i = tid; i < RWS * qn; i += TH) {
            const int row = i / qn, k = (i - row * qn) * 4;
            const bool ok = (m0 + row < a.n_rows) && (k < K1);
            float4 v = *reinterpret_cast<const float4*>(src + (size_t)row_at(m0 + row) * K1 + (k < K1 ? k : 0));
            if (BF) v = make_float4(bf16r(v.x), bf16r(v.y), bf16r(v.z), bf16r(v.w));
            *reinterpret_cast<float4*>(xs + row * XP + k) = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        for (int i = tid; i < RWS * K1P; i += TH) {
            const int row = i / K1P, k = i - row * K1P;
            const bool ok = (m0 + row < a.n_rows) && (k < K1);
            const float v = opnd<BF>(src[(size_t)row_at(m0 + row) * K1 + (k < K1 ? k : 0)]);
            xs[row * XP + k] = ok ? v : 0.0f;
        }
    }
    for (int i = tid; i < OD * H; i += TH) w3s[i] = opnd<BF>(a.theta[L.w3 + i]);
    __syncthreads();
    v4f acc[RT][NT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[rt][t] = v4f{0.f, 0.f, 0.f, 0.f};
    ring.template run_tiles<RT>(xs, XP, (K1 + 15) & ~15, ln, lj, acc);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = cb + NT * ln + t;
        const float bv = opnd<BF>(a.theta[L.b1 + col]);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) h1s[(16 * rt + 4 * lj + rr) * HP + col] = opnd<BF>(tanh_fast(opnd<BF>(acc[rt][t][rr] + bv)));
    }
    ring.start(a.theta_t + L.w2, H, cb, ln, lj);
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[rt][t] = v4f{0.f, 0.f, 0.f, 0.f};
    ring.template run_tiles<RT>(h1s, HP, H, ln, lj, acc);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = cb + NT * ln + t;
        const float bv = opnd<BF>(a.theta[L.b2 + col]);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) h2s[(16 * rt + 4 * lj + rr) * HP + col] = opnd<BF>(tanh_fast(opnd<BF>(acc[rt][t][rr] + bv)));
    }
    __syncthreads();
    const int r = tid / TPR, part = tid % TPR;
    const int64_t mm = m0 + r;
    const int64_t m = row_at(mm);              // where this row's outputs go
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = part; i < H; i += TPR) {
        const float h = h2s[r * HP + i];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < OD) out[j] += h * w3s[j * H + i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int o = 1; o < TPR; o <<= 1) out[j] += __shfl_xor(out[j], o);
    }
    if (part != 0 || mm >= a.n_rows) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = opnd<BF>(out[j] + opnd<BF>(a.theta[L.b3 + (j < OD ? j : 0)]));
    if (g != 0) {
        a.values[(size_t)blockIdx.y * a.n_out + m] = out[0];
        return;
    }
    if (a.dist_inputs) *reinterpret_cast<float4*>(a.dist_inputs + (size_t)m * 4) = make_float4(out[0], out[1], out[2], out[3]);
    if (a.eps) {       // TorchDiagGaussian.sample / logp (RLlib): mean + std * eps, -0.5 sum z^2 - sum log_std - log(2 pi)
        float act[2], lp = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float sd = expf(out[2 + j]);
            act[j] = out[j] + sd * a.eps[(size_t)m * 2 + j];
            const float z = (act[j] - out[j]) / sd;
            lp += -0.5f * z * z - out[2 + j] - 0.5f * kLog2Pi;
        }
        a.action[(size_t)m * 2] = act[0];
        a.action[(size_t)m * 2 + 1] = act[1];
        a.logp[m] = lp;
        if (a.clipped) {
            a.clipped[(size_t)m * 2] = fminf(fmaxf(act[0], -1.0f), 1.0f);
            a.clipped[(size_t)m * 2 + 1] = fminf(fmaxf(act[1], -1.0f), 1.0f);
        }
    }
}
