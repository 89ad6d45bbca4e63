// Influence graph (copo_influence_*, include/copo_hip.h; eval/influence.py): whose presence moves whose action.
// A policy learns of other vehicles through the LiDAR block of its observation row alone, so "vehicle j taken out of the scene" is an
// exact counterfactual of ego i's row: every beam that j OWNS (j is its strict minimum) falls back to the second minimum.
//   heading  before a step: the heading unit vector the step will give every slot (slot_dynamics, the step's own P0), which the step's
//            LiDAR reads and the state does not keep
//   obs      one wave per row, lanes over beams in passes of 64: (min1, owner, min2) per beam in registers from ONE walk over the static
//            boxes and the other slots -- the step's pair record and ray_box_nr --, the candidates by a fixed-order selection, the
//            variant rows
//   lists    one workgroup per member: the variant rows of its seat list, ascending, by a prefix over lanes and waves (rowlog's assign)
//   tally    the variants' distribution inputs (copo_jury_obs_seats_f32 on the lists) against the driver's own, eight int64 words
// No atomic decides a position; the tally adds integers, so nothing depends on the order.  The rules are restated by tests/influence_numpy.py.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capi_common.h"
#include "seat_common.h"
#include "sim_device.h"

namespace copo {

namespace {

constexpr int ROWS_PER_WG = 4;             // waves of a 256-thread workgroup: one row each
constexpr int PASSES = COPO_MAX_LASERS / 64;
constexpr int LIST_THREADS = 1024, LIST_WAVES = LIST_THREADS / 64;
constexpr uint64_t NO_KEY = ~0ull;

__device__ inline uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int32_t)(uint32_t)(v & 0xffffffffu), o);
        const uint32_t hi = (uint32_t)__shfl_xor((int32_t)(uint32_t)(v >> 32), o);
        const uint64_t w = ((uint64_t)hi << 32) | (uint64_t)lo;
        v = w < v ? w : v;
    }
    return v;
}
__device__ inline uint64_t wave_or_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int32_t)(uint32_t)(v & 0xffffffffu), o);
        const uint32_t hi = (uint32_t)__shfl_xor((int32_t)(uint32_t)(v >> 32), o);
        v |= ((uint64_t)hi << 32) | (uint64_t)lo;
    }
    return v;
}

// The heading unit vector the step's LiDAR used for slot (e, j), whose status word is `status`: the road's for a vehicle spawned by the
// step (spawn_slot), else what the heading launch kept of the step's P0, else -- nothing kept: (0, 0) -- sincos of the stored heading,
// which is the step's vector for a vehicle that stood still.
__device__ inline void heading_of(const SimParams& p, const float* __restrict__ heading, size_t o, int32_t status, int32_t route_word,
                                  float th, float& c, float& s) {
    if (st_status(status) == ST_ALIVE && st_age(status) == 0) {
        const int route = route_word & 0xffff;
        const float* g = p.route_segs + (size_t)(route < p.n_routes ? route : 0) * p.seg_rows * COPO_SEG_STRIDE;
        c = g[2]; s = g[3];
        return;
    }
    if (heading) {
        c = heading[2 * o]; s = heading[2 * o + 1];
        if (c != 0.0f || s != 0.0f) return;
    }
    sincos_det(th, s, c);
}

}  // namespace

__global__ __launch_bounds__(256) void influence_heading_kernel(const SimParams* __restrict__ pp, const float* __restrict__ act,
                                                                float* __restrict__ heading) {
    const SimParams& p = *pp;
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= (size_t)p.E * p.N) return;
    Slot s;
    load_slot(p, (int)(o / p.N), (int)(o % p.N), s);
    bool acted;
    float acc;
    slot_dynamics<true>(p, act, o, s, acted, acc);
    heading[2 * o] = s.hc;
    heading[2 * o + 1] = s.hs;
}

// One beam against one box in the box's frame (the record of lidar_by_wave): the entering distance as fp32 bits, `range_bits` for a miss
// or a hit that is not below the range.  Distances are >= +0, so their bit patterns order them; a NaN's is above every range.
__device__ __forceinline__ uint32_t beam_bits(float ox, float oy, float cr, float sr, float2 r, float hl, float hw, uint32_t range_bits) {
    bool hit;
    const float tt = ray_box_nr(ox, oy, fm(r.x, cr, r.y * sr), fm(r.y, cr, -(r.x * sr)), hl, hw, hit);
    const uint32_t b = __float_as_uint(tt);
    return (hit && b < range_bits) ? b : range_bits;
}

__global__ __launch_bounds__(256) void influence_obs_kernel(const SimParams* __restrict__ pp, const int32_t* __restrict__ seat,
                                                            const float* __restrict__ heading, const float* __restrict__ obs, int32_t M,
                                                            int32_t* __restrict__ who, float* __restrict__ obs_cf, int32_t* __restrict__ ncand,
                                                            uint8_t* __restrict__ ego, float* __restrict__ hit_out, float* __restrict__ clean) {
    const SimParams& p = *pp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t EN = (size_t)p.E * p.N;
    const size_t r = (size_t)blockIdx.x * ROWS_PER_WG + wave;
    if (r >= EN) return;                       // (the whole wave; there is no barrier in this kernel)
    const int N = p.N, O = p.O, NL = p.num_lasers;
    const int e = (int)(r / N), n = (int)(r % N);
    const float* st = p.state;
    const int32_t* si = reinterpret_cast<const int32_t*>(st);
    const int32_t status_n = (si + 13 * EN)[r];
    const bool is_ego = seat[r] >= 0 && st_status(status_n) == ST_ALIVE;
    if (!is_ego) {
        if (lane < M) who[r * M + lane] = -1;
        if (lane == 0) { ncand[r] = 0; ego[r] = 0; }
        return;
    }
    const float hl = p.hl, hw = p.hw, range = p.lidar_range, inv_range = p.inv_range;
    const uint32_t range_bits = __float_as_uint(range);
    const float circ = sqrtf(hl * hl + hw * hw), lim = range + circ;
    const float xi = (st + 0 * EN)[r], yi = (st + 1 * EN)[r];
    float ci, sn_i;
    heading_of(p, heading, r, status_n, (si + 12 * EN)[r], (st + 2 * EN)[r], ci, sn_i);

    float2 ray[PASSES];
    uint32_t min1[PASSES], min2[PASSES];
    int own[PASSES];
#pragma unroll
    for (int q = 0; q < PASSES; ++q) {
        const int k = lane + 64 * q;
        ray[q] = k < NL ? reinterpret_cast<const float2*>(p.ray_cs)[k] : make_float2(1.0f, 0.0f);
        min1[q] = range_bits; min2[q] = range_bits; own[q] = -1;
    }
    // the static boxes first, as owner -1: a vehicle owns a beam only where it is strictly below them
    if (p.n_boxes_lidar > 0) {
        for (int b = 0; b < p.n_boxes; ++b) {
            const float* B = p.boxes + b * COPO_BOX_STRIDE;
            const float rx = B[0] - xi, ry = B[1] - yi, lb = range + (B[4] + B[5]);
            if (!(fm(rx, rx, ry * ry) <= lb * lb)) continue;      // (uniform)
            const float ox = -fm(rx, B[2], ry * B[3]), oy = -fm(ry, B[2], -(rx * B[3]));
            const float cr = fm(ci, B[2], sn_i * B[3]), sr = fm(ci, B[3], -(sn_i * B[2]));
#pragma unroll
            for (int q = 0; q < PASSES; ++q) {
                if (64 * q >= NL) break;
                const uint32_t d = beam_bits(ox, oy, cr, sr, ray[q], B[4], B[5], range_bits);
                min1[q] = d < min1[q] ? d : min1[q];
            }
        }
    }
    // the other slots in slot order: a later slot takes a beam only when strictly nearer, so ties stay with the lower slot
    for (int j = 0; j < N; ++j) {
        const size_t oj = (size_t)e * N + j;
        const int32_t status_j = (si + 13 * EN)[oj];
        if (j == n || st_status(status_j) == ST_EMPTY) continue;      // (uniform)
        const float dx = (st + 0 * EN)[oj] - xi, dy = (st + 1 * EN)[oj] - yi;
        if (fm(dx, dx, dy * dy) > lim * lim) continue;                // the step's own reach test on the centre distance (uniform)
        float cj, sj;
        heading_of(p, heading, oj, status_j, (si + 12 * EN)[oj], (st + 2 * EN)[oj], cj, sj);
        const float ox = -fm(dx, cj, dy * sj), oy = -fm(dy, cj, -(dx * sj));
        const float cr = fm(ci, cj, sn_i * sj), sr = fm(ci, sj, -(sn_i * cj));
#pragma unroll
        for (int q = 0; q < PASSES; ++q) {
            if (64 * q >= NL) break;
            const uint32_t d = beam_bits(ox, oy, cr, sr, ray[q], hl, hw, range_bits);
            if (d < min1[q]) { min2[q] = min1[q]; min1[q] = d; own[q] = j; }
            else if (d < min2[q]) min2[q] = d;
        }
    }
    // candidates: the owners by (smallest owned distance, slot), the first M kept
    uint64_t mine = 0ull;
#pragma unroll
    for (int q = 0; q < PASSES; ++q)
        if (lane + 64 * q < NL && own[q] >= 0) mine |= 1ull << own[q];
    const int owners = __popcll(wave_or_u64(mine));
    const int kept = owners < M ? owners : M;
    uint64_t taken = 0ull;
    int my_who = -1;                           // lane c: candidate c
    uint32_t my_hit = range_bits;
    for (int c = 0; c < kept; ++c) {
        uint64_t key = NO_KEY;
#pragma unroll
        for (int q = 0; q < PASSES; ++q) {
            if (lane + 64 * q < NL && own[q] >= 0 && !((taken >> own[q]) & 1ull)) {
                const uint64_t k = ((uint64_t)min1[q] << 8) | (uint64_t)own[q];
                key = k < key ? k : key;
            }
        }
        key = wave_min_u64(key);
        const int j = (int)(key & 255ull);
        taken |= 1ull << j;
        if (lane == c) { my_who = j; my_hit = (uint32_t)(key >> 8); }
    }
    if (lane < M) {
        who[r * M + lane] = my_who;
        if (hit_out) hit_out[r * M + lane] = __uint_as_float(my_hit) * inv_range;
    }
    if (lane == 0) { ncand[r] = kept | ((owners - kept) << 16); ego[r] = (uint8_t)COPO_F_ACTED; }
    const int col = p.col_lidar;
    if (clean) {
#pragma unroll
        for (int q = 0; q < PASSES; ++q)
            if (lane + 64 * q < NL) clean[r * NL + lane + 64 * q] = __uint_as_float(min1[q]) * inv_range;
    }
    const float* src = obs + r * O;
    for (int c = 0; c < kept; ++c) {
        const int j = __shfl(my_who, c);
        float* dst = obs_cf + (r * M + c) * O;
        for (int k = lane; k < O; k += 64)
            if (k < col || k >= col + NL) dst[k] = src[k];
#pragma unroll
        for (int q = 0; q < PASSES; ++q)
            if (lane + 64 * q < NL) dst[col + lane + 64 * q] = __uint_as_float(own[q] == j ? min2[q] : min1[q]) * inv_range;
    }
}

__global__ __launch_bounds__(LIST_THREADS) void influence_lists_kernel(const int64_t* __restrict__ rows, const int32_t* __restrict__ counts,
                                                                       int64_t cap, int64_t n_out, const int32_t* __restrict__ ncand, int32_t M,
                                                                       int64_t* __restrict__ vrows, int32_t* __restrict__ vcounts) {
    __shared__ int wsum[LIST_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = blockIdx.x;
    int64_t cnt = counts[k];
    cnt = cnt < 0 ? 0 : (cnt > cap ? cap : cnt);
    const int64_t* list = rows + (size_t)k * cap;
    int64_t* dst = vrows + (size_t)k * cap * M;
    int64_t total = 0;
    for (int64_t i0 = 0; i0 < cnt; i0 += LIST_THREADS) {      // (uniform over the workgroup)
        const int64_t i = i0 + tid;
        const int64_t row = i < cnt ? list[i] : -1;
        int c = (row >= 0 && row < n_out) ? (ncand[row] & 0xffff) : 0;
        c = c > M ? M : c;
        int inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int off = 0, sum = 0;
#pragma unroll
        for (int w = 0; w < LIST_WAVES; ++w) {
            const int s = wsum[w];
            off += w < wave ? s : 0;
            sum += s;
        }
        const int64_t at = total + off + (inc - c);
        for (int q = 0; q < c; ++q) dst[at + q] = row * M + q;
        total += sum;
        __syncthreads();
    }
    if (tid == 0) vcounts[k] = (int32_t)total;
}

// The tally (the walk: seat_walk / SeatLane::serve, seat_common.h): a counted lane is an ego; it contributes its kept candidates' distances.
using InfluenceWords = WordKinds<W_COUNT, W_SUM, W_SUM, W_SUM, W_SUM, W_SUM, W_MAX, W_SUM>;

__global__ __launch_bounds__(256) void influence_tally_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ dist,
                                                              const float* __restrict__ verdict_cf, const int32_t* __restrict__ who,
                                                              const int32_t* __restrict__ ncand, const float* __restrict__ hit,
                                                              const int32_t* __restrict__ seat, const int32_t* __restrict__ group, int32_t E,
                                                              int32_t N, int32_t K, int32_t G, int32_t M, float delta_steer,
                                                              float delta_throttle, int64_t* __restrict__ out, float* __restrict__ edges) {
    seat_walk(seat, group, E, N, K, G, [&](const SeatLane& L) {
        const size_t idx = L.idx;
        const bool counted = L.seated && ((uint32_t)flags[idx] & COPO_F_ACTED) != 0u;
        if (!__ballot(counted)) return;        // (uniform)
        int64_t w[COPO_INFL_WORDS] = {1, 0, 0, 0, 0, 0, 0, 0};      // egos, pairs, moved, d0, d1, KL, max dev, truncated
        if (counted) {
            const float4 own = *reinterpret_cast<const float4*>(dist + idx * 4);
            w[7] = (int64_t)((uint32_t)ncand[idx] >> 16);
            for (int c = 0; c < M; ++c) {
                if (who[idx * M + c] < 0) continue;
                const float4 v = *reinterpret_cast<const float4*>(verdict_cf + ((idx * M + c) * K + L.s) * 4);
                const float d0 = fabsf(__fsub_rn(v.x, own.x)), d1 = fabsf(__fsub_rn(v.y, own.y));
                const double kl = jury_kl(own, v);
                w[1] += 1;
                w[2] += (d0 > delta_steer || d1 > delta_throttle) ? 1 : 0;
                w[3] += q16(d0);
                w[4] += q16(d1);
                w[5] += q16(kl);
                const int64_t m = q16(fmaxf(d0, d1));
                w[6] = m > w[6] ? m : w[6];
                if (edges) *reinterpret_cast<float4*>(edges + (idx * M + c) * 4) = make_float4(d0, d1, (float)kl, hit ? hit[idx * M + c] : 0.0f);
            }
        }
        L.serve(InfluenceWords{}, counted, w, out, [&](int m) { return (size_t)L.g * K + m; });
    });
}

}  // namespace copo

using namespace copo;

static int check_sim(const char* name, const copo_sim* sim) {
    if (!sim) return fail(COPO_ERR_NULL, "%s: NULL simulator", name);
    if (!sim->started) return fail(COPO_ERR_STATE, "%s: the simulator was never reset", name);
    return COPO_OK;
}

extern "C" int copo_influence_heading(copo_sim* sim, const float* act, float* heading, void* stream) {
    if (const int rc = check_sim("copo_influence_heading", sim)) return rc;
    if (!act || !heading) return fail(COPO_ERR_NULL, "copo_influence_heading: NULL argument");
    const size_t EN = (size_t)sim->p.E * sim->p.N;
    hipLaunchKernelGGL(influence_heading_kernel, dim3((unsigned)((EN + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), sim->p_dev,
                       act, heading);
    HIP_TRY(hipGetLastError());
    return COPO_OK;
}

extern "C" int copo_influence_obs(copo_sim* sim, const int32_t* seat, const float* heading, const float* obs, int32_t M, int32_t* who,
                                  float* obs_cf, int32_t* ncand, uint8_t* ego, float* hit, float* clean, void* stream) {
    if (const int rc = check_sim("copo_influence_obs", sim)) return rc;
    if (!seat || !obs || !who || !obs_cf || !ncand || !ego) return fail(COPO_ERR_NULL, "copo_influence_obs: NULL argument");
    if (M < 1 || M > COPO_INFL_MAX) return fail(COPO_ERR_DIM, "copo_influence_obs: M=%d (1..%d)", M, COPO_INFL_MAX);
    if (obs == obs_cf) return fail(COPO_ERR_DIM, "copo_influence_obs: obs_cf must not be obs");
    const size_t EN = (size_t)sim->p.E * sim->p.N;
    hipLaunchKernelGGL(influence_obs_kernel, dim3((unsigned)((EN + ROWS_PER_WG - 1) / ROWS_PER_WG)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       sim->p_dev, seat, heading, obs, M, who, obs_cf, ncand, ego, hit, clean);
    HIP_TRY(hipGetLastError());
    return COPO_OK;
}

extern "C" int copo_influence_lists(const int64_t* rows, const int32_t* counts, int32_t K, int64_t cap, int64_t n_out, const int32_t* ncand,
                                    int32_t M, int64_t* vrows, int32_t* vcounts, void* stream) {
    if (!rows || !counts || !ncand || !vrows || !vcounts) return fail(COPO_ERR_NULL, "copo_influence_lists: NULL argument");
    if (K < 1 || K > 65535 || cap < 1 || n_out < 1 || M < 1 || M > COPO_INFL_MAX || cap * M > 0x7fffffffll)
        return fail(COPO_ERR_DIM, "copo_influence_lists: K=%d (1..65535) cap=%lld n_out=%lld (>= 1) M=%d (1..%d), cap M below 2^31", K,
                    (long long)cap, (long long)n_out, M, COPO_INFL_MAX);
    hipLaunchKernelGGL(influence_lists_kernel, dim3(K), dim3(LIST_THREADS), 0, static_cast<hipStream_t>(stream), rows, counts, cap, n_out, ncand,
                       M, vrows, vcounts);
    HIP_TRY(hipGetLastError());
    return COPO_OK;
}

extern "C" int copo_influence_tally(const uint8_t* flags, const float* dist, const float* verdict_cf, const int32_t* who, const int32_t* ncand,
                                    const float* hit, const int32_t* seat, const int32_t* group, int32_t E, int32_t N, int32_t K, int32_t G,
                                    int32_t M, float delta_steer, float delta_throttle, int64_t* out, float* edges, void* stream) {
    if (!flags || !dist || !verdict_cf || !who || !ncand || !seat || !group || !out) return fail(COPO_ERR_NULL, "copo_influence_tally: NULL argument");
    if (const int rc = check_tally("copo_influence_tally", E, N, K, G)) return rc;
    if (M < 1 || M > COPO_INFL_MAX) return fail(COPO_ERR_DIM, "copo_influence_tally: M=%d (1..%d)", M, COPO_INFL_MAX);
    if (((reinterpret_cast<uintptr_t>(dist) | reinterpret_cast<uintptr_t>(verdict_cf) | reinterpret_cast<uintptr_t>(edges)) & 15) != 0)
        return fail(COPO_ERR_DIM, "copo_influence_tally: dist, verdict_cf and edges must be 16-byte aligned (their rows are one 128-bit word)");
    if (E == 0) return COPO_OK;
    hipLaunchKernelGGL(influence_tally_kernel, tally_grid(E), dim3(256), 0, static_cast<hipStream_t>(stream), flags, dist,
                       verdict_cf, who, ncand, hit, seat, group, E, N, K, G, M, delta_steer, delta_throttle, out, edges);
    HIP_TRY(hipGetLastError());
    return COPO_OK;
}
