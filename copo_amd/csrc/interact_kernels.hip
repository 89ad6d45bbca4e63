// Interaction meter over the simulator's scenes (copo_interact_*, include/copo_hip.h): surrogate safety measures of every driving
// agent against the other bodies of its scene.  One workgroup per scene: wave 0 stages the poses of the ALIVE / WRECK slots into a
// dense LDS list (ballot + prefix count), all lanes share the unordered pairs of that list (body-to-body gap, swept-axes time to
// collision), per-body minima are LDS integer minima -- non-negative floats order as unsigned integers, so the minimum is exact and
// does not depend on the order the pairs arrive in -- and wave 0 updates the per-agent accumulators; agents that ended are folded
// into the scene totals by one lane in slot order.  The rules are restated in numpy by
// tests/interact_numpy.py.
#include "sim_device.h"
#include "interact_common.h"

namespace copo {

namespace {

constexpr uint32_t INF_BITS = 0x7f800000u;

// one separating axis of the sweep: the bodies overlap on it for t in [lo, hi] (p: centre offset, q: its rate, r: sum of the half extents)
__device__ __forceinline__ void sweep_axis(float p, float q, float r, float& t_in, float& t_out, bool& never) {
    if (q == 0.0f) {
        never = never | (fabsf(p) > r);
    } else {
        const float inv = 1.0f / q;
        const float t1 = (-r - p) * inv, t2 = (r - p) * inv;
        t_in = fmaxf(t_in, fminf(t1, t2));
        t_out = fminf(t_out, fmaxf(t1, t2));
    }
}

// squared distance of a point (x, y), given in a body's frame, to that body's rectangle
__device__ __forceinline__ float rect_d2(float x, float y, float hl, float hw) {
    const float ax = fmaxf(fabsf(x) - hl, 0.0f), ay = fmaxf(fabsf(y) - hw, 0.0f);
    return fm(ax, ax, ay * ay);
}

}  // namespace

__global__ __launch_bounds__(256) void interact_record_kernel(InteractArgs a, float* __restrict__ gap_out, float* __restrict__ ttc_out) {
    __shared__ float sx[64], sy[64], sc[64], ss[64], sv[64];      // dense list of the scene's bodies: centre, heading vector, speed
    __shared__ int sown[64];                                       // 1: ALIVE (owns measurements), 0: WRECK (an obstacle, v = 0)
    __shared__ uint32_t sgap[64], sttc[64];                        // per-body minima, float bits
    __shared__ int sM;
    // agents that ended in this record, by slot
    __shared__ int f_steps[64], f_tet[64], f_near[64], f_brake[64];
    __shared__ float f_gap[64], f_ttc[64];
    __shared__ double f_tit[64];
    const int tid = threadIdx.x, e = blockIdx.x, N = a.N;
    const size_t EN = (size_t)a.E * N;
    const unsigned int o = (unsigned int)e * (unsigned int)N + (unsigned int)tid;      // slot `tid` of the scene (wave 0, tid < N)
    const int32_t* si32 = reinterpret_cast<const int32_t*>(a.state);

    // ---- stage ----
    int st = ST_EMPTY, aid = 0, pos = 0;
    float v = 0.0f;
    if (tid < 64) {
        float x = 0.0f, y = 0.0f, th = 0.0f;
        if (tid < N) {
            x = a.state[o]; y = (a.state + EN)[o]; th = (a.state + 2 * EN)[o]; v = (a.state + 3 * EN)[o];
            st = st_status((si32 + 13 * EN)[o]); aid = (si32 + 14 * EN)[o];
        }
        const bool present = st == ST_ALIVE || st == ST_WRECK;
        const unsigned long long m = __ballot(present);
        pos = __popcll(m & ((1ull << tid) - 1ull));
        if (present) {
            float sn, cs;
            sincos_det(th, sn, cs);
            sx[pos] = x; sy[pos] = y; sc[pos] = cs; ss[pos] = sn;
            sv[pos] = st == ST_ALIVE ? v : 0.0f;
            sown[pos] = st == ST_ALIVE;
            sgap[pos] = INF_BITS; sttc[pos] = INF_BITS;
        }
        if (tid == 0) sM = __popcll(m);
    }
    __syncthreads();

    // ---- pairs: offset c + 1 around the list for every body, c < (M - 1) / 2; for even M the opposite bodies once ----
    {
        const int M = sM, full = M * ((M - 1) / 2), total = M * (M - 1) / 2;
        const float hl = a.hl, hw = a.hw;
        for (int k = tid; k < total; k += blockDim.x) {
            int i, j;
            if (k < full) {
                const int c = k / M;
                i = k - c * M;
                j = i + 1 + c;
                j = j >= M ? j - M : j;
            } else {
                i = k - full;
                j = i + M / 2;
            }
            const int own_i = sown[i], own_j = sown[j];
            if (!(own_i | own_j)) continue;
            const float ci = sc[i], si = ss[i], cj = sc[j], sj = ss[j], vi = sv[i], vj = sv[j];
            const float dx = sx[j] - sx[i], dy = sy[j] - sy[i];
            const float dot = fm(ci, cj, si * sj), crs = ci * sj - si * cj;      // u_i . u_j, u_i x u_j
            const float cc = fabsf(dot), sn = fabsf(crs);
            const float ru = fm(hw, sn, fm(hl, cc, hl)), rn = fm(hl, sn, fm(hw, cc, hw));      // extents along a heading / a normal
            const float p0 = fm(dx, ci, dy * si), p1 = fm(dy, ci, -(dx * si));      // d in i's frame
            const float p2 = fm(dx, cj, dy * sj), p3 = fm(dy, cj, -(dx * sj));      // d in j's frame
            const bool overlap = fabsf(p0) <= ru && fabsf(p1) <= rn && fabsf(p2) <= ru && fabsf(p3) <= rn;
            float gap = 0.0f;
            if (!overlap) {
                float d2 = __uint_as_float(INF_BITS);
                const float lc = hl * dot, ls = hl * crs, wc = hw * dot, ws = hw * crs;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float sa = (q & 1) ? -1.0f : 1.0f, sb = (q & 2) ? -1.0f : 1.0f;
                    // vertex c_i + sa hl u_i + sb hw n_i in j's frame; vertex c_j + sa hl u_j + sb hw n_j in i's frame
                    d2 = fminf(d2, rect_d2(fm(sb, ws, fm(sa, lc, -p2)), fm(sb, wc, fm(-sa, ls, -p3)), hl, hw));
                    d2 = fminf(d2, rect_d2(fm(-sb, ws, fm(sa, lc, p0)), fm(sb, wc, fm(sa, ls, p1)), hl, hw));
                }
                gap = sqrtf(d2);
            }
            const float wx = vj * cj - vi * ci, wy = vj * sj - vi * si;
            float t_in = -__uint_as_float(INF_BITS), t_out = __uint_as_float(INF_BITS);
            bool never = false;
            sweep_axis(p0, fm(wx, ci, wy * si), ru, t_in, t_out, never);
            sweep_axis(p1, fm(wy, ci, -(wx * si)), rn, t_in, t_out, never);
            sweep_axis(p2, fm(wx, cj, wy * sj), ru, t_in, t_out, never);
            sweep_axis(p3, fm(wy, cj, -(wx * sj)), rn, t_in, t_out, never);
            float ttc = __uint_as_float(INF_BITS);
            if (!never && t_in <= t_out && t_out >= 0.0f) ttc = t_in > 0.0f ? t_in : 0.0f;
            if (ttc > a.horizon_s) ttc = __uint_as_float(INF_BITS);
            const uint32_t gb = __float_as_uint(gap), tb = __float_as_uint(ttc);
            if (own_i) { atomicMin(&sgap[i], gb); atomicMin(&sttc[i], tb); }
            if (own_j) { atomicMin(&sgap[j], gb); atomicMin(&sttc[j], tb); }
        }
    }
    __syncthreads();

    // ---- per slot: outputs and accumulators (wave 0, lane n = slot n) ----
    bool fold = false;
    if (tid < N) {
        const bool alive = st == ST_ALIVE;
        const float gap = alive ? __uint_as_float(sgap[pos]) : __uint_as_float(INF_BITS);
        const float ttc = alive ? __uint_as_float(sttc[pos]) : __uint_as_float(INF_BITS);
        if (gap_out) gap_out[o] = gap;
        if (ttc_out) ttc_out[o] = ttc;
        const int ep = a.env[(size_t)e * 4 + 1];
        int32_t* A = a.acc + o;
        int steps = A[IA_STEPS * EN];
        if (steps > 0 && (!alive || A[IA_AID * EN] != aid || A[IA_EPISODE * EN] != ep)) {
            fold = true;
            f_steps[tid] = steps; f_tet[tid] = A[IA_TET_STEPS * EN]; f_near[tid] = A[IA_NEAR_EVENTS * EN]; f_brake[tid] = A[IA_BRAKE_EVENTS * EN];
            f_gap[tid] = __int_as_float(A[IA_MIN_GAP * EN]); f_ttc[tid] = __int_as_float(A[IA_MIN_TTC * EN]);
            f_tit[tid] = a.tit[o];
            steps = 0;
            if (!alive) A[IA_STEPS * EN] = 0;
        }
        if (alive) {
            float min_gap = gap, min_ttc = ttc;
            int tet = 0, near_ev = 0, in_near = 0, brake = 0;
            double tit = 0.0;
            if (steps > 0) {
                min_gap = fminf(min_gap, __int_as_float(A[IA_MIN_GAP * EN])); min_ttc = fminf(min_ttc, __int_as_float(A[IA_MIN_TTC * EN]));
                tet = A[IA_TET_STEPS * EN]; near_ev = A[IA_NEAR_EVENTS * EN]; in_near = A[IA_IN_NEAR * EN]; brake = A[IA_BRAKE_EVENTS * EN];
                tit = a.tit[o];
                brake += ((__int_as_float(A[IA_LAST_SPEED * EN]) - v) / a.dt > a.brake_mps2) ? 1 : 0;
            }
            const bool critical = ttc < a.ttc_crit_s;
            if (critical) {
                tet += 1;
                tit += ((double)a.ttc_crit_s - (double)ttc) * (double)a.dt;
            }
            const int is_near = (critical || gap < a.gap_near_m) ? 1 : 0;
            near_ev += is_near & (in_near ^ 1);
            A[IA_AID * EN] = aid; A[IA_EPISODE * EN] = ep; A[IA_STEPS * EN] = steps + 1;
            A[IA_MIN_GAP * EN] = __float_as_int(min_gap); A[IA_MIN_TTC * EN] = __float_as_int(min_ttc);
            A[IA_TET_STEPS * EN] = tet; A[IA_NEAR_EVENTS * EN] = near_ev; A[IA_IN_NEAR * EN] = is_near; A[IA_BRAKE_EVENTS * EN] = brake;
            A[IA_LAST_SPEED * EN] = __float_as_int(v);
            a.tit[o] = tit;
        }
    }
    // ---- fold the ended agents into the scene totals: one lane, slot order (fp64 sums reproducible bit for bit) ----
    unsigned long long folded = __ballot(fold);      // (wave 0 holds the slots: lane 0 of the workgroup sees all of them)
    __syncthreads();
    if (tid == 0 && folded) {
        long long* Cn = a.counts + (size_t)e * INTERACT_COUNTS;
        double* S = a.sums + (size_t)e * INTERACT_SUMS;
        long long agents = Cn[IC_AGENTS], steps = Cn[IC_STEPS], tet = Cn[IC_TET_STEPS], near_ev = Cn[IC_NEAR_EVENTS], brake = Cn[IC_BRAKE_EVENTS],
                  finite = Cn[IC_FINITE_TTC];
        double s_gap = S[IS_MIN_GAP], s_ttc = S[IS_MIN_TTC], s_tit = S[IS_TIT];
        while (folded) {
            const int n = __ffsll((long long)folded) - 1;
            folded &= folded - 1ull;
            agents += 1; steps += f_steps[n]; tet += f_tet[n]; near_ev += f_near[n]; brake += f_brake[n];
            s_gap += (double)f_gap[n];
            const float t = f_ttc[n];
            if (t < __uint_as_float(INF_BITS)) { finite += 1; s_ttc += (double)t; }
            s_tit += f_tit[n];
        }
        Cn[IC_AGENTS] = agents; Cn[IC_STEPS] = steps; Cn[IC_TET_STEPS] = tet; Cn[IC_NEAR_EVENTS] = near_ev; Cn[IC_BRAKE_EVENTS] = brake;
        Cn[IC_FINITE_TTC] = finite;
        S[IS_MIN_GAP] = s_gap; S[IS_MIN_TTC] = s_ttc; S[IS_TIT] = s_tit;
    }
}

// one lane per scene
__global__ __launch_bounds__(64) void interact_totals_kernel(InteractArgs a, long long* __restrict__ counts_out, double* __restrict__ sums_out,
                                                            int flush_open) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    const size_t EN = (size_t)a.E * a.N;
    long long c[INTERACT_COUNTS];
    double s[INTERACT_SUMS];
    for (int k = 0; k < INTERACT_COUNTS; ++k) c[k] = a.counts[(size_t)e * INTERACT_COUNTS + k];
    for (int k = 0; k < INTERACT_SUMS; ++k) s[k] = a.sums[(size_t)e * INTERACT_SUMS + k];
    if (flush_open) {
        for (int n = 0; n < a.N; ++n) {
            const size_t o = (size_t)e * a.N + n;
            const int32_t* A = a.acc + o;
            const int steps = A[IA_STEPS * EN];
            if (steps == 0) continue;
            c[IC_AGENTS] += 1; c[IC_STEPS] += steps; c[IC_TET_STEPS] += A[IA_TET_STEPS * EN]; c[IC_NEAR_EVENTS] += A[IA_NEAR_EVENTS * EN];
            c[IC_BRAKE_EVENTS] += A[IA_BRAKE_EVENTS * EN];
            s[IS_MIN_GAP] += (double)__int_as_float(A[IA_MIN_GAP * EN]);
            const float t = __int_as_float(A[IA_MIN_TTC * EN]);
            if (t < __uint_as_float(INF_BITS)) { c[IC_FINITE_TTC] += 1; s[IS_MIN_TTC] += (double)t; }
            s[IS_TIT] += a.tit[o];
        }
    }
    for (int k = 0; k < INTERACT_COUNTS; ++k) counts_out[(size_t)e * INTERACT_COUNTS + k] = c[k];
    for (int k = 0; k < INTERACT_SUMS; ++k) sums_out[(size_t)e * INTERACT_SUMS + k] = s[k];
}

// threads per scene: four waves share the pairs while the scenes leave compute units idle, one wave per scene beyond that
hipError_t launch_interact_record(const InteractArgs& a, float* gap, float* ttc, hipStream_t stream) {
    const int block = a.E <= 2048 ? 256 : 64;
    hipLaunchKernelGGL(interact_record_kernel, dim3(a.E), dim3(block), 0, stream, a, gap, ttc);
    return hipGetLastError();
}

hipError_t launch_interact_totals(const InteractArgs& a, long long* counts_out, double* sums_out, int flush_open, hipStream_t stream) {
    hipLaunchKernelGGL(interact_totals_kernel, dim3((a.E + 63) / 64), dim3(64), 0, stream, a, counts_out, sums_out, flush_open);
    return hipGetLastError();
}

}  // namespace copo
