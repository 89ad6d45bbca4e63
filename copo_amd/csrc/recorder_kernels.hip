// Device evaluation recorder (copo_recorder_*, include/copo_hip.h): the per-episode evaluation row of the reference's RecorderEnv
// (copo/eval/recoder.py:188-349, with its SVO estimate :326-347) for E scenes, folded from one sampler fragment [T][E][N] per call.
// Three launches per fragment, whatever T is, and no host read:
//   count:   one wave per scene walks the fragment's flags: how many episodes of the scene end in it with at least one terminated
//            agent -- the rows it will emit
//   assign:  rowlog::assign: every scene gets the id of its first row, in scene order; ids from max_rows on are dropped
//   fold:    one wave per scene, four scenes per 256-thread workgroup, lanes over the slots (slot n = lane + 64 k); the loop over the T
//            steps runs here with the scene's accumulators and the slots' sums in registers, the next step's inputs are loaded while
//            this step is folded; a step that ends an episode writes the row and re-arms the accumulators
// count and fold decide what ends and what is emitted with the same integer rules.  The order of every sum over slots is
// recorder_common.h; the rules are restated by tests/recorder_numpy.py.  DESIGN.md section 8j.
#include <math.h>

#include "../../include/copo_hip.h"
#include "recorder_common.h"

namespace copo {

using namespace rowlog;

namespace {

constexpr double REC_INF = __builtin_huge_val();
constexpr double DEG = 180.0 / 3.14159265358979323846, RAD = 3.14159265358979323846 / 180.0;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ int votes(bool p) { return __popcll(__ballot(p)); }

__device__ __forceinline__ bool stopped(const RecorderArgs& a, long long episodes) { return a.limit > 0 && episodes >= a.limit; }

// one slot's inputs of one step; a lane without a slot reads flags 0 and takes part in nothing
struct SlotIn {
    uint32_t f;
    float vel, cost, len, erew, rew, nrew;
    int32_t nbr;
};

__device__ __forceinline__ SlotIn load_slot(const RecorderArgs& a, int t, int e, int n) {
    SlotIn s = {0u, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0};
    if (t < a.T && n < a.N) {
        const size_t o = ((size_t)t * a.E + e) * a.N + n;
        const float4 hi = reinterpret_cast<const float4*>(a.infos)[o * 2 + 1];     // cost, episode length, episode reward, -
        s.f = a.flags[o];
        s.vel = a.infos[o * COPO_INFO_DIM + COPO_I_VELOCITY];
        s.cost = hi.x; s.len = hi.y; s.erew = hi.z;
        s.rew = a.rew[o]; s.nrew = a.nei_rew[o]; s.nbr = a.nbr_cnt[o];
    }
    return s;
}

__device__ __forceinline__ void arm(double* A) {
#pragma unroll
    for (int k = 0; k < REC_ACC; ++k) A[k] = 0.0;
    A[RA_VMIN] = A[RA_RMIN] = A[RA_CMIN] = A[RA_SVO_MIN] = REC_INF;
    A[RA_VMAX] = A[RA_NMAX] = A[RA_RMAX] = A[RA_CMAX] = A[RA_SVO_MAX] = -REC_INF;
}

// the row of a finished episode (VecRecorder._flush, then recoder.py:326-347); n = A[RA_AGENTS] > 0
__device__ __forceinline__ void write_row(double* R, const double* A, int e, long long episode) {
    const double n = A[RA_AGENTS], steps = A[RA_STEPS] > 1.0 ? A[RA_STEPS] : 1.0, succ = A[RA_SUCC];
    R[0] = A[RA_VMIN];
    R[1] = A[RA_VSUM] / (A[RA_VSTEPS] > 1.0 ? A[RA_VSTEPS] : 1.0);
    R[2] = A[RA_VMAX];
    R[3] = A[RA_NSUM] / (A[RA_NSTEPS] > 1.0 ? A[RA_NSTEPS] : 1.0);
    R[4] = A[RA_NMAX];
    R[5] = n;
    R[6] = n / steps * 300.0;
    R[7] = succ / n;
    R[8] = succ;
    R[9] = succ / steps * 300.0;
    R[10] = A[RA_CRASH] / steps * 300.0;
    R[11] = A[RA_RSUM] / n;
    R[12] = A[RA_RMIN];
    R[13] = A[RA_RMAX];
    R[14] = A[RA_CSUM] / n;
    R[15] = A[RA_CMIN];
    R[16] = A[RA_CMAX];
    R[17] = A[RA_CSUM];
    R[18] = A[RA_CRASH] / n;
    R[19] = A[RA_CRASH];
    R[20] = A[RA_OUT] / n;
    R[21] = A[RA_OUT];
    R[22] = A[RA_LSUM] / n;
    R[23] = succ > 0.0 ? A[RA_SLSUM] / succ : 0.0;
    R[24] = A[RA_STEPS];
    R[25] = A[RA_SVO_SUM] / A[RA_SVO_N];
    R[26] = A[RA_SVO_MIN];
    R[27] = A[RA_SVO_MAX];
    R[28] = A[RA_SVO_REW] / n;
    R[29] = (double)e;
    R[30] = (double)episode;
}

}  // namespace

__global__ __launch_bounds__(TB) void recorder_count_kernel(RecorderArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = blockIdx.x * NW + wave; e < a.E; e += gridDim.x * NW) {       // (the whole wave)
        long long episodes = a.episodes[e];
        bool agents = a.acc[(size_t)e * REC_ACC + RA_AGENTS] > 0.0;
        int rows = 0;
        for (int t = 0; t < a.T && !stopped(a, episodes); ++t) {
            const uint8_t* f = a.flags + ((size_t)t * a.E + e) * a.N;
            bool done = false, reset = false;
            for (int n = lane; n < a.N; n += 64) {
                const uint32_t w = f[n];
                done |= (w & (COPO_F_ACTED | COPO_F_DONE)) == (COPO_F_ACTED | COPO_F_DONE);
                reset |= (w & COPO_F_ENV_RESET) != 0u;
            }
            agents |= __ballot(done) != 0ull;
            if (__ballot(reset) != 0ull) {
                rows += agents ? 1 : 0;
                agents = false;
                episodes += 1;
            }
        }
        if (lane == 0) a.n_rows[e] = rows;
    }
}

__global__ __launch_bounds__(ASSIGN_THREADS) void recorder_assign_kernel(RecorderArgs a) {
    assign(a.ids, a.E, [&](int e) { return a.n_rows[e]; });
}

// KS: slots per lane, N <= 64 KS
template <int KS>
__global__ __launch_bounds__(TB) void recorder_fold_kernel(RecorderArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N;
    const size_t EN = (size_t)a.E * N;
    for (int e = blockIdx.x * NW + wave; e < a.E; e += gridDim.x * NW) {       // (the whole wave)
        long long episodes = a.episodes[e];
        if (stopped(a, episodes)) continue;
        long long id = a.ids.base[e];
        double A[REC_ACC];
#pragma unroll
        for (int k = 0; k < REC_ACC; ++k) A[k] = a.acc[(size_t)e * REC_ACC + k];
        double cost[KS], own[KS], nei[KS];
        SlotIn cur[KS], nxt[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const int n = lane + 64 * k;
            const size_t o = (size_t)e * N + n;
            cost[k] = n < N ? a.slots[RS_COST * EN + o] : 0.0;
            own[k] = n < N ? a.slots[RS_OWN * EN + o] : 0.0;
            nei[k] = n < N ? a.slots[RS_NEI * EN + o] : 0.0;
            cur[k] = load_slot(a, 0, e, n);
        }
        for (int t = 0; t < a.T && !stopped(a, episodes); ++t) {
            bool reset = false;
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                nxt[k] = load_slot(a, t + 1, e, lane + 64 * k);
                reset |= (cur[k].f & COPO_F_ENV_RESET) != 0u;
            }
            // (the row that carries F_ENV_RESET flags the NEXT episode's slots as spawned: not part of this episode)
            const bool resetting = __ballot(reset) != 0ull;
            int na = 0, npres = 0, nb = 0, ndone = 0;
            double vs = 0.0;
            bool done[KS];
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                const SlotIn& s = cur[k];
                const bool acted = (s.f & COPO_F_ACTED) != 0u;
                const bool present = acted || ((s.f & COPO_F_SPAWNED) != 0u && !resetting);
                done[k] = acted && (s.f & COPO_F_DONE) != 0u;
                na += votes(acted);
                npres += votes(present);
                ndone += votes(done[k]);
                vs = vs + (acted ? (double)s.vel : 0.0);
                if (acted) cost[k] = cost[k] + (double)s.cost;
                if (present) {
                    nb += s.nbr;
                    own[k] = own[k] + (double)s.rew;
                    nei[k] = nei[k] + (double)(s.nbr > 0 ? s.nrew : s.rew);      // (nobody in range: the agent's own reward, recoder.py:56)
                }
            }
            A[RA_STEPS] += 1.0;
            if (na > 0) {
                const double vel = wave_sum(vs) / (double)na;
                A[RA_VSTEPS] += 1.0;
                A[RA_VSUM] += vel;
                A[RA_VMIN] = vel < A[RA_VMIN] ? vel : A[RA_VMIN];
                A[RA_VMAX] = vel > A[RA_VMAX] ? vel : A[RA_VMAX];
            }
            if (npres > 0) {
                const double nn = (double)wave_sum(nb) / (double)npres;
                A[RA_NSTEPS] += 1.0;
                A[RA_NSUM] += nn;
                A[RA_NMAX] = nn > A[RA_NMAX] ? nn : A[RA_NMAX];
            }
            if (ndone > 0) {
                int nsucc = 0, ncrash = 0, nout = 0;
                double rs = 0.0, cs = 0.0, ls = 0.0, sls = 0.0, ss = 0.0, sr = 0.0;
                double rmin = REC_INF, rmax = -REC_INF, cmin = REC_INF, cmax = -REC_INF, smin = REC_INF, smax = -REC_INF;
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    const SlotIn& s = cur[k];
                    const bool d = done[k], won = d && (s.f & COPO_F_ARRIVE) != 0u;
                    nsucc += votes(won);
                    ncrash += votes(d && (s.f & COPO_F_CRASH) != 0u);
                    nout += votes(d && (s.f & COPO_F_OUT) != 0u);
                    double er = 0.0, ec = 0.0, el = 0.0, svo = 0.0, w = 0.0;
                    if (d) {
                        er = (double)s.erew; ec = cost[k]; el = (double)s.len;
                        const double alpha = atan2(nei[k], own[k]) * DEG;
                        svo = alpha < 0.0 ? 0.0 : (alpha > 90.0 ? 90.0 : alpha);
                        w = hypot(nei[k], own[k]) * cos((svo - alpha) * RAD);
                        rmin = er < rmin ? er : rmin; rmax = er > rmax ? er : rmax;
                        cmin = ec < cmin ? ec : cmin; cmax = ec > cmax ? ec : cmax;
                        smin = svo < smin ? svo : smin; smax = svo > smax ? svo : smax;
                        cost[k] = 0.0; own[k] = 0.0; nei[k] = 0.0;         // (a new occupant of the slot starts at zero)
                    }
                    rs = rs + er; cs = cs + ec; ls = ls + el; sls = sls + (won ? el : 0.0); ss = ss + svo; sr = sr + w;
                }
                A[RA_AGENTS] += (double)ndone; A[RA_SUCC] += (double)nsucc; A[RA_CRASH] += (double)ncrash; A[RA_OUT] += (double)nout;
                A[RA_RSUM] += wave_sum(rs); A[RA_CSUM] += wave_sum(cs); A[RA_LSUM] += wave_sum(ls); A[RA_SLSUM] += wave_sum(sls);
                rmin = wave_min(rmin); rmax = wave_max(rmax); cmin = wave_min(cmin); cmax = wave_max(cmax);
                smin = wave_min(smin); smax = wave_max(smax);
                A[RA_RMIN] = rmin < A[RA_RMIN] ? rmin : A[RA_RMIN]; A[RA_RMAX] = rmax > A[RA_RMAX] ? rmax : A[RA_RMAX];
                A[RA_CMIN] = cmin < A[RA_CMIN] ? cmin : A[RA_CMIN]; A[RA_CMAX] = cmax > A[RA_CMAX] ? cmax : A[RA_CMAX];
                A[RA_SVO_N] += (double)ndone; A[RA_SVO_SUM] += wave_sum(ss); A[RA_SVO_REW] += wave_sum(sr);
                A[RA_SVO_MIN] = smin < A[RA_SVO_MIN] ? smin : A[RA_SVO_MIN]; A[RA_SVO_MAX] = smax > A[RA_SVO_MAX] ? smax : A[RA_SVO_MAX];
            }
            if (resetting) {
                if (A[RA_AGENTS] > 0.0) {      // (an episode in which nobody terminated leaves no row, VecRecorder._flush)
                    if (lane == 0 && id < a.ids.max_rows) write_row(a.rows + (size_t)id * REC_NCOL, A, e, episodes);
                    id += 1;
                }
                episodes += 1;
                arm(A);
            }
#pragma unroll
            for (int k = 0; k < KS; ++k) cur[k] = nxt[k];
        }
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const int n = lane + 64 * k;
            const size_t o = (size_t)e * N + n;
            if (n < N) {
                a.slots[RS_COST * EN + o] = cost[k];
                a.slots[RS_OWN * EN + o] = own[k];
                a.slots[RS_NEI * EN + o] = nei[k];
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < REC_ACC; ++k) a.acc[(size_t)e * REC_ACC + k] = A[k];
            a.episodes[e] = episodes;
        }
    }
}

__global__ void recorder_arm_kernel(double* acc, int32_t E) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    double A[REC_ACC];
    arm(A);
#pragma unroll
    for (int k = 0; k < REC_ACC; ++k) acc[(size_t)e * REC_ACC + k] = A[k];
}

hipError_t launch_recorder_add(const RecorderArgs& a, hipStream_t stream) {
    void (*fold)(RecorderArgs) = a.N <= 64 ? recorder_fold_kernel<1> : a.N <= 128 ? recorder_fold_kernel<2> : recorder_fold_kernel<REC_SLOTS_PER_LANE>;
    hipLaunchKernelGGL(recorder_count_kernel, scene_grid(a.E), dim3(TB), 0, stream, a);
    hipLaunchKernelGGL(recorder_assign_kernel, dim3(1), dim3(ASSIGN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(fold, scene_grid(a.E), dim3(TB), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_recorder_arm(double* acc, int32_t E, hipStream_t stream) {
    hipLaunchKernelGGL(recorder_arm_kernel, dim3((E + 255) / 256), dim3(256), 0, stream, acc, E);
    return hipGetLastError();
}

}  // namespace copo
