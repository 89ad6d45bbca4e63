// Scene rewind (copo_rewind_*, include/copo_hip.h): a ring of FULL snapshots per scene on the device, forks of one scene at one past
// record into scenes of another simulator, and a tally of how the forked branches end.  A snapshot is everything a scene resumes
// from except its seed: the COPO_STATE_FIELDS words of every slot as raw bits and the scene's four env words; the seed is read from
// the source simulator when a fork is made.
//   record:  one wave per scene, four scenes per workgroup, lane n = slot n (loads and stores coalesced over the slots); lanes 0..3
//            copy the env words
//   fork:    one wave per TARGET scene; the request's scene index and record are checked here, an invalid request leaves an
//            all-EMPTY scene and status -1
//   tally:   one wave per scene over one step's flags: ballots and popcounts, lanes 0..7 own the eight words of the row; no atomics
// Copies, integer logic and one fp32 clamp only.  The rules are restated in numpy by tests/rewind_numpy.py.
#include "sim_device.h"
#include "rewind_common.h"

namespace copo {

namespace {

constexpr int SCENES_PER_WG = 4;       // waves of a 256-thread workgroup

}  // namespace

__global__ __launch_bounds__(256) void rewind_record_kernel(RewindArgs a, int place) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * SCENES_PER_WG + wave;
    if (e >= a.E) return;                      // (the whole wave; there is no barrier in this kernel)
    const int N = a.N;
    const size_t EN = (size_t)a.E * N, o = (size_t)e * N + lane;
    const size_t snap = (size_t)e * a.depth + place;
    if (lane < N) {
        const uint32_t* su = reinterpret_cast<const uint32_t*>(a.state);
        uint32_t* R = a.ring + snap * COPO_STATE_FIELDS * N + lane;
        uint32_t w[COPO_STATE_FIELDS];
#pragma unroll
        for (int f = 0; f < COPO_STATE_FIELDS; ++f) w[f] = (su + f * EN)[o];
#pragma unroll
        for (int f = 0; f < COPO_STATE_FIELDS; ++f) R[(size_t)f * N] = w[f];
    }
    if (lane < REWIND_ENV_WORDS) a.ring_env[snap * REWIND_ENV_WORDS + lane] = a.env[(size_t)e * 4 + lane];
}

__global__ __launch_bounds__(256) void rewind_fork_kernel(RewindForkArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * SCENES_PER_WG + wave;
    if (j >= a.S) return;
    const int N = a.N;
    const int sc = a.scene[j], rc = a.rec[j];
    bool valid = a.n_records > 0 && rc >= 0 && sc >= 0 && sc < a.E;
    int q = 0;
    if (valid) {                               // newest stored record <= rc; it must still be among the last `depth` stored ones
        const int last = a.n_records - 1;
        q = (rc < last ? rc : last) / a.stride;
        valid = q > last / a.stride - a.depth;
    }
    const size_t snap = valid ? (size_t)sc * a.depth + q % a.depth : 0;
    const float lv = a.lcf ? a.lcf[j] : 0.0f;
    const bool set_lcf = a.lcf && lv == lv;    // NaN: the snapshot's LCF stays
    const float lcf_new = fminf(fmaxf(lv, -1.0f), 1.0f);
    const size_t TEN = (size_t)a.TE * N, o = (size_t)(a.first + j) * N + lane;
    int32_t alive_aid = -1;
    if (lane < N) {
        uint32_t* tu = reinterpret_cast<uint32_t*>(a.state);
        const uint32_t* F = a.ring + snap * COPO_STATE_FIELDS * N + lane;
        uint32_t w[COPO_STATE_FIELDS];
#pragma unroll
        for (int f = 0; f < COPO_STATE_FIELDS; ++f) w[f] = valid ? F[(size_t)f * N] : (f == 13 ? (uint32_t)ST_EMPTY : 0u);
        const bool alive = valid && (w[13] & 0xffu) == (uint32_t)ST_ALIVE;
        if (alive) alive_aid = (int32_t)w[14];
        if (alive && set_lcf) w[10] = __float_as_uint(lcf_new);
#pragma unroll
        for (int f = 0; f < COPO_STATE_FIELDS; ++f) (tu + f * TEN)[o] = w[f];
    }
    const int ws = a.watch_slot ? a.watch_slot[j] : -1;
    const bool watched = ws >= 0 && ws < N;
    const int32_t got = __shfl(alive_aid, watched ? ws : 0);
    if (lane < REWIND_ENV_WORDS)
        a.env[(size_t)(a.first + j) * 4 + lane] = valid ? a.ring_env[snap * REWIND_ENV_WORDS + lane] : (lane == 3 ? 1 : 0);
    if (lane == 0) {
        a.status[j] = valid ? q * a.stride : -1;
        if (a.watch_aid) a.watch_aid[j] = watched ? got : -1;
        if (a.new_seeds) a.seeds[a.first + j] = a.new_seeds[j];
        else if (valid) a.seeds[a.first + j] = a.src_seeds[sc];
    }
}

__global__ __launch_bounds__(256) void rewind_tally_kernel(const uint8_t* __restrict__ flags, const int32_t* __restrict__ watch_slot,
                                                           int32_t* __restrict__ tally, int32_t B, int32_t N) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * SCENES_PER_WG + wave;
    if (b >= B) return;
    const uint32_t f = lane < N ? (uint32_t)flags[(size_t)b * N + lane] : 0u;
    const bool done = (f & COPO_F_DONE) != 0u;
    const int n_acted = __popcll(__ballot((f & COPO_F_ACTED) != 0u));
    const int n_arrive = __popcll(__ballot(done && (f & COPO_F_ARRIVE) != 0u));
    const int n_crash = __popcll(__ballot(done && (f & COPO_F_CRASH) != 0u));
    const int n_out = __popcll(__ballot(done && (f & COPO_F_OUT) != 0u));
    const int n_maxstep = __popcll(__ballot(done && (f & COPO_F_MAXSTEP) != 0u));
    const int ws = watch_slot ? watch_slot[b] : -1;
    const bool watched = ws >= 0 && ws < N;
    const uint32_t fw = __shfl(f, watched ? ws : 0);
    int32_t* T = tally + (size_t)b * REWIND_TALLY;
    const int32_t old = lane < REWIND_TALLY ? T[lane] : 0;
    const int32_t steps = __shfl(old, RT_STEPS), seen = __shfl(old, RT_WATCH_FLAGS);
    const bool hit = seen == 0 && watched && (fw & COPO_F_DONE) != 0u;      // the watched slot's FIRST end only
    if (lane < REWIND_TALLY) {
        int32_t v = old;
        if (lane == RT_STEPS) v += 1;
        else if (lane == RT_ACTED) v += n_acted;
        else if (lane == RT_ARRIVE) v += n_arrive;
        else if (lane == RT_CRASH) v += n_crash;
        else if (lane == RT_OUT) v += n_out;
        else if (lane == RT_MAXSTEP) v += n_maxstep;
        else if (lane == RT_WATCH_FLAGS) v = hit ? (int32_t)fw : old;
        else v = hit ? steps : old;
        T[lane] = v;
    }
}

hipError_t launch_rewind_record(const RewindArgs& a, int place, hipStream_t stream) {
    hipLaunchKernelGGL(rewind_record_kernel, dim3((a.E + SCENES_PER_WG - 1) / SCENES_PER_WG), dim3(256), 0, stream, a, place);
    return hipGetLastError();
}

hipError_t launch_rewind_fork(const RewindForkArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(rewind_fork_kernel, dim3((a.S + SCENES_PER_WG - 1) / SCENES_PER_WG), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_rewind_tally(const uint8_t* flags, const int32_t* watch_slot, int32_t* tally, int32_t B, int32_t N, hipStream_t stream) {
    hipLaunchKernelGGL(rewind_tally_kernel, dim3((B + SCENES_PER_WG - 1) / SCENES_PER_WG), dim3(256), 0, stream, flags, watch_slot, tally, B, N);
    return hipGetLastError();
}

}  // namespace copo
