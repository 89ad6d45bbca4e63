// Event clips over the simulator's scenes (copo_clip_*, include/copo_hip.h): a flight recorder on the device.  Every record copies what
// the renderer and the interaction meter read of every scene -- x, y, heading, speed, status byte, agent id per slot, t_env and the
// episode counter per scene -- into that scene's ring of the last pre + post + 1 snapshots and runs the scene's trigger state machine;
// the scenes whose clip is complete receive clip ids in scene order and copy their records out of the ring into a bounded pool.
//   record:  one wave per scene, four scenes per workgroup, lane n = slot n (loads and stores coalesced over the slots); triggers are
//            wave ballots, the state machine is lane 0's
//   assign:  ONE workgroup walks the scenes in order (ballot + prefix count) and hands the ready ones their ids: no atomic decides
//            an id, so which clips exist, their order and which are dropped do not depend on how workgroups are scheduled
//   commit:  one workgroup per scene, gone at once unless the scene is ready
// Copies, integer logic and fp32 `<` only.  The rules are restated in numpy by tests/clip_numpy.py.
#include "sim_device.h"
#include "clip_common.h"

namespace copo {

namespace {

constexpr int SCENES_PER_WG = 4;       // waves of a 256-thread workgroup
constexpr int ASSIGN_THREADS = 1024, ASSIGN_WAVES = ASSIGN_THREADS / 64;

}  // namespace

__global__ __launch_bounds__(256) void clip_record_kernel(ClipArgs a, const uint8_t* __restrict__ flags, const float* __restrict__ ttc,
                                                          const float* __restrict__ gap) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * SCENES_PER_WG + wave;
    if (e >= a.E) return;                      // (the whole wave; there is no barrier in this kernel)
    const int N = a.N;
    const size_t EN = (size_t)a.E * N, o = (size_t)e * N + lane;
    const int r = a.counters[CC_RECORDS];
    const int head = r % a.cap;
    bool fire_f = false, fire_t = false, fire_g = false;
    int32_t aid = 0;
    if (lane < N) {
        const uint32_t* su = reinterpret_cast<const uint32_t*>(a.state);
        uint32_t* R = a.ring + (((size_t)e * a.cap + head) * CLIP_WORDS) * N + lane;
        const uint32_t w0 = su[o], w1 = (su + EN)[o], w2 = (su + 2 * EN)[o], w3 = (su + 3 * EN)[o];
        const uint32_t st = (su + 13 * EN)[o] & 0xffu, id = (su + 14 * EN)[o];
        R[0] = w0; R[N] = w1; R[2 * N] = w2; R[3 * N] = w3; R[4 * N] = st; R[5 * N] = id;
        aid = (int32_t)id;
        if (flags) fire_f = ((uint32_t)flags[o] & a.flag_mask) != 0u;
        if (ttc) fire_t = a.ttc_below > 0.0f && ttc[o] < a.ttc_below;
        if (gap) fire_g = a.gap_below > 0.0f && gap[o] < a.gap_below;
    }
    const unsigned long long mf = __ballot(fire_f), mt = __ballot(fire_t), mg = __ballot(fire_g);
    const unsigned long long m = mf | mt | mg;
    const int slot = m ? __ffsll((long long)m) - 1 : 0;
    const int32_t slot_aid = __shfl(aid, slot);
    if (lane == 0) {
        int32_t* Renv = a.ring_env + ((size_t)e * a.cap + head) * CLIP_ENV_WORDS;
        Renv[0] = a.env[(size_t)e * 4];
        Renv[1] = a.env[(size_t)e * 4 + 1];
        int32_t* S = a.scene + (size_t)e * CLIP_SCENE_WORDS;
        int armed = S[CS_ARMED], countdown = S[CS_COUNTDOWN];
        if (armed) {
            if (m) S[CS_N_EVENTS] += 1;
        } else if (m) {
            armed = 1;
            countdown = a.post;
            S[CS_ARMED] = 1; S[CS_TRIG_REC] = r; S[CS_TRIG_SLOT] = slot; S[CS_TRIG_AID] = slot_aid; S[CS_N_EVENTS] = 1;
            S[CS_KIND] = (mf ? CLIP_KIND_FLAG : 0) | (mt ? CLIP_KIND_TTC : 0) | (mg ? CLIP_KIND_GAP : 0);
        }
        if (armed) {
            if (countdown == 0) a.ready[e] = r + 1;      // (stays armed until the commit kernel of this call has moved the clip)
            else countdown -= 1;
            S[CS_COUNTDOWN] = countdown;
        }
    }
}

// one lane per scene: every armed scene commits with the records it has (an armed scene has at least its trigger record)
__global__ __launch_bounds__(256) void clip_flush_kernel(ClipArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    if (a.scene[(size_t)e * CLIP_SCENE_WORDS + CS_ARMED]) a.ready[e] = a.counters[CC_RECORDS];
}

// ONE workgroup: clip ids of the ready scenes in ascending scene order, then the counters (bump: a record ends here)
__global__ __launch_bounds__(ASSIGN_THREADS) void clip_assign_kernel(ClipArgs a, int bump) {
    __shared__ int wcnt[ASSIGN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = a.counters[CC_CLIPS];      // (read by every thread before the first barrier, written after the last)
    long long total = 0;
    for (int e0 = 0; e0 < a.E; e0 += ASSIGN_THREADS) {
        const int e = e0 + tid;
        const bool rdy = e < a.E && a.ready[e] != 0;
        const unsigned long long m = __ballot(rdy);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = 0, sum = 0;
#pragma unroll
        for (int w = 0; w < ASSIGN_WAVES; ++w) {
            const int c = wcnt[w];
            off += w < wave ? c : 0;
            sum += c;
        }
        if (rdy) {
            const long long id = base + total + off + __popcll(m & ((1ull << lane) - 1ull));
            a.cid[e] = (int32_t)(id < a.max_clips ? id : a.max_clips);      // (every id from max_clips on is dropped alike)
        }
        total += sum;
        __syncthreads();
    }
    if (tid == 0) {
        const long long stored = base + total < a.max_clips ? base + total : a.max_clips;
        a.counters[CC_CLIPS] = (int32_t)stored;
        a.counters[CC_DROPPED] += (int32_t)(base + total - stored);
        if (bump) a.counters[CC_RECORDS] += 1;
    }
}

__global__ __launch_bounds__(256) void clip_commit_kernel(ClipArgs a) {
    const int e = blockIdx.x, tid = threadIdx.x;
    const int rd = a.ready[e];
    if (rd == 0) return;                       // (uniform over the workgroup)
    const int32_t* S = a.scene + (size_t)e * CLIP_SCENE_WORDS;
    const int last = rd - 1, trig = S[CS_TRIG_REC], lo = S[CS_LO];
    const int first = trig - a.pre > lo ? trig - a.pre : lo;
    const int length = last - first + 1;
    const int id = a.cid[e];
    int32_t h[CLIP_HEADER];
    h[CH_SCENE] = e; h[CH_FIRST_REC] = first; h[CH_LENGTH] = length; h[CH_TRIG_REC] = trig; h[CH_TRIG_SLOT] = S[CS_TRIG_SLOT];
    h[CH_KIND] = S[CS_KIND]; h[CH_TRIG_AID] = S[CS_TRIG_AID]; h[CH_N_EVENTS] = S[CS_N_EVENTS];
    if (id < a.max_clips) {
        const int per = CLIP_WORDS * a.N;
        const uint32_t* ring = a.ring + (size_t)e * a.cap * per;
        uint32_t* clip = a.pool + (size_t)id * a.cap * per;
        for (int i = tid; i < length * per; i += blockDim.x) {
            const int k = i / per, j = i - k * per;
            clip[(size_t)k * per + j] = ring[(size_t)((first + k) % a.cap) * per + j];
        }
        for (int i = tid; i < length * CLIP_ENV_WORDS; i += blockDim.x) {
            const int k = i / CLIP_ENV_WORDS, j = i - k * CLIP_ENV_WORDS;
            a.pool_env[((size_t)id * a.cap + k) * CLIP_ENV_WORDS + j] = a.ring_env[((size_t)e * a.cap + (first + k) % a.cap) * CLIP_ENV_WORDS + j];
        }
    }
    __syncthreads();                           // every thread has read the scene's words
    if (tid == 0) {
        if (id < a.max_clips)
            for (int k = 0; k < CLIP_HEADER; ++k) a.header[(size_t)id * CLIP_HEADER + k] = h[k];
        int32_t* Sw = a.scene + (size_t)e * CLIP_SCENE_WORDS;
        Sw[CS_ARMED] = 0;
        Sw[CS_LO] = last + 1;
        a.ready[e] = 0;
    }
}

// playback: one wave per target scene, lane n = slot n
__global__ __launch_bounds__(256) void clip_scatter_kernel(float* __restrict__ state, int32_t* __restrict__ env, int32_t E, int32_t N,
                                                           const uint32_t* __restrict__ snaps, const int32_t* __restrict__ envw, int32_t cap,
                                                           const int32_t* __restrict__ clip_idx, const int32_t* __restrict__ frame_idx,
                                                           int32_t S) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * SCENES_PER_WG + wave;
    if (j >= S) return;
    const int ci = clip_idx[j], fi = frame_idx[j];
    const bool empty = fi < 0 || fi >= cap || ci < 0;      // -1: an all-EMPTY scene (so is anything else out of range)
    const size_t EN = (size_t)E * N, o = (size_t)j * N + lane;
    const size_t f0 = empty ? 0 : (size_t)ci * cap + fi;
    if (lane < N) {
        uint32_t* su = reinterpret_cast<uint32_t*>(state);
        const uint32_t* F = snaps + f0 * CLIP_WORDS * N + lane;
#pragma unroll
        for (int f = 0; f < COPO_STATE_FIELDS; ++f) {
            uint32_t v = 0;
            if (f < 4) v = empty ? 0u : F[(size_t)f * N];
            else if (f == 13) v = empty ? (uint32_t)ST_EMPTY : (F[(size_t)4 * N] & 0xffu);
            else if (f == 14) v = empty ? 0u : F[(size_t)5 * N];
            (su + f * EN)[o] = v;
        }
    }
    if (lane == 0) {
        int32_t* W = env + (size_t)j * 4;
        W[0] = empty ? 0 : envw[f0 * CLIP_ENV_WORDS];
        W[1] = empty ? 0 : envw[f0 * CLIP_ENV_WORDS + 1];
        W[2] = 0;
        W[3] = 1;
    }
}

static hipError_t launch_assign_commit(const ClipArgs& a, int bump, hipStream_t stream) {
    hipLaunchKernelGGL(clip_assign_kernel, dim3(1), dim3(ASSIGN_THREADS), 0, stream, a, bump);
    hipLaunchKernelGGL(clip_commit_kernel, dim3(a.E), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_clip_record(const ClipArgs& a, const uint8_t* flags, const float* ttc, const float* gap, hipStream_t stream) {
    hipLaunchKernelGGL(clip_record_kernel, dim3((a.E + SCENES_PER_WG - 1) / SCENES_PER_WG), dim3(256), 0, stream, a, flags, ttc, gap);
    return launch_assign_commit(a, 1, stream);
}

hipError_t launch_clip_flush(const ClipArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(clip_flush_kernel, dim3((a.E + 255) / 256), dim3(256), 0, stream, a);
    return launch_assign_commit(a, 0, stream);
}

hipError_t launch_clip_scatter(float* state, int32_t* env, int32_t E, int32_t N, const uint32_t* snaps, const int32_t* envw, int32_t cap,
                               const int32_t* clip_idx, const int32_t* frame_idx, int32_t S, hipStream_t stream) {
    hipLaunchKernelGGL(clip_scatter_kernel, dim3((S + SCENES_PER_WG - 1) / SCENES_PER_WG), dim3(256), 0, stream, state, env, E, N, snaps, envw,
                       cap, clip_idx, frame_idx, S);
    return hipGetLastError();
}

}  // namespace copo
