// Shared declarations of the device evaluation recorder (recorder_kernels.hip) and its C entry points (capi_recorder.hip): the
// per-episode evaluation row of the reference's RecorderEnv (copo/eval/recoder.py:188-349) for E scenes, folded on the device from the
// sampler's [T][E][N] tensors.  The rules are include/copo_hip.h (copo_recorder_*) and DESIGN.md section 8j.
//
// ORDER OF EVERY SUM OVER SLOTS (one fixed tree, nothing else): lane l adds the values of its slots l, l + 64, l + 128, ... in
// ascending order onto +0.0 (a slot that does not take part adds +0.0); then six butterfly stages over the wave at lane distances 32,
// 16, 8, 4, 2, 1, each `v = v + v[lane ^ d]` (commutative, so every lane ends with the same bits).  Minima and maxima take the same
// walk.  Counts are popcounts of ballots.  All fp64, no floating-point atomic, nothing depends on scheduling -- and a step's result does
// not depend on which fragment carried it, so the rows do not depend on how a stream of steps is cut into fragments.
// tests/recorder_numpy.py restates the tree.
//
// ROW IDS come from the row logs' assign rule (rowlog::assign over RowPoolArgs: scene order, ids from max_rows on dropped, the
// counters {rows, dropped}); only the ids and counters are shared.  The pool itself is local: these rows are REC_NCOL fp64 values,
// rowlog_common.h's `row()` and RowPoolArgs::pool are 16 32-bit words, so RowPoolArgs::pool stays NULL here and `rows` below is the pool.
#pragma once
#include "rowlog_common.h"

namespace copo {

constexpr int REC_SLOTS_PER_LANE = 4;                      // lanes stride over the slots when N > 64
constexpr int REC_MAX_SLOTS = 64 * REC_SLOTS_PER_LANE;
// per scene, [E][REC_ACC] fp64: VecRecorder.acc in its order, then the SVO estimate (recoder.py:326-347)
enum { RA_STEPS = 0, RA_VSTEPS, RA_VSUM, RA_VMIN, RA_VMAX, RA_NSTEPS, RA_NSUM, RA_NMAX, RA_AGENTS, RA_SUCC, RA_CRASH, RA_OUT, RA_RSUM,
       RA_RMIN, RA_RMAX, RA_CSUM, RA_CMIN, RA_CMAX, RA_LSUM, RA_SLSUM, RA_SVO_N, RA_SVO_SUM, RA_SVO_MIN, RA_SVO_MAX, RA_SVO_REW, REC_ACC };
// per slot, [REC_SLOT_PLANES][E][N] fp64: the current occupant's cost, own-reward and neighbour-reward sums
enum { RS_COST = 0, RS_OWN, RS_NEI, REC_SLOT_PLANES };
constexpr int REC_COLUMNS = 29;                            // vec_recorder.COLUMNS + the four SVO columns
constexpr int REC_NCOL = REC_COLUMNS + 2;                  // + scene, + episode index of the scene

// Arguments of one call (passed by value).  Device pointers; the five inputs are the sampler's own tensors and are only read.
struct RecorderArgs {
    const uint8_t* flags;          // [T][E][N]
    const float* infos;            // [T][E][N][COPO_INFO_DIM], 16-byte aligned
    const float *rew, *nei_rew;    // [T][E][N]
    const int32_t* nbr_cnt;        // [T][E][N]
    int32_t T, E, N;
    int32_t limit;                 // steps of a scene that has finished `limit` episodes are ignored; 0 = none
    double* acc;                   // [E][REC_ACC]
    double* slots;                 // [REC_SLOT_PLANES][E][N]
    long long* episodes;           // [E] finished episodes
    // between the launches of one call
    int32_t* n_rows;               // [E] rows the scene emits in this fragment
    RowPoolArgs ids;               // max_rows, base and counters; `pool` is NULL
    double* rows;                  // [max_rows][REC_NCOL]
};

hipError_t launch_recorder_add(const RecorderArgs& a, hipStream_t stream);
// every accumulator of every scene back to its start value (0, +inf for the minima, -inf for the maxima)
hipError_t launch_recorder_arm(double* acc, int32_t E, hipStream_t stream);

}  // namespace copo
