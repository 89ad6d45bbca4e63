// Critic audit (copo_audit_*, include/copo_hip.h): the layouts of the per-slot state and of the accumulator, and
// the launcher that audit_kernels.hip defines and capi_audit.hip checks arguments for.  The rules are restated as python loops by
// tests/critic_numpy.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/copo_hip.h"

namespace copo {

// accumulator words of one (group, member, head) cell: COPO_AUDIT_* of the header, then three planes of COPO_AUDIT_MAX_BINS
constexpr int AUDIT_WORDS = COPO_AUDIT_WORDS, AUDIT_MAX_BINS = COPO_AUDIT_MAX_BINS;
static_assert(AUDIT_WORDS == COPO_AUDIT_BIN_COUNT + 3 * AUDIT_MAX_BINS && COPO_AUDIT_BIN_VALUE == COPO_AUDIT_BIN_COUNT + AUDIT_MAX_BINS &&
              COPO_AUDIT_BIN_RETURN == COPO_AUDIT_BIN_VALUE + AUDIT_MAX_BINS, "copo_hip.h: the three bin planes follow the eight scalars");

// state planes of one (scene, slot, head), float64, plane-major ([plane][E N heads]): ten scalars, then four planes per bin
enum { AS_Q, AS_C, AS_Z, AS_U, AS_SV, AS_SVV, AS_SG, AS_SVG, AS_SGG, AS_N, AS_SCALARS };
inline int audit_state_planes(int bins) { return AS_SCALARS + 4 * bins; }

// One agent's sums are clamped to +-AUDIT_CLAMP before they are quantised to 2^-16 steps: |word| <= 2^48 per agent, so 2^15 agents at
// the clamp fit an int64 cell; at the magnitudes of the simulator's rewards (a thousand steps of returns near a hundred: sums of
// squares near 1e7) a cell holds some 1e7 agents.
constexpr double AUDIT_CLAMP = 4294967296.0, AUDIT_Q = 65536.0;

struct AuditArgs {
    const uint8_t* flags;     // [E][N]
    const float* values;      // [E N][heads]
    const float* rew[2];      // [E][N]: head 0, head 1
    const float* glob_rew;    // [E]: head 2
    const int32_t* seat;      // [E][N]
    const int32_t* group;     // [E]
    int32_t E, N, K, G, heads, bins, count_truncated;
    double gamma[3], lo[3], hi[3];
    double* state;            // [planes][E N heads]
    int64_t* acc;             // [G][K][heads][AUDIT_WORDS]
};

hipError_t launch_audit_record(const AuditArgs& a, hipStream_t stream);

}  // namespace copo
