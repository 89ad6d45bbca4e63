// Critic audit (copo_audit_record; eval/critics.py): one step's values V(s_t), rewards and flags folded into the
// forward-view sums of every agent's life, per (scene, slot, head), and a finished agent's sums committed per (scene group, member,
// head).  No trajectory is stored and nothing runs backward: with G_t = sum_{k >= t} gamma^(k - t) r_k up to the agent's last step,
//     sum_t G_t = sum_k r_k c_k,   sum_t V_t G_t = sum_k r_k z_k,   sum_t G_t^2 = sum_k r_k (r_k q_k + 2 gamma u_(k-1)),
//     sum_{t in bin b} G_t = sum_k r_k e_(b,k)
// with c_k = sum_{t <= k} gamma^(k - t), z_k = sum_{t <= k} gamma^(k - t) V_t, q_k = sum_{t <= k} gamma^(2 (k - t)),
// u_k = sum_{t <= k} gamma^(k - t) G_t^(k) (the returns as far as step k knows them) and e_(b,k) = sum_{t <= k, t in b} gamma^(k - t),
// each one multiply-add per step.  tests/critic_numpy.py proves the identity against the backward recursion.
// One thread per (scene, slot, head); its state is 10 + 4 bins float64 words, plane-major, so a wave reads and writes whole lines.  The
// updates of a thread touch its own words only; a commit quantises each sum once (2^-16 steps, round to nearest even, clamped: see
// audit_common.h) and adds it with a 64-bit integer atomic, so the accumulator does not depend on the order the device runs in.
// Every operation is individually rounded float64 (the unit is compiled without contraction), in the order the header states.
#include "audit_common.h"

namespace copo {

__device__ __forceinline__ int64_t audit_q(double x) {
    if (x != x) return 0;
    return (int64_t)llrint(fmin(fmax(x, -AUDIT_CLAMP), AUDIT_CLAMP) * AUDIT_Q);
}

__device__ __forceinline__ void audit_add(int64_t* cell, int w, int64_t v) {
    if (v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(cell) + w, (unsigned long long)v);
}

__global__ void __launch_bounds__(256) audit_record_kernel(AuditArgs a) {
    const size_t total = (size_t)a.E * a.N * a.heads;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int h = (int)(i % a.heads);
    const size_t row = i / a.heads;                 // e N + n
    const int e = (int)(row / a.N);
    const int g = a.group[e], m = a.seat[row];
    if (g < 0 || g >= a.G || m < 0 || m >= a.K) return;      // nobody's seat, or a scene outside the groups: not audited
    const uint32_t f = a.flags[row];
    const bool acted = (f & COPO_F_ACTED) != 0u, done = acted && (f & COPO_F_DONE) != 0u;
    const bool leaves = (f & (COPO_F_DONE | COPO_F_SPAWNED | COPO_F_ENV_RESET)) != 0u;
    if (!acted && !leaves) return;
    const int B = a.bins;
    double* st = a.state + i;
    auto S = [&](int plane) -> double& { return st[(size_t)plane * total]; };
    if (acted) {
        const double gam = a.gamma[h], V = (double)a.values[i];
        const double r = h == 2 ? (double)a.glob_rew[e] : (double)a.rew[h][row];
        const double t = (V - a.lo[h]) / (a.hi[h] - a.lo[h]) * (double)B;
        const int bin = !(t >= 0.0) ? 0 : (t >= (double)B ? B - 1 : (int)t);      // (NaN lands in bin 0)
        const double q = gam * gam * S(AS_Q) + 1.0;
        const double c = gam * S(AS_C) + 1.0;
        const double z = gam * S(AS_Z) + V;
        const double u0 = S(AS_U);
        S(AS_Q) = q; S(AS_C) = c; S(AS_Z) = z;
        S(AS_SV) += V;
        S(AS_SVV) += V * V;
        S(AS_N) += 1.0;
        S(AS_SG) += r * c;
        S(AS_SVG) += r * z;
        S(AS_SGG) += r * (r * q + 2.0 * gam * u0);
        S(AS_U) = gam * u0 + r * q;
        for (int b = 0; b < B; ++b) {
            const double hit = b == bin ? 1.0 : 0.0;
            const double eb = gam * S(AS_SCALARS + b) + hit;
            S(AS_SCALARS + b) = eb;
            S(AS_SCALARS + B + b) += hit;
            S(AS_SCALARS + 2 * B + b) += V * hit;
            S(AS_SCALARS + 3 * B + b) += r * eb;
        }
    }
    if (done) {
        // by the max-step flag alone: truncated, not terminated -- its returns stop short, so its sums count only on request
        const bool truncated = (f & COPO_F_MAXSTEP) != 0u && (f & (COPO_F_ARRIVE | COPO_F_CRASH | COPO_F_OUT)) == 0u;
        int64_t* cell = a.acc + (((size_t)g * a.K + m) * a.heads + h) * AUDIT_WORDS;
        if (truncated) audit_add(cell, COPO_AUDIT_TRUNCATED, 1);
        if (!truncated || a.count_truncated) {
            audit_add(cell, COPO_AUDIT_AGENTS, 1);
            audit_add(cell, COPO_AUDIT_STEPS, (int64_t)S(AS_N));
            audit_add(cell, COPO_AUDIT_SUM_V, audit_q(S(AS_SV)));
            audit_add(cell, COPO_AUDIT_SUM_VV, audit_q(S(AS_SVV)));
            audit_add(cell, COPO_AUDIT_SUM_G, audit_q(S(AS_SG)));
            audit_add(cell, COPO_AUDIT_SUM_VG, audit_q(S(AS_SVG)));
            audit_add(cell, COPO_AUDIT_SUM_GG, audit_q(S(AS_SGG)));
            for (int b = 0; b < B; ++b) {
                audit_add(cell, COPO_AUDIT_BIN_COUNT + b, (int64_t)S(AS_SCALARS + B + b));
                audit_add(cell, COPO_AUDIT_BIN_VALUE + b, audit_q(S(AS_SCALARS + 2 * B + b)));
                audit_add(cell, COPO_AUDIT_BIN_RETURN + b, audit_q(S(AS_SCALARS + 3 * B + b)));
            }
        }
    }
    if (leaves) {      // the next occupant starts from zero; an agent the scene's reset took away is not counted
        const int planes = AS_SCALARS + 4 * B;
        for (int p = 0; p < planes; ++p) S(p) = 0.0;
    }
}

hipError_t launch_audit_record(const AuditArgs& a, hipStream_t stream) {
    const size_t total = (size_t)a.E * a.N * a.heads;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(audit_record_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace copo
