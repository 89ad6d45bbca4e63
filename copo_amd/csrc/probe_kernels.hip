// Linear probes of the hidden layers (copo_probe_targets, copo_probe_accumulate; eval/probes.py): the sufficient
// statistics of ridge regressions from a layer's activations to eight scene quantities, over the rows a seated evaluation visits, split
// into a train and a test fold by scene.
// ------------------------------------------------------------------------------------------------------------
// probe_targets_kernel, one launch per env step behind the simulator step, one wave per position p < count of the common row list.  From
// the observation row the policy read, the step's flags and the step's individual reward it writes targets[p][0..16) (eight targets,
// seven zeros, 1.0) and xobs[p][0..Op) (the row, zero beyond O).  The lanes walk the beams in ascending order and are folded by an xor
// butterfly whose every step is a total order (value, then beam index) or an integer sum: the result does not depend on the order, and
// two launches give the same bits.  cos / sin of the nearest beam come from the host's table, never from the device.
// probe_gram_kernel, one launch per env step and feature workspace.  With x_b[p] the D features of block b at position p and the positions
// COUNTED in fold f (gram_common.h, with the fold term):
//     G[f,b][i][j] += sum_p x_b[p][i] x_b[p][j]   (64 x 64 tiles ti <= tj)      C[f,b][i][c] += sum_p x_b[p][i] t[p][c]      T[f][c][d] += sum_p t[p][c] t[p][d]
// Grid: (nt (nt + 1) / 2 + 1) x B x (2 folds * R planes), nt = D / 64, 256 threads.  Workgroup x < nt (nt + 1) / 2 owns the upper tile
// (ti, tj) of G[f,b] in plane r and is gram_tile (gram_common.h: the chunk walk, the staging, the matrix-core loop and the promotion to
// float64 are described there) with both operands taken from one block and no riders.  The last workgroup x of a block owns C[f,b], the
// 16-wide target panel as one more tile column: wave w holds rows 64 t + 16 w .. + 15 of every tile t as nt accumulators, operands
// straight from memory (16 lanes on 64 consecutive bytes of one position); the one of block 0 owns T[f] as well, in wave 0.  It walks
// the tile's chunks in the tile's order, promotes at the tile's interval and masks the operand as the tile does.  A block whose base does
// not fit the workspace adds nothing.
#include "probe_common.h"
#include "gram_common.h"

namespace copo {

__global__ __launch_bounds__(256) void probe_targets_kernel(ProbeTargetArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t count = gram_count(a.count, a.cap);
    if (p >= count) return;      // (uniform over the wave)
    const int64_t row = a.rows[p];
    if (row < 0 || row >= a.n_out) return;
    const float* o = a.obs + (size_t)row * a.O;
    const int n = a.num_lasers;
    float best = INFINITY, front = INFINITY;
    int at = 0x7fffffff, hits = 0;
    for (int k = lane; k < n; k += 64) {
        const float v = o[a.lidar_lo + k];
        if (v < best) {      // (ascending k: the lowest beam of a tie stays)
            best = v;
            at = k;
        }
        hits += v < 1.0f ? 1 : 0;
        if (((k + n / 8) % n) * 4 / n == 0 && v < front) front = v;      // the front quadrant: within n / 8 of beam 0 on either side
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float ob = __shfl_xor(best, off), of = __shfl_xor(front, off);
        const int oa = __shfl_xor(at, off);
        if (ob < best || (ob == best && oa < at)) {
            best = ob;
            at = oa;
        }
        hits += __shfl_xor(hits, off);
        if (of < front) front = of;
    }
    const bool any = hits > 0;      // some beam below 1.0: `at` names a beam
    const float nearest = any ? best : 1.0f, reach = 1.0f - nearest;
    const uint8_t fl = a.flags[row];
    float v = 0.0f;
    switch (lane) {
        case 0: v = nearest; break;
        case 1: v = any ? reach * a.trig[2 * at] : 0.0f; break;
        case 2: v = any ? reach * a.trig[2 * at + 1] : 0.0f; break;
        case 3: v = (float)hits / (float)n; break;
        case 4: v = front < 1.0f ? front : 1.0f; break;
        case 5: v = a.reward[row]; break;
        case 6: v = (fl & COPO_F_CRASH) ? 1.0f : 0.0f; break;
        case 7: v = (fl & COPO_F_DONE) ? 1.0f : 0.0f; break;
        case PROBE_PANEL - 1: v = 1.0f; break;
        default: break;
    }
    if (lane < PROBE_PANEL) a.targets[(size_t)p * PROBE_PANEL + lane] = v;
    for (int c = lane; c < a.Op; c += 64) a.xobs[(size_t)p * a.Op + c] = c < a.O ? o[c] : 0.0f;
}

typedef GramMask<true> ProbeMask;

// the workgroup of the target panel: C[f,b] = X_b^T t of this plane's chunks, and T[f] = t^T t where own_T
__device__ __forceinline__ void probe_panel(const ProbeArgs a, const ProbeMask mask, const float* xb, bool valid, bool own_T, int plane, int64_t n_chunks,
                                            double* C, double* T) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 15, lj = lane >> 4;
    const int nt = valid ? a.D / GRAM_TILE : 0;
    gram_v4f acc[PROBE_MAX_TILES], acct = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < PROBE_MAX_TILES; ++t) acc[t] = gram_v4f{0.f, 0.f, 0.f, 0.f};
    C += (size_t)(16 * wave + 4 * lj) * PROBE_PANEL + ln;
    T += (size_t)(4 * lj) * PROBE_PANEL + ln;
    auto promote = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < PROBE_MAX_TILES; ++t) {
            if (t < nt) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    double* at = C + (size_t)(GRAM_TILE * t + rr) * PROBE_PANEL;
                    *at = *at + (double)acc[t][rr];
                }
            }
            acc[t] = gram_v4f{0.f, 0.f, 0.f, 0.f};
        }
        if (own_T && wave == 0) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) T[rr * PROBE_PANEL] = T[rr * PROBE_PANEL] + (double)acct[rr];
        }
        acct = gram_v4f{0.f, 0.f, 0.f, 0.f};
    };
    int since = 0;
    for (int64_t c = plane; c < n_chunks; c += a.R) {
        const unsigned long long bits = __ballot(lane < GRAM_CHUNK && gram_counted(mask, c * GRAM_CHUNK + lane));      // the chunk's counted positions
#pragma unroll 2
        for (int ks = 0; ks < GRAM_CHUNK / 4; ++ks) {
            const bool ok = (bits >> (4 * ks + lj)) & 1;
            const size_t p = ok ? (size_t)(c * GRAM_CHUNK + 4 * ks + lj) : 0;
            const float tl = a.targets[p * PROBE_PANEL + ln], tv = ok ? tl : 0.f;      // the operand is masked, not the product
#pragma unroll
            for (int t = 0; t < PROBE_MAX_TILES; ++t) {
                if (t < nt) {
                    const float xl = xb[p * a.pos_stride + GRAM_TILE * t + 16 * wave + ln];
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? xl : 0.f, tv, acc[t], 0, 0, 0);
                }
            }
            if (own_T && wave == 0) acct = __builtin_amdgcn_mfma_f32_16x16x4f32(tv, tv, acct, 0, 0, 0);
        }
        if (++since == GRAM_PROMOTE_CHUNKS) {
            promote();
            since = 0;
        }
    }
    if (since) promote();
}

__global__ __launch_bounds__(256) void probe_gram_kernel(ProbeArgs a) {
    const int D = a.D, nt = D / GRAM_TILE, n_upper = nt * (nt + 1) / 2, B = a.B, R = a.R;
    const int b = blockIdx.y, f = blockIdx.z / R, plane = blockIdx.z - f * R;
    const int64_t count = gram_count(a.count, a.cap), n_chunks = gram_chunks(count);
    if (plane >= n_chunks) return;      // (uniform over the workgroup: this plane has no chunk in this launch)
    const ProbeMask mask{a.rows, a.flags, a.seat, a.fold, count, a.n_out, a.slots, a.rows_of, f};
    const int64_t base = a.block_base[b];
    // (uniform) a block must lie inside the workspace with all its cap positions, on a 16-byte boundary
    const bool valid = base >= 0 && (base & 3) == 0 && base + (a.cap - 1) * a.pos_stride + D <= a.x_floats;
    const size_t slab = ((size_t)plane * 2 + f) * B + b;
    if ((int)blockIdx.x == n_upper) {
        const bool own_T = b == 0;
        if (!valid && !own_T) return;
        probe_panel(a, mask, a.x + (valid ? base : 0), valid, own_T, plane, n_chunks, a.C + slab * D * PROBE_PANEL,
                    a.T + ((size_t)plane * 2 + f) * PROBE_PANEL * PROBE_PANEL);
        return;
    }
    if (!valid) return;
    int ti, tj;
    gram_upper(blockIdx.x, nt, ti, tj);
    gram_tile<false>(a.x + base + GRAM_TILE * ti, a.x + base + GRAM_TILE * tj, (size_t)a.pos_stride, mask, plane, R,
                     a.G + slab * D * D + (size_t)(GRAM_TILE * ti) * D + GRAM_TILE * tj, (size_t)D);
}

hipError_t launch_probe_targets(const ProbeTargetArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(probe_targets_kernel, dim3((unsigned)((a.cap + 3) / 4)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_probe_accumulate(const ProbeArgs& a, hipStream_t stream) {
    const int nt = a.D / GRAM_TILE;
    hipLaunchKernelGGL(probe_gram_kernel, dim3(nt * (nt + 1) / 2 + 1, a.B, 2 * a.R), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace copo
