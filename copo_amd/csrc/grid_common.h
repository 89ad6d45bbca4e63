// What the observers over a grid of cells per scene share (field_kernels.hip, encroach_kernels.hip; the scene groups also
// gate_kernels.hip): the grid, the footprint rule and the routing of a scene into its scene group.  DESIGN.md section 8e.
#pragma once
#include "sim_math.h"

namespace copo {

constexpr int GRID_MAX_SIDE = 1024, GRID_MAX_GROUPS = 64;      // cells per side, scene groups

// cells [lo, hi] of an axis of n cells that a footprint around coordinate f (in cells) can reach, r cells to either side
__device__ __forceinline__ bool reach(float f, float r, int n, int& lo, int& hi) {
    const float a = floorf(f - r), b = floorf(f + r);
    if (!(b >= 0.0f) || !(a < (float)n)) return false;      // (NaN reaches nothing)
    lo = (int)fmaxf(a, 0.0f);
    hi = (int)fminf(b, (float)(n - 1));
    return true;
}

// W x H cells of `cell` metres with the origin (x0, y0); cell (ix, iy) is iy * W + ix
struct GridSpec {
    float x0, y0, cell, inv_cell;  // inv_cell = 1 / cell, rounded once to fp32 on the host
    int32_t W, H;
    // the cell that holds (x, y), -1 outside the grid: subtraction, product and floor rounded one by one
    __device__ __forceinline__ int cell_of(float x, float y) const {
        const float fx = floorf((x - x0) * inv_cell), fy = floorf((y - y0) * inv_cell);
        if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) return -1;
        return (int)fy * W + (int)fx;
    }
    __device__ __forceinline__ float centre_x(int ix) const { return x0 + ((float)ix + 0.5f) * cell; }      // of column ix / row iy
    __device__ __forceinline__ float centre_y(int iy) const { return y0 + ((float)iy + 0.5f) * cell; }
    // the cells a body at (x, y) can reach, false: none (half its diagonal stays below hl + hw; one cell on top for the cell coordinates' rounding)
    __device__ __forceinline__ bool reach_box(float x, float y, float hl, float hw, int& lox, int& hix, int& loy, int& hiy) const {
        const float r = (hl + hw) * inv_cell + 1.0f;
        return reach((x - x0) * inv_cell, r, W, lox, hix) && reach((y - y0) * inv_cell, r, H, loy, hiy);
    }
};

// THE footprint rule: whether a cell centre at (dx, dy) from the centre of a body with heading vector (cs, sn) lies in the body.  (By
// reference on purpose: by value the tile pass of the field maps measured 8 % slower at 16 384 scenes, 493 against 457 us a record.)
__device__ __forceinline__ bool covers(const float& dx, const float& dy, const float& cs, const float& sn, const float& hl, const float& hw) {
    const float u = fm(dx, cs, dy * sn), w = fm(dy, cs, -(dx * sn));
    return fabsf(u) <= hl && fabsf(w) <= hw;
}

// Scene e adds to scene group group[e], a value outside 0..G-1 to none (the field maps' tile pass, a launch per group, compares group[e] with its g)
struct SceneGroups {
    const int32_t* group;          // [E]
    int32_t G;
    __device__ __forceinline__ int of(int e) const { const int g = group[e]; return (uint32_t)g < (uint32_t)G ? g : -1; }
};

}  // namespace copo
