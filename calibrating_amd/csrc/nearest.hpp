// nearest.hpp -- the bins of the nearest fill and the search of one pixel through them, shared by sparse.hip (every pixel)
// and lidar.hip (the pixels inside the samples' convex hull): one definition, so the two fills cannot drift apart.
#pragma once

#include <cmath>

#include "common.hpp"

namespace camd {

constexpr int SP_MAX_RADIUS = CAMD_NEAREST_MAX_RADIUS;

// A sample (u, v) lies in the integer cell (floor(u), floor(v)).  A pixel x can only be nearer than `distance` <= R to
// samples with x - R < u < x + R, i.e. cells x - R .. x + R - 1 (the float64 difference x - u is monotonic in u and R is
// representable, so rounding cannot move a sample across that bound).  Cells -R .. w + R - 2 therefore serve every pixel
// of a w-wide grid: bins_w = w + 2R - 1, bins_h = h + 2R - 1; samples in no such cell cannot be anybody's answer.
struct SpBins {
    int w, h, R, bw, bh;
};

// The sample nearest to pixel (x, y) of the grid, 0 <= x < w, 0 <= y < h: float32 of its z if its float64 distance
// sqrt(dx * dx + dy * dy) is < distance, else 0; of equal distances the lowest row wins.  The 2R cells of one bin row that
// a pixel needs are adjacent, so each bin row is one contiguous run of sorted samples.  Both loops are bounded by input
// sizes (2R rows, the samples binned into them).  z: the samples' values, z_stride elements apart.
template <typename Z>
__device__ __forceinline__ float sp_nearest_value(const double* __restrict__ sorted_uv, const uint32_t* __restrict__ sorted_idx,
                                                  const uint32_t* __restrict__ start, const Z* __restrict__ z, size_t z_stride,
                                                  const SpBins& b, double distance, int x, int y)
{
    const double px = (double)x, py = (double)y;
    double best = INFINITY;
    uint32_t best_i = 0xffffffffu;
    for (int r = 0; r < 2 * b.R; r++) {
        const size_t row = (size_t)(y + r) * b.bw;  // bin row of cell y - R + r
        const uint32_t s = start[row + x], e = start[row + x + 2 * b.R];
        for (uint32_t k = s; k < e; k++) {
            const double dx = px - sorted_uv[(size_t)k * 2], dy = py - sorted_uv[(size_t)k * 2 + 1];
            const double d = __dsqrt_rn(dx * dx + dy * dy);
            const uint32_t i = sorted_idx[k];
            if (d < best || (d == best && i < best_i)) { best = d; best_i = i; }
        }
    }
    float v = 0.0f;
    if (best < distance) v = (float)z[(size_t)best_i * z_stride];
    return v;
}

static inline int make_bins(SpBins* b, int w, int h, double distance, const char* who)
{
    if (w <= 0 || h <= 0) { set_error("%s: bad grid size %d x %d", who, w, h); return CAMD_ERR_BAD_ARG; }
    if (!(distance == distance) || distance > (double)SP_MAX_RADIUS) {
        set_error("%s: distance %g needs a search window beyond the supported %d cells each way (distance <= %d)", who,
                  distance, SP_MAX_RADIUS, SP_MAX_RADIUS);
        return CAMD_ERR_UNSUPPORTED;
    }
    int R = distance > 1.0 ? (int)ceil(distance) : 1;  // (distance <= 0: nothing is ever nearer, the window may be minimal)
    b->w = w; b->h = h; b->R = R; b->bw = w + 2 * R - 1; b->bh = h + 2 * R - 1;
    if ((unsigned long long)b->bw * (unsigned long long)b->bh >= 0x7fffffffull || h > 65535) {
        set_error("%s: a %d x %d grid is beyond the 32-bit cell index / 65535 rows", who, w, h);
        return CAMD_ERR_UNSUPPORTED;
    }
    return CAMD_OK;
}

}  // namespace camd
