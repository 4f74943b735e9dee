// hull_common.hpp -- what hull.hip (the plane inside the hull) and lidar.hip (the nearest sample inside the hull) share of
// the mask contract: the status bits, the bound of a rounded pixel, and the closed span of an image row inside a hull.
#pragma once

#include <climits>

#include "common.hpp"

namespace camd {

enum { HULL_NO_SAMPLE = 1, HULL_DEGENERATE = 2, HULL_OUT_OF_RANGE = 4 };
constexpr int HULL_MAX_POINTS = CAMD_HULL_MAX_POINTS;
constexpr double HULL_MAX_COORD = 1048576.;    // 2^20: differences fit 22 bits, their products 43: all int64

__device__ __forceinline__ long long floor_div(long long a, long long b)  // b > 0
{
    const long long q = a / b;
    return q * b > a ? q - 1 : q;
}
__device__ __forceinline__ long long ceil_div(long long a, long long b)  // b > 0
{
    const long long q = a / b;
    return q * b < a ? q + 1 : q;
}

// The closed span [xl, xr] of row y inside the hull, clipped to [0, w - 1]; xl > xr: the row is empty.  The line y = const
// meets a convex polygon in one segment: its ends are the lowest and the highest crossing with an edge that reaches the
// row, so xl = min over those edges of ceil(crossing), xr = max of floor(crossing).  An edge along the row gives both its
// ends.  One vertex is the edge from itself to itself.  Wave-cooperative: the edges are lane-strided and meet in a
// butterfly, so EVERY lane of the wave must call it; the same span in every lane.
__device__ __forceinline__ void hull_span(const int* __restrict__ verts, int count, int y, int w, int lane, int* xl, int* xr)
{
    long long lo = LLONG_MAX, hi = LLONG_MIN;
    for (int k = lane; k < count; k += 64) {
        const int k2 = k + 1 < count ? k + 1 : 0;
        const long long ax = verts[k * 2], ay = verts[k * 2 + 1], bx = verts[k2 * 2], by = verts[k2 * 2 + 1];
        if ((y < ay && y < by) || (y > ay && y > by)) continue;
        if (ay == by) {
            lo = min(lo, min(ax, bx)), hi = max(hi, max(ax, bx));
            continue;
        }
        long long den = by - ay, num = ax * den + ((long long)y - ay) * (bx - ax);  // crossing = num / den
        if (den < 0) den = -den, num = -num;
        lo = min(lo, ceil_div(num, den)), hi = max(hi, floor_div(num, den));
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        lo = min(lo, (long long)__shfl_xor(lo, m, 64));
        hi = max(hi, (long long)__shfl_xor(hi, m, 64));
    }
    lo = max(lo, 0ll), hi = min(hi, (long long)w - 1);
    if (lo > hi) lo = 1, hi = 0;
    *xl = (int)lo, *xr = (int)hi;
}

}  // namespace camd
