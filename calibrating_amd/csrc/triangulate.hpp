// triangulate.hpp -- the per-match solve shared by camd_matched_uvs_to_zs (sparse.hip) and camd_epipolar_sums
// (epipolar.hip): one __device__ function, so a match that is solved again under the same pose gives the same bits.
#pragma once

#include "common.hpp"

namespace camd {

// a * b - c * d with the rounding error of c * d carried along (Kahan): exact to ~1.5 ulp without cancellation loss
__device__ __forceinline__ double diff_of_products(double a, double b, double c, double d)
{
    const double w = c * d;
    const double e = __fma_rn(-c, d, w);
    const double f = __fma_rn(a, b, -w);
    return f + e;
}
__device__ __forceinline__ void cross3(const double* p, const double* q, double* r)
{
    r[0] = diff_of_products(p[1], q[2], p[2], q[1]);
    r[1] = diff_of_products(p[2], q[0], p[0], q[2]);
    r[2] = diff_of_products(p[0], q[1], p[1], q[0]);
}

// X = Kinv (u, v, 1) for both pixels of a match
__device__ __forceinline__ void tri_rays(const double* k1, const double* k2, double u1, double v1, double u2, double v2,
                                         double* x1, double* b)
{
    for (int r = 0; r < 3; r++) {
        x1[r] = __fma_rn(k1[r * 3 + 2], 1.0, __fma_rn(k1[r * 3 + 1], v1, k1[r * 3] * u1));
        b[r] = __fma_rn(k2[r * 3 + 2], 1.0, __fma_rn(k2[r * 3 + 1], v2, k2[r * 3] * u2));
    }
}

// X2 z2 = R X1 z1 + t  ->  [a, b] (z1, z2)^T = t with a = -R X1, b = X2.  The 2x2 normal equations
//   (a.a) z1 + (a.b) z2 = a.t,  (a.b) z1 + (b.b) z2 = b.t
// have, by Lagrange's identity, the closed form z1 = (a x b).(t x b) / |a x b|^2, z2 = (a x b).(a x t) / |a x b|^2.
// That form is evaluated: for the near-parallel rays of a stereo rig the determinant (a.a)(b.b) - (a.b)^2 loses
// sin^-2 of the angle between the rays in digits, the cross product only sin^-1.
__device__ __forceinline__ void tri_solve(const double* x1, const double* b, const double* R, const double* t, double* z1,
                                          double* z2)
{
    double a[3], axb[3], txb[3], axt[3];
    for (int r = 0; r < 3; r++)
        a[r] = -__fma_rn(R[r * 3 + 2], x1[2], __fma_rn(R[r * 3 + 1], x1[1], R[r * 3] * x1[0]));
    cross3(a, b, axb);
    cross3(t, b, txb);
    cross3(a, t, axt);
    const double den = __fma_rn(axb[2], axb[2], __fma_rn(axb[1], axb[1], axb[0] * axb[0]));
    *z1 = __fma_rn(axb[2], txb[2], __fma_rn(axb[1], txb[1], axb[0] * txb[0])) / den;
    *z2 = __fma_rn(axb[2], axt[2], __fma_rn(axb[1], axt[1], axb[0] * axt[0])) / den;
}

}  // namespace camd
