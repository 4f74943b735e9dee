// camera_model.hpp -- cv2's pinhole + distortion model, stated once for tables.hip, distort.hip and points.hip.
//
// Two forward forms, because cv2's two call sites order the polynomial differently and every bit matters (a one-ulp
// difference moves a pixel across a truncation border): distort_forward is cv2.projectPoints (powers
// r2, r4, r6 and a reciprocal; U22 / U24), distort_horner is cv2.initUndistortRectifyMap (Horner chains and a quotient).
// The iteration of cv2.undistortPoints (U23) is a third order: undistort_iterate, for points.hip and the start pose of pnp.hip.
// distort_forward_jacobian is the analytic derivative of distort_forward, for the Levenberg-Marquardt of pnp.hip.
#pragma once

#include <cmath>

#include "common.hpp"

namespace camd {

struct Lens { double k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4; };
struct Pinhole { double fx, fy, cx, cy, ifx, ify; };  // ifx = 1. / fx, ify = 1. / fy (cv2 multiplies by the reciprocal)

// K and dist[0 .. ndist) (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tauX tauY, the missing ones 0) -> cam, lens.  Which ndist an
// entry point takes is its own rule, checked before it comes here together with the pointers.  CAMD_OK, or
// CAMD_ERR_UNSUPPORTED with the message set for a tilted sensor.
inline int unpack_camera(const char* who, const double K[9], const double* dist, int ndist, Pinhole* cam, Lens* lens)
{
    double dv[14] = {0};
    for (int i = 0; i < ndist; i++) dv[i] = dist[i];
    if (dv[12] != 0. || dv[13] != 0.) {
        set_error("%s: tilted-sensor distortion (tauX, tauY) not implemented", who);
        return CAMD_ERR_UNSUPPORTED;
    }
    *cam = {K[0], K[4], K[2], K[5], 1. / K[0], 1. / K[4]};
    *lens = {dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], dv[6], dv[7], dv[8], dv[9], dv[10], dv[11]};
    return CAMD_OK;
}

// cv2.projectPoints on a normalised point (cvProjectPoints2Internal)
__device__ __forceinline__ void distort_forward(const Lens& k, double x, double y, double& xd, double& yd)
{
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
    const double cdist = 1 + k.k1 * r2 + k.k2 * r4 + k.k3 * r6;
    const double icdist2 = __ddiv_rn(1., 1 + k.k4 * r2 + k.k5 * r4 + k.k6 * r6);
    xd = x * cdist * icdist2 + k.p1 * a1 + k.p2 * a2 + k.s1 * r2 + k.s2 * r4;
    yd = y * cdist * icdist2 + k.p1 * a3 + k.p2 * a1 + k.s3 * r2 + k.s4 * r4;
}

// d(xd, yd) / d(x, y) of distort_forward, row-major {dxd/dx, dxd/dy, dyd/dx, dyd/dy}: the chain rule through r2 on the
// same polynomial (q = cdist * icdist2; dq/dr2 = (cdist' - q * den') * icdist2)
__device__ __forceinline__ void distort_forward_jacobian(const Lens& k, double x, double y, double j[4])
{
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double cdist = 1 + k.k1 * r2 + k.k2 * r4 + k.k3 * r6;
    const double icdist2 = __ddiv_rn(1., 1 + k.k4 * r2 + k.k5 * r4 + k.k6 * r6);
    const double q = cdist * icdist2;
    const double dq = ((k.k1 + 2 * k.k2 * r2 + 3 * k.k3 * r4) - q * (k.k4 + 2 * k.k5 * r2 + 3 * k.k6 * r4)) * icdist2;
    const double gx = 2 * x * dq, gy = 2 * y * dq;  // dq/dx, dq/dy
    j[0] = q + x * gx + 2 * k.p1 * y + 6 * k.p2 * x + 2 * k.s1 * x + 4 * k.s2 * r2 * x;
    j[1] = x * gy + 2 * k.p1 * x + 2 * k.p2 * y + 2 * k.s1 * y + 4 * k.s2 * r2 * y;
    j[2] = y * gx + 2 * k.p1 * x + 2 * k.p2 * y + 2 * k.s3 * x + 4 * k.s4 * r2 * x;
    j[3] = q + y * gy + 6 * k.p1 * y + 2 * k.p2 * x + 2 * k.s3 * y + 4 * k.s4 * r2 * y;
}

// cv2.undistortPoints' fixed-point iteration from the normalised raw point (xs, ys): `iters` rounds, the same trip count
// for every lane -- a lane that met icdist < 0 keeps its start value through selects
__device__ __forceinline__ void undistort_iterate(const Lens& k, double xs, double ys, int iters, double& x, double& y)
{
    x = xs, y = ys;
    bool done = false;
    for (int j = 0; j < iters; j++) {
        const double r2 = x * x + y * y;
        const double icdist = __ddiv_rn(1 + ((k.k6 * r2 + k.k5) * r2 + k.k4) * r2, 1 + ((k.k3 * r2 + k.k2) * r2 + k.k1) * r2);
        const double dX = 2 * k.p1 * x * y + k.p2 * (r2 + 2 * x * x) + k.s1 * r2 + k.s2 * r2 * r2;
        const double dY = k.p1 * (r2 + 2 * y * y) + 2 * k.p2 * x * y + k.s3 * r2 + k.s4 * r2 * r2;
        const bool neg = icdist < 0;
        const double xn = neg ? xs : (xs - dX) * icdist, yn = neg ? ys : (ys - dY) * icdist;
        x = done ? x : xn;
        y = done ? y : yn;
        done = done || neg;
    }
}

// cv2.initUndistortRectifyMap on a normalised point
__host__ __device__ inline void distort_horner(const Lens& k, double x, double y, double& xd, double& yd)
{
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, _2xy = 2 * x * y;
    const double kr = (1 + ((k.k3 * r2 + k.k2) * r2 + k.k1) * r2) / (1 + ((k.k6 * r2 + k.k5) * r2 + k.k4) * r2);
    xd = (x * kr + k.p1 * _2xy + k.p2 * (r2 + 2 * x2) + k.s1 * r2 + k.s2 * r2 * r2);
    yd = (y * kr + k.p1 * (r2 + 2 * y2) + k.p2 * _2xy + k.s3 * r2 + k.s4 * r2 * r2);
}

// the ray (X, Y, W) of a destination pixel -> where it reads the source image: initUndistortRectifyMap's loop body
__host__ __device__ inline void ray_to_pixel(const Pinhole& c, const Lens& k, double X, double Y, double W, double& u, double& v)
{
    const double ww = 1. / W;
    double xd, yd;
    distort_horner(k, X * ww, Y * ww, xd, yd);
    u = c.fx * xd + c.cx, v = c.fy * yd + c.cy;
}

// the same as cv2.undistort's CV_16SC2 cell + CV_16UC1 phase: cvRound(u * INTER_TAB_SIZE), half to even
__host__ __device__ inline void ray_to_fixed_cell(const Pinhole& c, const Lens& k, double X, double Y, double W, int16_t* xy,
                                                  uint16_t* phase)
{
    double u, v;
    ray_to_pixel(c, k, X, Y, W, u, v);
#ifdef __HIP_DEVICE_COMPILE__
    const int iu = (int)rint(u * INTER_TAB_SIZE), iv = (int)rint(v * INTER_TAB_SIZE);
#else
    const int iu = (int)lrint(u * INTER_TAB_SIZE), iv = (int)lrint(v * INTER_TAB_SIZE);
#endif
    xy[0] = (int16_t)(iu >> INTER_BITS);
    xy[1] = (int16_t)(iv >> INTER_BITS);
    *phase = (uint16_t)((iv & (INTER_TAB_SIZE - 1)) * INTER_TAB_SIZE + (iu & (INTER_TAB_SIZE - 1)));
}

// 3x3 inverse through the adjugate, row-major (all zeros for a singular matrix)
__host__ __device__ inline void inv3(const double* m, double* o)
{
    double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
               m[2] * (m[3] * m[7] - m[4] * m[6]);
    d = d != 0. ? 1. / d : 0.;
    double t[9] = {(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d,
                   (m[1] * m[5] - m[2] * m[4]) * d, (m[5] * m[6] - m[3] * m[8]) * d,
                   (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
                   (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d,
                   (m[0] * m[4] - m[1] * m[3]) * d};
    for (int i = 0; i < 9; i++) o[i] = t[i];
}

// cv2.undistort works in stripes of rows: how many, and the inverse camera matrix of the stripe that starts at row y0
// (the stripe offset is folded into cy, R = I)
inline int undistort_stripe_rows(int w, int h)
{
    const int stripe = (1 << 12) / (w > 1 ? w : 1);
    return stripe < 1 ? 1 : (stripe > h ? h : stripe);
}
__host__ __device__ inline void stripe_inverse(const double K[9], int y0, double ir[9])
{
    double Ar[9];
    for (int q = 0; q < 9; q++) Ar[q] = K[q];
    Ar[5] = K[5] - y0;
    inv3(Ar, ir);
}

}  // namespace camd
