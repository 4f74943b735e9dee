// pnp_common.hpp -- what the per-frame solvers share: pnp.hip (a pose per frame) and calibrate.hip (the intrinsics and a
// pose per frame).  One wavefront per frame.  It offers:
//   points_ok, doubles_ok; frame_rows, load_point, frame_nonfinite   the host's check of the points; a frame's checked rows
//   wave_sum, wave_sum_all, wave_or, uniform   the fixed-order butterfly: the same bits of a sum in every lane
//   wave_lds_fence                             orders a wave's writes to its own LDS slice against its other lanes' reads
//   load_pose, store_pose, pose_terms          R, t as 12 doubles; a point's residual (raw pixels) and 2 x 6 pose Jacobian
//   add_outer, add_gradient                    J^T J (packed lower triangle) and J^T r, two rows of J at a time
//   damped, cholesky, cholesky_solve           (A + lambda diag A) x = b in registers
//   unit_diagonal_pivot, SINGULAR_PIVOT        the rank test: the smallest pivot of A scaled to a unit diagonal
//   LM_*, lm_small, lm_next, lm_stopped        the one Levenberg-Marquardt rule (damping, stopping); pose_norm2: its |p|^2
//   lm_better                                  the joint solvers' acceptance: a lower cost, or one within the rounding of the sums
//   rotate_left; null_vector, direct_linear_transform   R <- exp([w]x) R; the Hartley-normalised start (H or P)
// pnp.hip accepts a step by the bare comparison of the costs; the joint solvers (calibrate.hip, stereo_calibrate.hip,
// bundle.hip) by lm_better, inside joint_common.hpp's lm_update: what those solvers share beyond these primitives is there.
#pragma once

#include <climits>

#include "camera_model.hpp"

namespace camd {

enum { PNP_OK = 0, PNP_FEW = 1, PNP_NONFINITE = 2, PNP_SINGULAR = 3 };
constexpr int PNP_MAX_ITERATIONS = 100;
constexpr int PNP_UNDISTORT_ITERS = 10;  // rounds of cv2.undistortPoints' iteration for the start pose (cv2 runs 5)
constexpr double SINGULAR_PIVOT = 1e-10;  // smallest pivot of the unit-diagonal (reduced) normal matrix that still counts

// ---- the Levenberg-Marquardt rule of every solver here: Marquardt's lambda diag(J^T J); calibrate.py writes the start ----
constexpr double LM_LAMBDA_START = 1e-3, LM_LAMBDA_DOWN = 0.1, LM_LAMBDA_UP = 10.;  // after a step that is taken / is not
constexpr double LM_LAMBDA_MIN = 1e-12, LM_LAMBDA_MAX = 1e12, LM_EPS = 0x1p-52;  // small: |step| < eps (|p| + eps), given squared
__device__ __forceinline__ bool lm_small(double step2, double norm2) { return sqrt(step2) < LM_EPS * (sqrt(norm2) + LM_EPS); }
__device__ __forceinline__ double lm_next(double lambda, bool better) { return better ? lambda * LM_LAMBDA_DOWN : lambda * LM_LAMBDA_UP; }
__device__ __forceinline__ bool lm_stopped(bool small, double lambda) { return small || lambda < LM_LAMBDA_MIN || lambda > LM_LAMBDA_MAX; }
// The acceptance of a step of the JOINT solvers (calibrate.hip, stereo_calibrate.hip): a candidate is taken when its cost
// is lower, or higher by no more than the rounding of the sums can explain (64 ulp of the cost).  Near the minimum the
// cost is flat to rounding while the step is still accurate (it comes from the gradient); rejecting such steps by the
// noise of `c2 < c` would leave the parameters about sqrt(eps c / h) from the minimum along the flattest direction h,
// 1e-7 .. 1e-6 px in K, and dependent on the order of the sums.  (pnp.hip takes the bare comparison.)
constexpr double LM_COST_RESOLUTION = 64 * 0x1p-52;
__device__ __forceinline__ bool lm_better(double c2, double c) { return c2 < c || c2 - c <= LM_COST_RESOLUTION * c; }
// |p|^2 of one pose: R's Frobenius norm and t
__device__ __forceinline__ double pose_norm2(const double* t) { return 3. + t[0] * t[0] + t[1] * t[1] + t[2] * t[2]; }

struct PnpArgs {
    Pinhole cam;
    Lens k;
    camd_pnp_points p;
    double plane[9];  // camd_pnp_init, planar: the rotation that lays the target's plane on z = const
    int planar, min_points;
};

// the host's checks: rows of a float type, aligned to an element, with their strides; an aligned device array of doubles
static inline bool points_ok(const camd_pnp_points* p)
{
    return p && p->frames >= 0 && float_type_ok(p->object_type) && float_type_ok(p->image_type) && p->object_stride >= 3 &&
           p->image_stride >= 2 &&
           (p->frames == 0 || (p->object && p->image && p->start && (uintptr_t)p->start % 8 == 0 &&
                               (uintptr_t)p->object % (p->object_type == CAMD_VALUE_F64 ? 8 : 4) == 0 &&
                               (uintptr_t)p->image % (p->image_type == CAMD_VALUE_F64 ? 8 : 4) == 0));
}
static inline bool doubles_ok(const void* p) { return p && (uintptr_t)p % 8 == 0; }

// sum over the wave, the same bits in every lane: lane i adds lane i ^ m, and a + b == b + a
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}
template <int N>
__device__ __forceinline__ void wave_sum_all(double* x)
{
#pragma unroll
    for (int q = 0; q < N; q++) x[q] = wave_sum(x[q]);
}
__device__ __forceinline__ int wave_or(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v |= __shfl_xor(v, m, 64);
    return v;
}
// a flag every lane agrees on, as a scalar: the branches on it are uniform and the wave stays whole for the butterflies
__device__ __forceinline__ bool uniform(bool b) { return __builtin_amdgcn_readfirstlane((int)b) != 0; }
// what a wave wrote to its own slice of LDS is read by its other lanes (and the other way round): LDS serves a wave's
// instructions in order, so only the compiler has to be held to that order (subpix.hip, chessboard.hip)
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double load_value(const void* p, int type, size_t i)
{
    return with_float(type, [&](auto v) { return (double)((const decltype(v)*)p)[i]; });
}

// the rows of one frame, checked: [s, s + n) of the image rows, the same of the object rows or [0, n) of a shared block
struct Frame {
    size_t uv0, obj0;
    int n, status;
};

__device__ __forceinline__ Frame frame_rows(const camd_pnp_points& p, int f, int min_points)
{
    Frame fr = {0, 0, 0, PNP_OK};
    const long long s = p.start[f], e = p.start[f + 1];
    const unsigned long long obj_rows = p.object_rows;
    if (s < 0 || e < s || (unsigned long long)e > p.image_rows || e - s > INT_MAX ||
        (unsigned long long)(p.object_shared ? e - s : e) > obj_rows) {
        fr.status = PNP_NONFINITE;  // a range outside the rows: nothing of it is read
        return fr;
    }
    fr.n = (int)(e - s), fr.uv0 = (size_t)s, fr.obj0 = p.object_shared ? 0 : (size_t)s;
    if (fr.n < min_points) fr.status = PNP_FEW;
    return fr;
}

__device__ __forceinline__ void load_point(const camd_pnp_points& p, const Frame& fr, int i, double X[3], double uv[2])
{
    const size_t o = (fr.obj0 + i) * (size_t)p.object_stride, q = (fr.uv0 + i) * (size_t)p.image_stride;
    X[0] = load_value(p.object, p.object_type, o), X[1] = load_value(p.object, p.object_type, o + 1);
    X[2] = load_value(p.object, p.object_type, o + 2);
    uv[0] = load_value(p.image, p.image_type, q), uv[1] = load_value(p.image, p.image_type, q + 1);
}

// 1 when any coordinate of the frame is NaN or infinite (every lane gets the answer)
__device__ __forceinline__ bool frame_nonfinite(const camd_pnp_points& p, const Frame& fr, int lane)
{
    int bad = 0;
    for (int i = lane; i < fr.n; i += 64) {
        double X[3], uv[2];
        load_point(p, fr, i, X, uv);
        bad |= !(isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) && isfinite(uv[0]) && isfinite(uv[1]));
    }
    return uniform(wave_or(bad) != 0);
}

// R, t as 12 doubles; false where one of them is NaN or infinite
__device__ __forceinline__ bool load_pose(const double* src, double* R, double* t)
{
    bool finite = true;
    for (int q = 0; q < 12; q++) {
        const double v = src[q];
        finite = finite && isfinite(v);
        if (q < 9) R[q] = v; else t[q - 9] = v;
    }
    return finite;
}
__device__ __forceinline__ void store_pose(double* dst, const double* R, const double* t, bool ok = true)  // NaN where not ok
{
    for (int q = 0; q < 12; q++) dst[q] = ok ? (q < 9 ? R[q] : t[q - 9]) : NAN;
}

// One point under R, t, cam, lens: the residual r (projected - observed, raw pixels) and its 2 x 6 Jacobian J with respect
// to R <- exp([w]x) R, t <- t + d.  Returned: the normalised image point before the lens (x, y) and behind it (xd, yd).
struct Projected { double x, y, xd, yd; };
__device__ __forceinline__ Projected pose_terms(const camd_pnp_points& p, const Frame& fr, int i, const Pinhole& cam, const Lens& k,
                                                const double* R, const double* t, double r[2], double J[2][6])
{
    double X[3], uv[2];
    load_point(p, fr, i, X, uv);
    const double P[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2], R[3] * X[0] + R[4] * X[1] + R[5] * X[2],
                         R[6] * X[0] + R[7] * X[1] + R[8] * X[2]};
    const double z = P[2] + t[2];
    const double iz = z != 0. ? __ddiv_rn(1., z) : 1.;  // (camd_project_points' rule)
    const double x = (P[0] + t[0]) * iz, y = (P[1] + t[1]) * iz;
    double xd, yd, d[4];
    distort_forward(k, x, y, xd, yd);
    distort_forward_jacobian(k, x, y, d);
    r[0] = xd * cam.fx + cam.cx - uv[0], r[1] = yd * cam.fy + cam.cy - uv[1];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const double f = e ? cam.fy : cam.fx, dx = d[2 * e] * f, dy = d[2 * e + 1] * f;
        const double g[3] = {dx * iz, dy * iz, -(dx * x + dy * y) * iz};  // d pixel / d camera point
        J[e][0] = P[1] * g[2] - P[2] * g[1];                            // (R X) x g
        J[e][1] = P[2] * g[0] - P[0] * g[2];
        J[e][2] = P[0] * g[1] - P[1] * g[0];
        J[e][3] = g[0], J[e][4] = g[1], J[e][5] = g[2];
    }
    return {x, y, xd, yd};
}

// ---- a symmetric positive definite system of N unknowns, lower triangle packed row by row: L[i (i + 1) / 2 + j] ----
// every index is a constant after unrolling, so the triangle lives in registers
// A += a0 a0^T + a1 a1^T and g += a0 r[0] + a1 r[1]: the two rows of one point's Jacobian
template <int N>
__device__ __forceinline__ void add_outer(double* A, const double* a0, const double* a1)
{
#pragma unroll
    for (int p = 0; p < N; p++)
#pragma unroll
        for (int q = 0; q <= p; q++) A[p * (p + 1) / 2 + q] += a0[p] * a0[q] + a1[p] * a1[q];
}
template <int N>
__device__ __forceinline__ void add_gradient(double* g, const double* a0, const double* a1, const double* r)
{
#pragma unroll
    for (int p = 0; p < N; p++) g[p] += a0[p] * r[0] + a1[p] * r[1];
}
// L = A + lambda diag A, for the caller to factor
template <int N>
__device__ __forceinline__ void damped(const double* A, double lambda, double* L)
{
#pragma unroll
    for (int q = 0; q < N * (N + 1) / 2; q++) L[q] = A[q];
#pragma unroll
    for (int q = 0; q < N; q++) L[q * (q + 1) / 2 + q] += lambda * A[q * (q + 1) / 2 + q];
}
template <int N>
__device__ __forceinline__ bool cholesky(double* L, double& min_pivot)
{
    bool ok = true;
    min_pivot = INFINITY;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double d = L[j * (j + 1) / 2 + j];
#pragma unroll
        for (int q = 0; q < j; q++) d -= L[j * (j + 1) / 2 + q] * L[j * (j + 1) / 2 + q];
        min_pivot = d < min_pivot ? d : min_pivot;
        ok = ok && d > 0. && isfinite(d);
        const double r = sqrt(d), ir = __ddiv_rn(1., r);
        L[j * (j + 1) / 2 + j] = r;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double s = L[i * (i + 1) / 2 + j];
#pragma unroll
            for (int q = 0; q < j; q++) s -= L[i * (i + 1) / 2 + q] * L[j * (j + 1) / 2 + q];
            L[i * (i + 1) / 2 + j] = s * ir;
        }
    }
    return ok;
}
template <int N>
__device__ __forceinline__ void cholesky_solve(const double* L, double* x)  // x: the right-hand side in, the solution out
{
#pragma unroll
    for (int i = 0; i < N; i++) {
        double s = x[i];
#pragma unroll
        for (int q = 0; q < i; q++) s -= L[i * (i + 1) / 2 + q] * x[q];
        x[i] = __ddiv_rn(s, L[i * (i + 1) / 2 + i]);
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double s = x[i];
#pragma unroll
        for (int q = i + 1; q < N; q++) s -= L[q * (q + 1) / 2 + i] * x[q];
        x[i] = __ddiv_rn(s, L[i * (i + 1) / 2 + i]);
    }
}

// the rank test: A scaled to a unit diagonal, factored; its smallest pivot is compared with SINGULAR_PIVOT by the caller
template <int N>
__device__ __forceinline__ bool unit_diagonal_pivot(const double* A, double& pivot)
{
    double L[N * (N + 1) / 2], s[N];
#pragma unroll
    for (int q = 0; q < N; q++) s[q] = __ddiv_rn(1., sqrt(A[q * (q + 1) / 2 + q]));
#pragma unroll
    for (int p = 0; p < N; p++)
#pragma unroll
        for (int q = 0; q <= p; q++) L[p * (p + 1) / 2 + q] = A[p * (p + 1) / 2 + q] * s[p] * s[q];
    return cholesky<N>(L, pivot);
}

// R2 = exp([w]x) R: I + A [w]x + B [w]x^2 with A = sin(th) / th, B = (sin(th / 2) / (th / 2))^2 / 2, no cancellation
__device__ __forceinline__ void rotate_left(const double w[3], const double* R, double* R2)
{
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), h = 0.5 * th;
    const double A = th > 0. ? __ddiv_rn(sin(th), th) : 1., sh = h > 0. ? __ddiv_rn(sin(h), h) : 1., B = 0.5 * sh * sh;
    const double E[9] = {1 - B * (w[1] * w[1] + w[2] * w[2]), B * w[0] * w[1] - A * w[2], B * w[0] * w[2] + A * w[1],
                         B * w[0] * w[1] + A * w[2], 1 - B * (w[0] * w[0] + w[2] * w[2]), B * w[1] * w[2] - A * w[0],
                         B * w[0] * w[2] - A * w[1], B * w[1] * w[2] + A * w[0], 1 - B * (w[0] * w[0] + w[1] * w[1])};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R2[3 * i + j] = E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j] + E[3 * i + 2] * R[6 + j];
}

// The null vector of the N x N normal matrix M of a direct linear transform (lower triangle packed): inverse iteration on
// M + mu I, a fixed number of rounds -- a start for the refinement needs no more
template <int N>
__device__ __forceinline__ bool null_vector(double* M, double* v)
{
    double trace = 0.;
#pragma unroll
    for (int q = 0; q < N; q++) trace += M[q * (q + 1) / 2 + q];
    const double mu = 1e-13 * trace;
#pragma unroll
    for (int q = 0; q < N; q++) M[q * (q + 1) / 2 + q] += mu, v[q] = 1. + 0.25 * q;
    double pivot;
    bool ok = cholesky<N>(M, pivot);
#pragma unroll 1
    for (int round = 0; round < 6; round++) {
        cholesky_solve<N>(M, v);
        double s = 0.;
#pragma unroll
        for (int q = 0; q < N; q++) s += v[q] * v[q];
        s = __ddiv_rn(1., sqrt(s));
#pragma unroll
        for (int q = 0; q < N; q++) v[q] *= s;
    }
#pragma unroll
    for (int q = 0; q < N; q++) ok = ok && isfinite(v[q]);
    return ok;
}

// C = 3: the homography of a plane (object x, y -> normalised image), C = 4: the projection matrix (x, y, z -> image).
// Hartley-normalised on both sides; G (3 x C, row-major) comes back in the units of the caller.
template <int C>
__device__ __forceinline__ bool direct_linear_transform(const PnpArgs& a, const Frame& fr, int lane, double* G, double* centre)
{
    constexpr int N = 3 * C, D = C - 1;
    // the object points in the plane's frame (planar) and the undistorted, normalised image points: means, then scales
    auto point = [&](int i, double* X, double* xy) {
        double W[3], uv[2];
        load_point(a.p, fr, i, W, uv);
        for (int q = 0; q < 3; q++) X[q] = a.plane[3 * q] * W[0] + a.plane[3 * q + 1] * W[1] + a.plane[3 * q + 2] * W[2];
        undistort_iterate(a.k, (uv[0] - a.cam.cx) * a.cam.ifx, (uv[1] - a.cam.cy) * a.cam.ify, PNP_UNDISTORT_ITERS, xy[0], xy[1]);
    };
    double m[5] = {0., 0., 0., 0., 0.};
    for (int i = lane; i < fr.n; i += 64) {
        double X[3], xy[2];
        point(i, X, xy);
        m[0] += X[0], m[1] += X[1], m[2] += X[2], m[3] += xy[0], m[4] += xy[1];
    }
    const double in = __ddiv_rn(1., (double)fr.n);
#pragma unroll
    for (int q = 0; q < 5; q++) m[q] = wave_sum(m[q]) * in;
    centre[0] = m[0], centre[1] = m[1], centre[2] = m[2];
    double so = 0., si = 0.;
    for (int i = lane; i < fr.n; i += 64) {
        double X[3], xy[2];
        point(i, X, xy);
        double dd = 0.;
        for (int q = 0; q < D; q++) dd += (X[q] - m[q]) * (X[q] - m[q]);
        so += sqrt(dd);
        si += sqrt((xy[0] - m[3]) * (xy[0] - m[3]) + (xy[1] - m[4]) * (xy[1] - m[4]));
    }
    so = __ddiv_rn(sqrt((double)D), wave_sum(so) * in), si = __ddiv_rn(sqrt(2.), wave_sum(si) * in);  // mean distance sqrt(D), sqrt(2)
    double M[N * (N + 1) / 2];
#pragma unroll
    for (int q = 0; q < N * (N + 1) / 2; q++) M[q] = 0.;
    for (int i = lane; i < fr.n; i += 64) {
        double X[3], xy[2], h[C], r[2][N];
        point(i, X, xy);
#pragma unroll
        for (int q = 0; q < D; q++) h[q] = (X[q] - m[q]) * so;
        h[D] = 1.;
        const double x = (xy[0] - m[3]) * si, y = (xy[1] - m[4]) * si;
#pragma unroll
        for (int q = 0; q < C; q++) {
            r[0][q] = h[q], r[0][C + q] = 0., r[0][2 * C + q] = -x * h[q];
            r[1][q] = 0., r[1][C + q] = h[q], r[1][2 * C + q] = -y * h[q];
        }
        add_outer<N>(M, r[0], r[1]);
    }
    wave_sum_all<N * (N + 1) / 2>(M);
    double v[N];
    const bool ok = null_vector<N>(M, v);
    // G = Ti^-1 Gn To: To = [so I, -so mean; 0 1], Ti^-1 = [1 / si, 0, mx; 0, 1 / si, my; 0, 0, 1]
    const double isi = __ddiv_rn(1., si);
#pragma unroll
    for (int row = 0; row < 3; row++) {
        double last = v[row * C + D];
#pragma unroll
        for (int q = 0; q < D; q++) last -= so * m[q] * v[row * C + q], G[row * C + q] = so * v[row * C + q];
        G[row * C + D] = last;
    }
#pragma unroll
    for (int q = 0; q < C; q++) {
        G[q] = G[q] * isi + m[3] * G[2 * C + q];
        G[C + q] = G[C + q] * isi + m[4] * G[2 * C + q];
    }
    return ok;
}

}  // namespace camd
