// points.hip -- matched points between the raw image and the pinhole model: Cam.undistort_points, Cam.project_points.
//
// Replaces (file:line in the reference's calibrating/):
//   camera.py:282-287   cv2.undistortPoints(uvs, K, D)[:, 0] * [[fx, fy]] + [cx, cy]   (epipolar_geometry.py:285-288, 327
//                       begins every run with it: matchers and optical flow see the raw frames)
//   camera.py:275-280   cv2.projectPoints(xyzs, rvec, tvec, K, D)[0][:, 0]
// One lane per point, nothing shared between lanes.  The arithmetic of the two cv2 calls is restated from OpenCV 4.x
// calib3d (cvUndistortPointsInternal without R / P and with TermCriteria(MAX_ITER, iters): a fixed trip count;
// cvProjectPoints2Internal without Jacobians) -- DESIGN.md section 2, U23 / U24: float64 inside, the input's type where
// cv2 hands an array over, products and sums in cv2's order, no contraction (-ffp-contract=off), divisions rounded once.
#include <climits>

#include "camera_model.hpp"

namespace camd {

struct PointsArgs {
    Pinhole cam;
    Lens k;
    double R[9], t[3];  // camd_project_points only
    int ndist, iters, pixels;  // camd_undistort_points only
};

// (u, v) of a row: one 8- / 16-byte access when every row starts on such a boundary (VEC), two scalar loads otherwise
template <typename T, bool VEC>
__device__ __forceinline__ void load_pair(const T* __restrict__ p, double& a, double& b)
{
    T v[2];
    if (VEC) {
        __builtin_memcpy(v, __builtin_assume_aligned(p, 2 * sizeof(T)), 2 * sizeof(T));
    } else {
        v[0] = p[0];
        v[1] = p[1];
    }
    a = (double)v[0], b = (double)v[1];
}

// out rows are [n][2] contiguous and start on a 2 * sizeof(T) boundary (the entry points insist): one 8- / 16-byte store
template <typename T>
__device__ __forceinline__ void store_pair(T* __restrict__ p, double a, double b)
{
    const T v[2] = {(T)a, (T)b};
    __builtin_memcpy(__builtin_assume_aligned(p, 2 * sizeof(T)), v, 2 * sizeof(T));
}

// TI: the rows' type, TO: the stored type.  The normalised point is rounded to TI first (what cv2 hands over), then
// either stored, or -- a.pixels -- taken back to pixels of the pinhole camera in float64: value * f + c, as NumPy does
// with the float64 K in camera.py:287.
template <typename TI, typename TO, bool VEC>
__global__ __launch_bounds__(256) void k_undistort_points(PointsArgs a, const TI* __restrict__ uv, size_t n, size_t stride,
                                                          TO* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double u, v;
    load_pair<TI, VEC>(uv + i * stride, u, v);
    const Lens& k = a.k;
    const double xs = (u - a.cam.cx) * a.cam.ifx, ys = (v - a.cam.cy) * a.cam.ify;
    double x = xs, y = ys;
    if (a.ndist) undistort_iterate(k, xs, ys, a.iters, x, y);
    x = (double)(TI)x, y = (double)(TI)y;
    if (a.pixels) x = x * a.cam.fx + a.cam.cx, y = y * a.cam.fy + a.cam.cy;
    store_pair<TO>(out + i * 2, x, y);
}

// VEC: float rows of a stride that is a multiple of 4 arrive as one 16-byte load (x, y, z and the element after them, which
// belongs to the row: stride >= 4 -- except, possibly, in the last row of a buffer that ends with z: that row is read
// element by element); double rows of an even stride as a 16-byte load (x, y) and z.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_project_points(PointsArgs a, const T* __restrict__ xyz, size_t n, size_t stride,
                                                        T* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const T* p = xyz + i * stride;
    double X, Y, Z;
    if (VEC && sizeof(T) == 4 && i + 1 < n) {
        T v[4];
        __builtin_memcpy(v, __builtin_assume_aligned(p, 16), 16);
        X = (double)v[0], Y = (double)v[1], Z = (double)v[2];
    } else if (VEC && sizeof(T) == 8) {
        load_pair<T, true>(p, X, Y);
        Z = (double)p[2];
    } else {
        X = (double)p[0], Y = (double)p[1], Z = (double)p[2];
    }
    double x = a.R[0] * X + a.R[1] * Y + a.R[2] * Z + a.t[0];
    double y = a.R[3] * X + a.R[4] * Y + a.R[5] * Z + a.t[1];
    const double z = a.R[6] * X + a.R[7] * Y + a.R[8] * Z + a.t[2];
    const double iz = z != 0. ? __ddiv_rn(1., z) : 1.;  // (z ? 1. / z : 1: a NaN z is "true" and divides)
    x *= iz, y *= iz;
    double xd, yd;
    distort_forward(a.k, x, y, xd, yd);
    store_pair<T>(out + i * 2, xd * a.cam.fx + a.cam.cx, yd * a.cam.fy + a.cam.cy);
}

static size_t value_bytes(int t) { return with_float(t, [](auto v) { return sizeof(v); }); }

// the point calls take cv2's own coefficient counts only; then K, dist -> a
static int camera_args(const char* who, const double K[9], const double* dist, int ndist, PointsArgs& a)
{
    if (!K || (ndist != 0 && ndist != 4 && ndist != 5 && ndist != 8 && ndist != 12 && ndist != 14) || (ndist > 0 && !dist)) {
        set_error("%s: bad arguments (K is 9 host doubles; ndist is 0, 4, 5, 8, 12 or 14, got %d)", who, ndist);
        return CAMD_ERR_BAD_ARG;
    }
    a.ndist = ndist;
    return unpack_camera(who, K, dist, ndist, &a.cam, &a.k);
}

// rows of `stride` elements of `type` starting at `in`, n of them, at least `need` elements each; out: [n][2] of out_type
static bool rows_ok(const void* in, int type, size_t n, int stride, int need, const void* out, int out_type)
{
    return float_type_ok(type) && float_type_ok(out_type) && stride >= need && n <= (size_t)INT_MAX &&
           (n == 0 || (in && out && (uintptr_t)in % value_bytes(type) == 0 && (uintptr_t)out % (2 * value_bytes(out_type)) == 0));
}

template <typename TI, typename TO>
static void launch_undistort(const PointsArgs& a, const void* uv, size_t n, int stride, void* out, hipStream_t stream)
{
    const bool vec = stride % 2 == 0 && (uintptr_t)uv % (2 * sizeof(TI)) == 0;
    const dim3 grid(div_up((long long)n, 256));
    if (vec)
        hipLaunchKernelGGL((k_undistort_points<TI, TO, true>), grid, dim3(256), 0, stream, a, (const TI*)uv, n, (size_t)stride,
                           (TO*)out);
    else
        hipLaunchKernelGGL((k_undistort_points<TI, TO, false>), grid, dim3(256), 0, stream, a, (const TI*)uv, n, (size_t)stride,
                           (TO*)out);
}

template <typename T>
static void launch_project(const PointsArgs& a, const void* xyz, size_t n, int stride, void* out, hipStream_t stream)
{
    const bool vec = stride % (16 / (int)sizeof(T)) == 0 && (uintptr_t)xyz % 16 == 0;
    const dim3 grid(div_up((long long)n, 256));
    if (vec)
        hipLaunchKernelGGL((k_project_points<T, true>), grid, dim3(256), 0, stream, a, (const T*)xyz, n, (size_t)stride, (T*)out);
    else
        hipLaunchKernelGGL((k_project_points<T, false>), grid, dim3(256), 0, stream, a, (const T*)xyz, n, (size_t)stride, (T*)out);
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_undistort_points(const void* uv, int uv_type, size_t n, int uv_stride, const double K[9], const double* dist,
                          int ndist, int iters, void* out, int out_type, void* stream)
{
    const int pixels = out_type & CAMD_POINTS_PIXELS;
    out_type &= ~CAMD_POINTS_PIXELS;
    if (!rows_ok(uv, uv_type, n, uv_stride, 2, out, out_type) || iters < 1 || iters > 100) {
        set_error("camd_undistort_points: bad arguments (uv / out: CAMD_VALUE_F64 or _F32, aligned to an element / a row of "
                  "two; uv_stride >= 2, got %d; n < 2^31; iters 1 .. 100, got %d)", uv_stride, iters);
        return CAMD_ERR_BAD_ARG;
    }
    PointsArgs a = {};
    int rc = camera_args("camd_undistort_points", K, dist, ndist, a);
    if (rc != CAMD_OK) return rc;
    a.iters = iters, a.pixels = pixels;
    if (n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    const hipStream_t st = (hipStream_t)stream;
    with_float(uv_type, [&](auto vi) {
        with_float(out_type, [&](auto vo) { launch_undistort<decltype(vi), decltype(vo)>(a, uv, n, uv_stride, out, st); });
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_project_points(const void* xyz, int xyz_type, size_t n, int xyz_stride, const double R[9], const double t[3],
                        const double K[9], const double* dist, int ndist, void* out, void* stream)
{
    if (!rows_ok(xyz, xyz_type, n, xyz_stride, 3, out, xyz_type) || !R || !t) {
        set_error("camd_project_points: bad arguments (xyz / out: CAMD_VALUE_F64 or _F32, aligned to an element / a row of "
                  "two; xyz_stride >= 3, got %d; n < 2^31; R, t: 9 and 3 host doubles)", xyz_stride);
        return CAMD_ERR_BAD_ARG;
    }
    PointsArgs a = {};
    int rc = camera_args("camd_project_points", K, dist, ndist, a);
    if (rc != CAMD_OK) return rc;
    for (int i = 0; i < 9; i++) a.R[i] = R[i];
    for (int i = 0; i < 3; i++) a.t[i] = t[i];
    if (n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    with_float(xyz_type, [&](auto v) { launch_project<decltype(v)>(a, xyz, n, xyz_stride, out, (hipStream_t)stream); });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
