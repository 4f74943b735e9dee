// distort.hip -- depth registered to the RAW (still distorted) image of camera 1: Stereo.distort_depth.
//
// Replaces (file:line in /root/reference/calibrating/):
//   stereo_camera.py:440-462   every pixel (u, v) of the undistorted image through cv2.undistortPoints(points, K, None),
//                              cv2.convertPointsToHomogeneous, cv2.projectPoints(., 0, 0, K, D), .astype(np.int32), then
//                              np.unique(axis=0, return_index=True): for every target pixel the FIRST source index
//   stereo_camera.py:438,463   res = zeros; res[y, x] = depths[index]
// The pixel mapping depends on the rig only: it is built once as a table of source indices (k_distort_index_scatter,
// "lowest source index wins" = atomicMin), and a call is one gather through that table (k_gather_by_index).
//
// The arithmetic of the two cv2 calls is restated from OpenCV 4.x calib3d (cvUndistortPointsInternal without
// distortion / R / P; cvProjectPoints2Internal with R = I, t = 0) -- DESIGN.md section 2, U21 / U22: float64 inside,
// float32 where cv2 hands an array over, the products and sums in cv2's order, no contraction (-ffp-contract=off).
#include <climits>

#include "camera_model.hpp"

namespace camd {

struct DistortArgs {
    Pinhole cam;
    Lens k;
    int w, h;
};

// stats words (int32): how the host learns, once per table, whether every target lies inside the image
enum { ST_N_OUT = 0, ST_MIN_U = 1, ST_MAX_U = 2, ST_MIN_V = 3, ST_MAX_V = 4, ST_N_NONFINITE = 5, ST_WORDS = 6 };

__host__ __device__ inline int stat_identity(int word)
{
    return (word == ST_MIN_U || word == ST_MIN_V) ? INT_MAX : ((word == ST_MAX_U || word == ST_MAX_V) ? INT_MIN : 0);
}

__global__ __launch_bounds__(256) void k_distort_index_init(uint32_t* __restrict__ key, int n, int* __restrict__ stats)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) key[i] = 0xFFFFFFFFu;  // "nobody lands here"; read back as int32 it is the hole marker -1
    if (i < ST_WORDS) stats[i] = stat_identity(i);
}

// .astype(np.int32) of a finite float32: truncation toward zero (values beyond +-2^30 are far outside any image and
// only feed the min / max words of the error message: clamped)
__device__ __forceinline__ int trunc_i32(float f)
{
    return fabsf(f) < 1073741824.f ? (int)f : (f < 0.f ? -1073741824 : 1073741824);
}

// One lane per source pixel i = v * w + u (row-major, the meshgrid order of stereo_camera.py:440-446).
__global__ __launch_bounds__(256) void k_distort_index_scatter(DistortArgs a, uint32_t* __restrict__ key,
                                                               int* __restrict__ stats)
{
    __shared__ int s[ST_WORDS];
    if (threadIdx.x < ST_WORDS) s[threadIdx.x] = stat_identity(threadIdx.x);
    __syncthreads();
    const int n = a.w * a.h;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int v = i / a.w, u = i - v * a.w;
        // cv2.undistortPoints(points, K, None): no distortion, no R, no P -> one multiply by the reciprocal; float32 out
        const double x = (double)(float)(((double)u - a.cam.cx) * a.cam.ifx);
        const double y = (double)(float)(((double)v - a.cam.cy) * a.cam.ify);
        // cv2.projectPoints((x, y, 1), rvec = 0, tvec = 0, K, D): R = I exactly, z = 1
        double xd, yd;
        distort_forward(a.k, x, y, xd, yd);
        const float U = (float)(xd * a.cam.fx + a.cam.cx), V = (float)(yd * a.cam.fy + a.cam.cy);
        if (!__builtin_isfinite(U) || !__builtin_isfinite(V)) {
            atomicAdd(&s[ST_N_OUT], 1);
            atomicAdd(&s[ST_N_NONFINITE], 1);
        } else {
            const int iu = trunc_i32(U), iv = trunc_i32(V);
            atomicMin(&s[ST_MIN_U], iu);
            atomicMax(&s[ST_MAX_U], iu);
            atomicMin(&s[ST_MIN_V], iv);
            atomicMax(&s[ST_MAX_V], iv);
            // the bounds test comes before the only global store of this lane: a target outside the image is counted,
            // never written (the reference raises IndexError on one side and wraps around on the other)
            if ((unsigned)iu < (unsigned)a.w && (unsigned)iv < (unsigned)a.h)
                atomicMin(&key[(size_t)iv * a.w + iu], (uint32_t)i);  // np.unique(return_index): the first occurrence
            else
                atomicAdd(&s[ST_N_OUT], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s[ST_N_OUT]) atomicAdd(&stats[ST_N_OUT], s[ST_N_OUT]);
        if (s[ST_N_NONFINITE]) atomicAdd(&stats[ST_N_NONFINITE], s[ST_N_NONFINITE]);
        if (s[ST_MIN_U] != INT_MAX) {  // (a workgroup of non-finite targets only has nothing to report)
            atomicMin(&stats[ST_MIN_U], s[ST_MIN_U]);
            atomicMax(&stats[ST_MAX_U], s[ST_MAX_U]);
            atomicMin(&stats[ST_MIN_V], s[ST_MIN_V]);
            atomicMax(&stats[ST_MAX_V], s[ST_MAX_V]);
        }
    }
}

// out[b][p] = idx[p] is a hole ? 0 : in[b][idx[p]].  A lane owns VEC consecutive target pixels -- their indices arrive
// as one 8- / 16-byte load and every image's values leave as one 16-byte store (VEC = 16 / sizeof(T); VEC = 1 when the
// image size or a pointer does not allow it) -- and blockIdx.y owns `zb` consecutive images of the batch, which share
// the index loads.  An index outside [0, n) reads nothing: holes (-1) and a foreign table alike.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_gather_by_index(const T* __restrict__ in, const int32_t* __restrict__ idx,
                                                         T* __restrict__ out, int n, int batch, int zb)
{
    const long long p = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (p >= n) return;  // (n % VEC == 0: a lane's pixels are all inside or all outside)
    int32_t s[VEC];
    __builtin_memcpy(s, __builtin_assume_aligned(idx + p, 4 * VEC), 4 * VEC);
    const int z0 = blockIdx.y * zb, nz = min(zb, batch - z0);
    const T* src = in + (size_t)z0 * n;
    T* dst = out + (size_t)z0 * n + p;
#pragma unroll 4
    for (int z = 0; z < nz; z++, src += n, dst += n) {
        T val[VEC];
#pragma unroll
        for (int q = 0; q < VEC; q++) val[q] = (unsigned)s[q] < (unsigned)n ? src[s[q]] : (T)0;
        __builtin_memcpy(__builtin_assume_aligned(dst, sizeof(T) * VEC), val, sizeof(T) * VEC);
    }
}

template <typename T>
static void launch_gather(const void* in, const int32_t* idx, void* out, int n, int batch, hipStream_t stream)
{
    constexpr int V = 16 / (int)sizeof(T);
    // 16-byte stores need every image of the batch to start on a 16-byte boundary (n % V == 0 with an aligned base)
    const bool vec = n % V == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)idx % (4 * V) == 0;
    const int lanes = vec ? n / V : n;
    const int zb = images_per_group(div_up(lanes, 256), batch);  // as k_unrectify: the images share the index loads
    const dim3 grid(div_up(lanes, 256), div_up(batch, zb));
    if (vec)
        hipLaunchKernelGGL((k_gather_by_index<T, V>), grid, dim3(256), 0, stream, (const T*)in, idx, (T*)out, n, batch, zb);
    else
        hipLaunchKernelGGL((k_gather_by_index<T, 1>), grid, dim3(256), 0, stream, (const T*)in, idx, (T*)out, n, batch, zb);
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_distort_index_map(const double K[9], const double* dist, int ndist, int w, int h, int32_t* src_index,
                           int32_t* stats, void* stream)
{
    if (!K || !src_index || !stats || w <= 0 || h <= 0 || ndist < 0 || ndist > 14 || (ndist > 0 && !dist) ||
        (long long)w * h > INT_MAX || w >= (1 << 24) || h >= (1 << 24)) {
        set_error("camd_distort_index_map: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    DistortArgs a;
    int rc = unpack_camera("camd_distort_index_map", K, dist, ndist, &a.cam, &a.k);
    if (rc != CAMD_OK) return rc;
    CAMD_NEED_DEVICE();
    a.w = w, a.h = h;
    const int n = w * h;
    const dim3 grid(div_up(n > ST_WORDS ? n : ST_WORDS, 256));
    hipLaunchKernelGGL(k_distort_index_init, grid, dim3(256), 0, (hipStream_t)stream, (uint32_t*)src_index, n, stats);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_distort_index_scatter, grid, dim3(256), 0, (hipStream_t)stream, a, (uint32_t*)src_index, stats);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_distort_depth(const void* depth, int elem_bytes, int w, int h, const int32_t* src_index, void* out, int batch,
                       void* stream)
{
    if (!depth || !src_index || !out || depth == out || w <= 0 || h <= 0 || batch <= 0 || batch > (1 << 19) ||
        (long long)w * h > INT_MAX ||
        (elem_bytes != 4 && elem_bytes != 8) || (uintptr_t)depth % elem_bytes || (uintptr_t)out % elem_bytes ||
        (uintptr_t)src_index % 4) {
        set_error("camd_distort_depth: bad arguments (elem_bytes is 4 or 8; out must not alias depth; batch <= 2^19)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    if (elem_bytes == 8)
        launch_gather<double>(depth, src_index, out, w * h, batch, (hipStream_t)stream);
    else
        launch_gather<float>(depth, src_index, out, w * h, batch, (hipStream_t)stream);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
