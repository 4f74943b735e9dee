// subpix.hip -- detected corners refined to sub-pixel, every corner of every frame in one launch; the gray image they
// are refined on.
//
// Replaces (file:line in the reference's calibrating/):
//   boards.py:159      cv2.cvtColor(img, cv2.COLOR_BGR2GRAY) on uint8                     -> camd_bgr_to_gray_u8
//   boards.py:163-169  cv2.cornerSubPix(gray, corners, (4, 4), (-1, -1), (EPS + MAX_ITER, 30, 0.01))  -> camd_corner_sub_pix
// One wavefront per corner, four corners per 256-thread workgroup and NO workgroup barrier anywhere, as in pnp.hip: the
// waves of a group belong to different corners and run different numbers of iterations.  Per iteration the lanes sample
// the (2 win + 3)^2 float32 patch around the corner into the wave's own slice of LDS (written and read by this wave
// only: a wavefront-scope fence orders the two), then stride over the window -- pixel k, row-major, belongs to lane
// k % 64, which adds its pixels in rising k -- and an xor butterfly of fixed order leaves the same bits of the five
// sums in every lane.  The 2 x 2 solve and the stopping rule are computed by every lane, redundantly and uniformly, and
// a corner's result depends on nothing but its own start and its frame: alone or anywhere in a batch it gets the same
// bits.  Every loop has a trip count bounded by a constant, the window or the frame count.
//
// cv2's own arithmetic is UNPINNED: both procedures are restated from recollection.
#include <cfloat>

#include "pnp_common.hpp"

namespace camd {

enum { SUBPIX_SINGULAR = 1, SUBPIX_LEFT_IMAGE = 2, SUBPIX_REVERTED = 4, SUBPIX_BAD_START = 8 };
constexpr int SUBPIX_MAX_ITERATIONS = 100;
constexpr int SUBPIX_MAX_PATCH = 4096;  // floats of one wave's slice: four slices fill the 64 KiB a group may ask for

struct SubpixArgs {
    const uint8_t* gray;
    size_t pitch, stride;
    const void* corners;
    const long long* start;  // frames + 1 rising row indices, or null: `per_frame` rows each
    const float* mask;
    void* out;
    int* iterations;
    int* status;
    double eps;
    unsigned rows, per_frame;
    int w, h, frames, win_w, win_h, max_iters;
};

// the frame that owns row c, or -1: the first f with start[f + 1] > c (frames without a row are stepped over)
__device__ __forceinline__ int frame_of(const SubpixArgs& a, unsigned c)
{
    if (!a.start) {
        const unsigned f = c / a.per_frame;
        return f < (unsigned)a.frames ? (int)f : -1;
    }
    int lo = 0, hi = a.frames;
    while (lo < hi) {  // at most 31 rounds
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (a.start[mid + 1] > (long long)c) hi = mid; else lo = mid + 1;
    }
    return lo < a.frames && a.start[lo] <= (long long)c ? lo : -1;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <typename T>
__device__ __forceinline__ void store_corner(const SubpixArgs& a, unsigned c, T x, T y, int iterations, int status)
{
    T* o = (T*)a.out + (size_t)c * 2;
    o[0] = x, o[1] = y;
    a.iterations[c] = iterations;
    a.status[c] = status;
}

template <typename T>
__global__ __launch_bounds__(256) void k_corner_sub_pix(SubpixArgs a)
{
    extern __shared__ float slices[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long row = (unsigned long long)blockIdx.x * 4 + wave;
    if (row >= a.rows) return;  // (the whole wave; there is no barrier to miss)
    const unsigned c = (unsigned)row;
    const int ww = a.win_w, wh = a.win_h, pw = 2 * ww + 3, ph = 2 * wh + 3, winw = 2 * ww + 1, nwin = winw * (2 * wh + 1);
    const int npatch = pw * ph;
    float* patch = slices + (size_t)wave * npatch;

    const T sx = ((const T*)a.corners)[(size_t)c * 2], sy = ((const T*)a.corners)[(size_t)c * 2 + 1];
    const float cTx = (float)sx, cTy = (float)sy;
    const int f = frame_of(a, c);
    // a start that is not a pixel of its frame: cv2 asserts; here the corner comes back as it came and nothing is read
    if (!uniform(f >= 0 && cTx >= 0.f && cTx < (float)a.w && cTy >= 0.f && cTy < (float)a.h)) {
        if (lane == 0) store_corner<T>(a, c, sx, sy, 0, SUBPIX_BAD_START);
        return;
    }
    const uint8_t* img = a.gray + (size_t)f * a.stride;
    float cIx = cTx, cIy = cTy;
    int iter = 0, count = 0, status = 0;
    double err = 0.;
    do {
        count++;
        // the patch: getRectSubPix of pw x ph at cI, replicate border
        const float cx = cIx - (float)(pw - 1) * 0.5f, cy = cIy - (float)(ph - 1) * 0.5f;
        const float fx = floorf(cx), fy = floorf(cy);
        const int ix = (int)fx, iy = (int)fy;
        const float fa = cx - fx, fb = cy - fy;
        const float a11 = (1.f - fa) * (1.f - fb), a12 = fa * (1.f - fb), a21 = (1.f - fa) * fb, a22 = fa * fb;
        for (int p = lane; p < npatch; p += 64) {
            const int i = p / pw, j = p - i * pw;
            const int x0 = clampi(ix + j, a.w - 1), x1 = clampi(ix + j + 1, a.w - 1);
            const uint8_t* r0 = img + (size_t)clampi(iy + i, a.h - 1) * a.pitch;
            const uint8_t* r1 = img + (size_t)clampi(iy + i + 1, a.h - 1) * a.pitch;
            patch[p] = ((a11 * (float)r0[x0] + a12 * (float)r0[x1]) + a21 * (float)r1[x0]) + a22 * (float)r1[x1];
        }
        wave_lds_fence();
        double s[5] = {0., 0., 0., 0., 0.};  // a, b, c, bb1, bb2
        for (int k = lane; k < nwin; k += 64) {
            const int i = k / winw, j = k - i * winw;
            const float* q = patch + (i + 1) * pw + (j + 1);
            const double tgx = (double)q[1] - (double)q[-1], tgy = (double)q[pw] - (double)q[-pw], m = (double)a.mask[k];
            const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
            const double px = (double)(j - ww), py = (double)(i - wh);
            s[0] += gxx, s[1] += gxy, s[2] += gyy;
            s[3] += gxx * px + gxy * py;
            s[4] += gxy * px + gyy * py;
        }
        wave_lds_fence();  // (the next round writes the slice again)
        wave_sum_all<5>(s);
        const double det = s[0] * s[2] - s[1] * s[1];
        if (uniform(!(fabs(det) > DBL_EPSILON * DBL_EPSILON))) {
            status |= SUBPIX_SINGULAR;
            break;
        }
        const double scale = __ddiv_rn(1., det);
        const float nx = (float)((double)cIx + s[2] * scale * s[3] - s[1] * scale * s[4]);
        const float ny = (float)((double)cIy - s[1] * scale * s[3] + s[0] * scale * s[4]);
        const double dx = (double)(nx - cIx), dy = (double)(ny - cIy);
        err = dx * dx + dy * dy;
        cIx = nx, cIy = ny;
        if (uniform(!(cIx >= 0.f && cIx < (float)a.w && cIy >= 0.f && cIy < (float)a.h))) {  // (a NaN has left it too)
            status |= SUBPIX_LEFT_IMAGE;
            break;
        }
    } while (uniform(++iter < a.max_iters && err > a.eps));
    // a corner that moved further than its window was not the one it started at
    if (uniform(!(fabsf(cIx - cTx) <= (float)ww && fabsf(cIy - cTy) <= (float)wh))) {
        cIx = cTx, cIy = cTy;
        status |= SUBPIX_REVERTED;
    }
    if (lane == 0) store_corner<T>(a, c, (T)cIx, (T)cIy, count, status);
}

// ---- gray -------------------------------------------------------------------------------------------------------
// four pixels per thread: 12 bytes in, 4 out; rows whose bytes are dword-aligned on both sides move as dwords
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_bgr_to_gray_u8(const uint8_t* __restrict__ src, int w, int h, size_t src_pitch,
                                                       size_t src_stride, uint8_t* __restrict__ dst, size_t dst_pitch,
                                                       size_t dst_stride, int batch, int k0, int k1, int k2, int shift)
{
    const int x = (int)(blockIdx.x * 256 + threadIdx.x) * 4;
    if (x >= w) return;
    const int half = 1 << (shift - 1);
    for (int b = blockIdx.z; b < batch; b += gridDim.z)
        for (int y = blockIdx.y; y < h; y += gridDim.y) {
            const uint8_t* s = src + (size_t)b * src_stride + (size_t)y * src_pitch + (size_t)x * 3;
            uint8_t* d = dst + (size_t)b * dst_stride + (size_t)y * dst_pitch + x;
            if (ALIGNED && x + 4 <= w) {
                const uint32_t* s4 = (const uint32_t*)s;
                const uint32_t q0 = s4[0], q1 = s4[1], q2 = s4[2];
                const int g0 = (int)(q0 & 255) * k0 + (int)((q0 >> 8) & 255) * k1 + (int)((q0 >> 16) & 255) * k2 + half;
                const int g1 = (int)(q0 >> 24) * k0 + (int)(q1 & 255) * k1 + (int)((q1 >> 8) & 255) * k2 + half;
                const int g2 = (int)((q1 >> 16) & 255) * k0 + (int)(q1 >> 24) * k1 + (int)(q2 & 255) * k2 + half;
                const int g3 = (int)((q2 >> 8) & 255) * k0 + (int)((q2 >> 16) & 255) * k1 + (int)(q2 >> 24) * k2 + half;
                *(uint32_t*)d = (uint32_t)(g0 >> shift) | (uint32_t)(g1 >> shift) << 8 | (uint32_t)(g2 >> shift) << 16 |
                                (uint32_t)(g3 >> shift) << 24;
            } else {
                const int n = w - x < 4 ? w - x : 4;
                for (int q = 0; q < n; q++)
                    d[q] = (uint8_t)(((int)s[3 * q] * k0 + (int)s[3 * q + 1] * k1 + (int)s[3 * q + 2] * k2 + half) >> shift);
            }
        }
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_corner_sub_pix(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, const void* corners,
                        int corner_type, size_t rows, const long long* start, int win_w, int win_h, const float* mask,
                        int max_iters, double eps, void* out, int* iterations, int* status, void* queue)
{
    const size_t elem = corner_type == CAMD_VALUE_F64 ? 8 : 4;
    if (win_w <= 0 || win_h <= 0) {
        set_error("camd_corner_sub_pix: the window's half-sizes must be positive, got (%d, %d)", win_w, win_h);
        return CAMD_ERR_BAD_ARG;
    }
    if (w < 1 || h < 1 || frames < 1 || (long long)w < 2LL * win_w + 5 || (long long)h < 2LL * win_h + 5) {
        set_error("camd_corner_sub_pix: %d image(s) of %d x %d; a window of (%d, %d) needs at least %lld x %lld", frames, w, h,
                  win_w, win_h, 2LL * win_w + 5, 2LL * win_h + 5);
        return CAMD_ERR_BAD_ARG;
    }
    if (!float_type_ok(corner_type) || rows >= ((size_t)1 << 31) || max_iters < 1 || max_iters > SUBPIX_MAX_ITERATIONS ||
        !(eps >= 0.) || pitch < (size_t)w || (frames > 1 && stride < (size_t)(h - 1) * pitch + (size_t)w) ||
        (!start && rows % (size_t)frames != 0) || (start && (uintptr_t)start % 8 != 0)) {
        set_error("camd_corner_sub_pix: bad arguments (corners: CAMD_VALUE_F64 or _F32, fewer than 2^31 rows, without start a "
                  "multiple of the %d frames, got %zu; start: frames + 1 device int64; max_iters 1 .. 100, got %d; eps >= 0; "
                  "pitch >= w, stride >= an image)", frames, rows, max_iters);
        return CAMD_ERR_BAD_ARG;
    }
    if ((long long)(2 * win_w + 3) * (2 * win_h + 3) > SUBPIX_MAX_PATCH) {
        set_error("camd_corner_sub_pix: a window of (%d, %d) needs a patch of %lld floats, a wave's slice holds %d", win_w, win_h,
                  (long long)(2 * win_w + 3) * (2 * win_h + 3), SUBPIX_MAX_PATCH);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (rows == 0) return CAMD_OK;
    if (!gray || !corners || !mask || !out || !iterations || !status || (uintptr_t)corners % elem != 0 ||
        (uintptr_t)out % elem != 0 || (uintptr_t)mask % 4 != 0 || (uintptr_t)iterations % 4 != 0 || (uintptr_t)status % 4 != 0) {
        set_error("camd_corner_sub_pix: bad arguments (gray, corners, mask, out, iterations, status: device arrays, aligned to an "
                  "element)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    SubpixArgs a = {};
    a.gray = gray, a.pitch = pitch, a.stride = stride, a.corners = corners, a.start = start, a.mask = mask, a.out = out;
    a.iterations = iterations, a.status = status, a.eps = eps, a.rows = (unsigned)rows;
    a.per_frame = (unsigned)(rows / (size_t)frames), a.w = w, a.h = h, a.frames = frames;
    a.win_w = win_w, a.win_h = win_h, a.max_iters = max_iters;
    const size_t lds = (size_t)4 * (2 * win_w + 3) * (2 * win_h + 3) * sizeof(float);
    with_float(corner_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_corner_sub_pix<T>), dim3(div_up((long long)rows, 4)), dim3(256), lds, (hipStream_t)queue, a);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_bgr_to_gray_u8(const uint8_t* src, int w, int h, size_t src_pitch, size_t src_stride, uint8_t* dst, size_t dst_pitch,
                        size_t dst_stride, int batch, int k0, int k1, int k2, int shift, void* queue)
{
    if (!src || !dst || w <= 0 || h <= 0 || batch <= 0 || src_pitch < (size_t)w * 3 || dst_pitch < (size_t)w ||
        (batch > 1 && (src_stride < (size_t)(h - 1) * src_pitch + (size_t)w * 3 || dst_stride < (size_t)(h - 1) * dst_pitch + (size_t)w)) ||
        shift < 1 || shift > 22 || k0 < 0 || k1 < 0 || k2 < 0 || (long long)k0 + k1 + k2 != (1LL << shift)) {
        set_error("camd_bgr_to_gray_u8: bad arguments (w, h, batch > 0; src_pitch >= 3 w, dst_pitch >= w, strides >= an image; "
                  "three weights >= 0 that add up to 1 << shift, shift 1 .. 22)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const bool aligned = ((uintptr_t)src | src_pitch | src_stride | (uintptr_t)dst | dst_pitch | dst_stride) % 4 == 0;
    const dim3 grid(div_up(div_up(w, 4), 256), h < 65535 ? h : 65535, batch < 65535 ? batch : 65535);
#define ARGS src, w, h, src_pitch, src_stride, dst, dst_pitch, dst_stride, batch, k0, k1, k2, shift
    if (aligned) hipLaunchKernelGGL((k_bgr_to_gray_u8<true>), grid, dim3(256), 0, (hipStream_t)queue, ARGS);
    else hipLaunchKernelGGL((k_bgr_to_gray_u8<false>), grid, dim3(256), 0, (hipStream_t)queue, ARGS);
#undef ARGS
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
