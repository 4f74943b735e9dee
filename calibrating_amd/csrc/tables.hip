// tables.hip -- the rig's lookup tables built on the GPU: cv2.initUndistortRectifyMap
// (CV_32FC1 maps, stereo_camera.py:159-165 and utils.py:184-191) with the rectify valid mask
// (stereo_camera.py:167-176) fused, and the CV_16SC2 + CV_16UC1 maps cv2.undistort builds internally
// (stereo_camera.py:430-431).  Bit-identical to the host construction (geometry.py; camd_undistort_maps_host at the
// end of this file runs the kernel's own per-pixel functions, camera_model.hpp) and to the oracle: float64, no
// contraction (-ffp-contract=off), correctly rounded division.
//
// OpenCV accumulates X, Y, W along a row by repeated addition (_x += ir[0] ...).  That recurrence is the
// only sequential part: a workgroup owns one row, three of its lanes run the three chains for a chunk of
// columns into LDS (a few microseconds; all rows run in parallel), then all 256 lanes do the per-pixel
// distortion arithmetic from LDS.
#include "camera_model.hpp"

namespace camd {

struct TableArgs {
    Pinhole cam;     // camera matrix of the SOURCE image
    Lens k;
    double New[9];   // new camera matrix * R (its inverse maps destination pixels to rays)
    int w, h;        // destination size
    int src_w, src_h;  // valid-mask bounds (mask != nullptr)
    int stripe;      // fixed-point variant: rows per stripe (cv2.undistort folds the stripe offset into cy)
};

static constexpr int TAB_CHUNK = 1024;  // columns per chunk: 3 x 8 KB of LDS

// FIXED = false: float maps (+ optional mask).  FIXED = true: int16 (x, y) + uint16 phase maps, row stripes.
template <bool FIXED>
__global__ __launch_bounds__(256) void k_undistort_rectify_map(TableArgs a, float* __restrict__ mapx,
                                                               float* __restrict__ mapy, uint8_t* __restrict__ mask,
                                                               int16_t* __restrict__ mapxy, uint16_t* __restrict__ mapa)
{
    __shared__ double sX[TAB_CHUNK], sY[TAB_CHUNK], sW[TAB_CHUNK];
    __shared__ double carry[3];
    const int row = blockIdx.x;
    double ir[9];
    int i = row;
    if (FIXED) {
        const int y0 = row - row % a.stripe;
        stripe_inverse(a.New, y0, ir);
        i = row - y0;
    } else {
        inv3(a.New, ir);
    }
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        carry[c] = i * ir[3 * c + 1] + ir[3 * c + 2];
    }
    for (int j0 = 0; j0 < a.w; j0 += TAB_CHUNK) {
        const int n = min(TAB_CHUNK, a.w - j0);
        if (threadIdx.x < 3) {
            const int c = threadIdx.x;
            double* dst = c == 0 ? sX : (c == 1 ? sY : sW);
            const double step = ir[3 * c];
            double acc = carry[c];
            for (int j = 0; j < n; j++) {
                dst[j] = acc;
                acc += step;
            }
            carry[c] = acc;
        }
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += 256) {
            const size_t o = (size_t)row * a.w + j0 + j;
            if (FIXED) {
                ray_to_fixed_cell(a.cam, a.k, sX[j], sY[j], sW[j], mapxy + o * 2, mapa + o);
            } else {
                double u, v;
                ray_to_pixel(a.cam, a.k, sX[j], sY[j], sW[j], u, v);
                const float fu = (float)u, fv = (float)v;
                mapx[o] = fu;
                mapy[o] = fv;
                if (mask)  // stereo_camera.py:167-176: (-0.5 < mapx) & (mapx < w - 0.5) & (-0.5 < mapy) & (mapy < h - 0.5)
                    mask[o] = (-0.5f < fu && fu < (float)a.src_w - 0.5f && -0.5f < fv && fv < (float)a.src_h - 0.5f) ? 1 : 0;
            }
        }
        __syncthreads();
    }
}

static int fill_args(TableArgs* a, const double A[9], const double* dist, int ndist, int w, int h, const char* who)
{
    if (!A || w <= 0 || h <= 0 || ndist < 0 || ndist > 14 || (ndist > 0 && !dist)) {
        set_error("%s: bad arguments", who);
        return CAMD_ERR_BAD_ARG;
    }
    const int rc = unpack_camera(who, A, dist, ndist, &a->cam, &a->k);
    if (rc != CAMD_OK) return rc;
    a->w = w;
    a->h = h;
    a->src_w = a->src_h = 0;
    a->stripe = undistort_stripe_rows(w, h);
    return CAMD_OK;
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_init_undistort_rectify_map(const double A[9], const double* dist, int ndist, const double* R,
                                    const double Anew[9], int w, int h, float* mapx, float* mapy,
                                    uint8_t* valid_mask, int src_w, int src_h, void* stream)
{
    TableArgs a;
    int rc = fill_args(&a, A, dist, ndist, w, h, "camd_init_undistort_rectify_map");
    if (rc != CAMD_OK) return rc;
    if (!Anew || !mapx || !mapy) { set_error("camd_init_undistort_rectify_map: NULL argument"); return CAMD_ERR_BAD_ARG; }
    CAMD_NEED_DEVICE();
    static const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double* Rm = R ? R : I3;
    for (int i = 0; i < 3; i++)  // Anew * R, the accumulation order of a plain triple loop (s = 0; s += a*b)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int q = 0; q < 3; q++) s += Anew[i * 3 + q] * Rm[q * 3 + j];
            a.New[i * 3 + j] = s;
        }
    a.src_w = src_w;
    a.src_h = src_h;
    hipLaunchKernelGGL((k_undistort_rectify_map<false>), dim3(h), dim3(256), 0, (hipStream_t)stream, a, mapx, mapy,
                       valid_mask, (int16_t*)nullptr, (uint16_t*)nullptr);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_undistort_maps(const double K[9], const double* dist, int ndist, int w, int h, int16_t* mapxy,
                        uint16_t* mapa, void* stream)
{
    TableArgs a;
    int rc = fill_args(&a, K, dist, ndist, w, h, "camd_undistort_maps");
    if (rc != CAMD_OK) return rc;
    if (!mapxy || !mapa) { set_error("camd_undistort_maps: NULL argument"); return CAMD_ERR_BAD_ARG; }
    CAMD_NEED_DEVICE();
    for (int i = 0; i < 9; i++) a.New[i] = K[i];
    hipLaunchKernelGGL((k_undistort_rectify_map<true>), dim3(h), dim3(256), 0, (hipStream_t)stream, a, (float*)nullptr,
                       (float*)nullptr, (uint8_t*)nullptr, mapxy, mapa);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

// the same maps on the host: one text with the kernel (camera_model.hpp), the row recurrence a plain loop
int camd_undistort_maps_host(const double K[9], const double* dist, int ndist, int w, int h, int16_t* mapxy,
                             uint16_t* mapa)
{
    if (!mapxy || !mapa) { set_error("camd_undistort_maps_host: bad arguments"); return CAMD_ERR_BAD_ARG; }
    TableArgs a;
    const int rc = fill_args(&a, K, dist, ndist, w, h, "camd_undistort_maps_host");
    if (rc != CAMD_OK) return rc;
    for (int y0 = 0; y0 < h; y0 += a.stripe) {
        double ir[9];
        stripe_inverse(K, y0, ir);
        for (int i = 0; i < a.stripe && y0 + i < h; i++) {
            double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
            const size_t o = (size_t)(y0 + i) * w;
            for (int j = 0; j < w; j++, _x += ir[0], _y += ir[3], _w += ir[6])
                ray_to_fixed_cell(a.cam, a.k, _x, _y, _w, mapxy + (o + j) * 2, mapa + o + j);
        }
    }
    return CAMD_OK;
}

}  // extern "C"
