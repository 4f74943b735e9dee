// remap.hip -- cv2.remap / cv2.undistort on 8-bit images for gfx950.
//
// Replaces (file:line in /root/reference/calibrating/):
//   stereo_camera.py:217-228  cv2.remap(img, mapx, mapy, cv2.INTER_LANCZOS4)       (rectify, x2)
//   stereo_camera.py:230-240  the x-translation of rectify_img2 (x_shift, fused)
//   stereo_camera.py:430-431  cv2.undistort(img1, K, D)   (bilinear through 1/32-px fixed maps)
// Arithmetic follows OpenCV's 8-bit fixed-point remap: 1/32-pixel phases, 15-bit int16 weights from
// a 32x32-entry table (sum forced to 32768), int32 accumulate, (sum + 16384) >> 15, BORDER_CONSTANT 0.
// The sampler itself lives in remap_sample.hpp (flow.hip samples through it too); the tables are built here.
#include "remap_sample.hpp"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

namespace camd {

static inline short sat_short(int v) { return (short)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }

// ---- fixed-point interpolation tables (host, built once per process and option value) ------------------------
// The table of a KS-tap kernel has 32 x 32 entries (one per 1/32-pixel phase pair), each KS*KS int16 weights
// = round(wy[ky] * wx[kx] * 32768) whose sum is then forced to exactly 32768.
//
// U15: which taps take that correction is a process-wide option shared with the oracle's switch
// of the same name, so the two cannot drift apart: the correction looks at the 2x2 taps (k1, k2) in
// [lo, lo+2) x [lo, lo+2) of the entry, adds the missing weight to the largest of them or removes the excess from
// the smallest.  lo = KS/2 by default (OpenCV's loop bounds as recalled; 4 for Lanczos-4), settable to KS/2 - 1
// through camd_set_global_option(CAMD_GOPT_LANCZOS_FIX_GROUP_LO, 3).
static int g_fix_group_lo8 = 4;

// Phase table of the 1-D kernels, [32][KS] float32.
static std::vector<float> phase_weights(int ks)
{
    std::vector<float> w((size_t)INTER_TAB_SIZE * ks);
    if (ks == 2) {  // bilinear: (1 - t, t)
        for (int p = 0; p < INTER_TAB_SIZE; p++) {
            const float t = p * (1.f / INTER_TAB_SIZE);
            w[p * 2] = 1.f - t;
            w[p * 2 + 1] = t;
        }
        return w;
    }
    // Lanczos-4, taps at offsets -3..4 from the integer position: w_k ~ sin(pi d) sin(pi d / 4) / d^2 with
    // d = t + 3 - k, evaluated the way OpenCV does -- sin(pi d) sin(pi d/4) is expanded into the sine and
    // cosine of ONE angle a = -(t+3) pi/4 with a table of eighth-turn rotations, in double, divided by (pi d / 4)^2,
    // rounded to float; a tap the sample falls on (|d| < 1e-6) gets 1e30; the eight floats are then scaled by the
    // float reciprocal of their float sum.
    const double q = 0.70710678118654752440084436210485, pi4 = 3.1415926535897932384626433832795 * 0.25;
    const double rot[8][2] = {{1, 0}, {-q, -q}, {0, 1}, {q, -q}, {-1, 0}, {q, q}, {0, -1}, {-q, q}};
    for (int p = 0; p < INTER_TAB_SIZE; p++) {
        const float t = p * (1.f / INTER_TAB_SIZE);
        const double a = -(t + 3) * pi4, sa = std::sin(a), ca = std::cos(a);
        float* o = &w[(size_t)p * 8];
        float total = 0;
        for (int k = 0; k < 8; k++) {
            const float d = t + 3 - k;
            if (std::fabs(d) < 1e-6f) o[k] = 1e30f;
            else {
                const double y = -d * pi4;
                o[k] = (float)((rot[k][0] * sa + rot[k][1] * ca) / (y * y));
            }
            total += o[k];
        }
        const float inv = 1.f / total;
        for (int k = 0; k < 8; k++) o[k] *= inv;
    }
    return w;
}

// [32*32][ks*ks] int16.  The correction of an entry is applied right after the entry is quantised, while the
// entries behind it are still zero: for the 2x2 table the window [lo, lo+2)^2 = [1, 3)^2 reaches past the entry
// into that zero region (as in cv2's builder), where it can only ever fire at phase (0,0) -- the weight 32768
// saturates to 32767 and the missing 1 lands on tap (1,1).
static void build_itab(int ks, int16_t* itab)
{
    const std::vector<float> w = phase_weights(ks);
    const int n = ks * ks, lo = ks == 8 ? g_fix_group_lo8 : ks / 2;
    const long total = (long)INTER_TAB_SIZE * INTER_TAB_SIZE * n;
    std::fill(itab, itab + total, (int16_t)0);
    for (int py = 0; py < INTER_TAB_SIZE; py++)
        for (int px = 0; px < INTER_TAB_SIZE; px++) {
            int16_t* e = itab + ((long)py * INTER_TAB_SIZE + px) * n;
            int sum = 0;
            for (int ky = 0; ky < ks; ky++)
                for (int kx = 0; kx < ks; kx++) {
                    const float v = w[py * ks + ky] * w[px * ks + kx];
                    sum += e[ky * ks + kx] = sat_short((int)lrintf(v * COEF_SCALE));
                }
            const int excess = sum - COEF_SCALE;
            if (excess == 0) continue;
            // largest / smallest tap of the 2x2 group, first one wins on ties (scan order ky, kx)
            const long room = total - (e - itab);
            int big = lo * ks + lo, small = big;
            for (int ky = lo; ky < lo + 2; ky++)
                for (int kx = lo; kx < lo + 2; kx++) {
                    const int i = ky * ks + kx;
                    if (i >= room) continue;
                    if (e[i] < e[small]) small = i;
                    else if (e[i] > e[big]) big = i;
                }
            const int at = excess < 0 ? big : small;
            e[at] = (short)(e[at] - excess);
        }
}

// device copies of the tables, one set per device, created on first use
struct DevTables {
    int16_t* lanczos = nullptr;
    int16_t* bilinear = nullptr;
};
static std::mutex g_tab_mutex;
static DevTables g_tabs[64];

int get_tables(const int16_t** lanczos, const int16_t** bilinear)
{
    int dev = 0;
    CAMD_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) { set_error("device index %d out of range", dev); return CAMD_ERR_HIP; }
    std::lock_guard<std::mutex> lock(g_tab_mutex);
    DevTables& t = g_tabs[dev];
    if (!t.lanczos) {
        std::vector<int16_t> hl(1024 * 64), hb(1024 * 4);
        build_itab(8, hl.data());
        build_itab(2, hb.data());
        int16_t *dl = nullptr, *db = nullptr;
        CAMD_HIP(hipMalloc((void**)&dl, hl.size() * 2));
        CAMD_HIP(hipMalloc((void**)&db, hb.size() * 2));
        CAMD_HIP(hipMemcpy(dl, hl.data(), hl.size() * 2, hipMemcpyHostToDevice));
        CAMD_HIP(hipMemcpy(db, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
        t.lanczos = dl;
        t.bilinear = db;
    }
    *lanczos = t.lanczos;
    *bilinear = t.bilinear;
    return CAMD_OK;
}

// cv2.remap with CV_32FC1 maps; blockIdx.z owns `zb` consecutive images of the batch.
#ifndef CAMD_REMAP_ROWS_PER_FETCH
#define CAMD_REMAP_ROWS_PER_FETCH 4
#endif
template <int KS, int CN, int HR = (KS == 8 ? CAMD_REMAP_ROWS_PER_FETCH : KS)>
__global__ __launch_bounds__(256, KS != 8 ? 1 : HR == 8 ? 4 : HR == 4 ? 6 : 7)
void k_remap_f32(const uint8_t* __restrict__ src, int sw, int sh, size_t src_pitch, size_t src_stride,
                 const float* __restrict__ mapx, const float* __restrict__ mapy, uint8_t* __restrict__ dst, int dw,
                 int dh, size_t dst_pitch, size_t dst_stride, const int16_t* __restrict__ tab, int x_shift, int batch,
                 int zb)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, xm = x - x_shift;
    const int z0 = blockIdx.z * zb, nz = min(zb, batch - z0);
    const bool act = x < dw && xm >= 0 && xm < dw;
    int a = 0, ix = 0, iy = 0;
    if (act) {
        const size_t mi = (size_t)y * dw + xm;
        map_to_window<KS>(mapx[mi], mapy[mi], a, ix, iy);
    }
    uint32_t wreg[KS * KS / 2];
    fetch_weight_entry<KS>(tab, a, wreg);
    if (x >= dw) return;
    uint8_t* out = dst + (size_t)z0 * dst_stride + (size_t)y * dst_pitch + (size_t)x * CN;
    if (!act) {  // the columns the x-shift leaves empty
        for (int z = 0; z < nz; z++, out += dst_stride) {
#pragma unroll
            for (int c = 0; c < CN; c++) out[c] = 0;
        }
        return;
    }
    gather_pixel_batch<KS, CN, HR>(src + (size_t)z0 * src_stride, sw, sh, src_pitch, src_stride, ix, iy, wreg, out,
                                   dst_stride, nz);
}

template <int CN>
__global__ __launch_bounds__(256) void k_remap_nearest_u8(const uint8_t* __restrict__ src, int sw, int sh,
                                                          size_t src_pitch, size_t src_stride,
                                                          const float* __restrict__ mapx,
                                                          const float* __restrict__ mapy,
                                                          uint8_t* __restrict__ dst, int dw, int dh,
                                                          size_t dst_pitch, size_t dst_stride, int x_shift)
{
    int x = blockIdx.x * 256 + threadIdx.x;
    int y = blockIdx.y;
    if (x >= dw) return;
    uint8_t* out = dst + (size_t)blockIdx.z * dst_stride + (size_t)y * dst_pitch + (size_t)x * CN;
    int xm = x - x_shift;
    bool ok = xm >= 0 && xm < dw;
    int sx = 0, sy = 0;
    if (ok) {
        size_t mi = (size_t)y * dw + xm;
        map_to_nearest(mapx[mi], mapy[mi], sx, sy);
        ok = (unsigned)sx < (unsigned)sw && (unsigned)sy < (unsigned)sh;
    }
    const uint8_t* p = src + (size_t)blockIdx.z * src_stride + (size_t)sy * src_pitch + (size_t)sx * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) out[c] = ok ? p[c] : 0;
}

template <int CN>
__global__ __launch_bounds__(256) void k_remap_fixed_bilinear(const uint8_t* __restrict__ src, int sw, int sh,
                                                              size_t src_pitch, size_t src_stride,
                                                              const int16_t* __restrict__ mapxy,
                                                              const uint16_t* __restrict__ mapa,
                                                              uint8_t* __restrict__ dst, int dw, int dh,
                                                              size_t dst_pitch, size_t dst_stride,
                                                              const int16_t* __restrict__ tab, int batch, int zb)
{
    int x = blockIdx.x * 256 + threadIdx.x;
    int y = blockIdx.y;
    if (x >= dw) return;
    const int z0 = blockIdx.z * zb, nz = min(zb, batch - z0);
    size_t mi = (size_t)y * dw + x;
    int ix = mapxy[mi * 2], iy = mapxy[mi * 2 + 1];
    int a = mapa[mi] & (INTER_TAB_SIZE * INTER_TAB_SIZE - 1);
    const uint32_t* e = reinterpret_cast<const uint32_t*>(tab + (size_t)a * 4);
    const uint32_t wreg[2] = {e[0], e[1]};
    gather_pixel_batch<2, CN, 2>(src + (size_t)z0 * src_stride, sw, sh, src_pitch, src_stride, ix, iy, wreg,
                                 dst + (size_t)z0 * dst_stride + (size_t)y * dst_pitch + (size_t)x * CN, dst_stride, nz);
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_set_global_option(int option, int value)
{
    if (option == CAMD_GOPT_LANCZOS_FIX_GROUP_LO && (value == 3 || value == 4)) {
        std::lock_guard<std::mutex> lock(g_tab_mutex);
        if (value != g_fix_group_lo8) {
            g_fix_group_lo8 = value;
            for (DevTables& t : g_tabs) {  // rebuilt on next use (the old copies may still be read by running kernels)
                t.lanczos = nullptr;
                t.bilinear = nullptr;
            }
        }
        return CAMD_OK;
    }
    set_error("unknown global option %d / value %d", option, value);
    return CAMD_ERR_BAD_ARG;
}

int camd_lanczos4_table_host(int16_t* tab)
{
    if (!tab) { set_error("NULL table"); return CAMD_ERR_BAD_ARG; }
    build_itab(8, tab);
    return CAMD_OK;
}

int camd_bilinear_table_host(int16_t* tab)
{
    if (!tab) { set_error("NULL table"); return CAMD_ERR_BAD_ARG; }
    build_itab(2, tab);
    return CAMD_OK;
}

int camd_remap_u8(const uint8_t* src, int sw, int sh, int cn, size_t src_pitch, size_t src_stride,
                  const float* mapx, const float* mapy, uint8_t* dst, int dw, int dh, size_t dst_pitch,
                  size_t dst_stride, int interp, int x_shift, int batch, void* stream)
{
    if (!src || !mapx || !mapy || !dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || batch <= 0 ||
        (cn != 1 && cn != 3) || src_pitch < (size_t)sw * cn || dst_pitch < (size_t)dw * cn) {
        set_error("camd_remap_u8: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const int16_t *tl = nullptr, *tb = nullptr;
    const int rc = get_tables(&tl, &tb);
    if (rc != CAMD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(div_up(dw, 256), dh, batch), block(256);
    const int zb = images_per_group(grid.x * grid.y, batch);
    const dim3 gridz(grid.x, grid.y, div_up(batch, zb));
#define ARGS src, sw, sh, src_pitch, src_stride, mapx, mapy, dst, dw, dh, dst_pitch, dst_stride
    if (interp == CAMD_INTER_LANCZOS4) {
        if (cn == 1) hipLaunchKernelGGL((k_remap_f32<8, 1>), gridz, block, 0, st, ARGS, tl, x_shift, batch, zb);
        else hipLaunchKernelGGL((k_remap_f32<8, 3>), gridz, block, 0, st, ARGS, tl, x_shift, batch, zb);
    } else if (interp == CAMD_INTER_LINEAR) {
        if (cn == 1) hipLaunchKernelGGL((k_remap_f32<2, 1>), gridz, block, 0, st, ARGS, tb, x_shift, batch, zb);
        else hipLaunchKernelGGL((k_remap_f32<2, 3>), gridz, block, 0, st, ARGS, tb, x_shift, batch, zb);
    } else if (interp == CAMD_INTER_NEAREST) {
        if (cn == 1) hipLaunchKernelGGL((k_remap_nearest_u8<1>), grid, block, 0, st, ARGS, x_shift);
        else hipLaunchKernelGGL((k_remap_nearest_u8<3>), grid, block, 0, st, ARGS, x_shift);
    } else {
        set_error("camd_remap_u8: interpolation %d not implemented", interp);
        return CAMD_ERR_UNSUPPORTED;
    }
#undef ARGS
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_remap_fixed_bilinear_u8(const uint8_t* src, int sw, int sh, int cn, size_t src_pitch,
                                 size_t src_stride, const int16_t* mapxy, const uint16_t* mapa, uint8_t* dst,
                                 int dw, int dh, size_t dst_pitch, size_t dst_stride, int batch, void* stream)
{
    if (!src || !mapxy || !mapa || !dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || batch <= 0 ||
        (cn != 1 && cn != 3) || src_pitch < (size_t)sw * cn || dst_pitch < (size_t)dw * cn) {
        set_error("camd_remap_fixed_bilinear_u8: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const int16_t *tl = nullptr, *tb = nullptr;
    const int rc = get_tables(&tl, &tb);
    if (rc != CAMD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int zb = images_per_group(div_up(dw, 256) * dh, batch);
    dim3 grid(div_up(dw, 256), dh, div_up(batch, zb)), block(256);
    if (cn == 1)
        hipLaunchKernelGGL((k_remap_fixed_bilinear<1>), grid, block, 0, st, src, sw, sh, src_pitch, src_stride,
                           mapxy, mapa, dst, dw, dh, dst_pitch, dst_stride, tb, batch, zb);
    else
        hipLaunchKernelGGL((k_remap_fixed_bilinear<3>), grid, block, 0, st, src, sw, sh, src_pitch, src_stride,
                           mapxy, mapa, dst, dw, dh, dst_pitch, dst_stride, tb, batch, zb);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
