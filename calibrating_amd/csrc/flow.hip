// flow.hip -- flow_utils.warp_flow on 8-bit images for gfx950: an image moved through a dense optical flow.
//
// Replaces (file:line in /root/reference/calibrating/):
//   flow_utils.py:111-112,127-129  remap_xy + flow * [[[w]], [[h]]] -> float32 maps -> cv2.remap(img2, ...)   (backward)
//   flow_utils.py:111-125          round, mask, scatter of the source coordinates, cv2.remap(img1, ...)       (forward)
// The map position of pixel (x, y) is m = float64(x) + float64(flow_x) * float64(w) (and y, h): NumPy promotes the
// product with the Python list to float64 even for a float32 flow, so the product and the sum are each rounded once
// in float64 -- never fused.  No map reaches memory: the backward kernel samples straight from m (remap_sample.hpp,
// the sampler camd_remap_u8 uses), the forward kernels keep one int32 per target pixel.
#include "remap_sample.hpp"

namespace camd {

template <typename T>
__device__ __forceinline__ double flow_position(int i, T flow, int n)
{
    return __dadd_rn((double)i, __dmul_rn((double)flow, (double)n));
}

// cvRound of a float on x86 (cvtss2si) gives INT_MIN for NaN, the infinities and everything beyond int: a cell
// left of / above every image, so the pixel is the border.  v_cvt_i32_f32 saturates instead (and turns NaN into 0),
// hence the explicit test.  `v` is the map * 32, the number cv2 rounds (INTER_NEAREST rounds the map itself; where only
// the product leaves int its short saturation has put the pixel outside every image already, so one test serves).
__device__ __forceinline__ bool rounds_to_int(float v) { return v >= -2147483648.f && v < 2147483648.f; }

// Backward branch: dst(x, y) = img2 sampled at float32(m).  One lane per destination pixel; image z of the batch has
// its own flow.  KS = 8 Lanczos-4, 2 bilinear, 1 nearest.
template <int KS, int CN, typename T>
__global__ __launch_bounds__(256) void k_warp_backward(const uint8_t* __restrict__ src, size_t src_pitch,
                                                       size_t src_stride, const T* __restrict__ flow, size_t flow_stride,
                                                       uint8_t* __restrict__ dst, int w, int h, size_t dst_pitch,
                                                       size_t dst_stride, const int16_t* __restrict__ tab)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    const bool act = x < w;
    float mx = 0.f, my = 0.f;
    bool finite = false;
    if (act) {
        const T* f = flow + (size_t)z * flow_stride + (size_t)y * w + x;
        mx = __double2float_rn(flow_position(x, f[0], w));
        my = __double2float_rn(flow_position(y, f[(size_t)w * h], h));
        finite = rounds_to_int(mx * (float)INTER_TAB_SIZE) && rounds_to_int(my * (float)INTER_TAB_SIZE);
    }
    src += (size_t)z * src_stride;
    uint8_t* out = dst + (size_t)z * dst_stride + (size_t)y * dst_pitch + (size_t)x * CN;
    if constexpr (KS == 1) {
        if (!act) return;
        int sx, sy;
        map_to_nearest(mx, my, sx, sy);
        const bool ok = finite && (unsigned)sx < (unsigned)w && (unsigned)sy < (unsigned)h;
        const uint8_t* p = src + (ok ? (size_t)sy * src_pitch + (size_t)sx * CN : 0);
#pragma unroll
        for (int c = 0; c < CN; c++) out[c] = ok ? p[c] : 0;
    } else {
        int a = 0, ix = 0, iy = 0;
        if (finite) map_to_window<KS>(mx, my, a, ix, iy);
        uint32_t wreg[KS * KS / 2];
        fetch_weight_entry<KS>(tab, a, wreg);  // (every lane of the block: the Lanczos entry is fetched wave-wide)
        if (!act) return;
        if (!finite) ix = iy = -32768;  // no tap inside any image: the border, as on x86
        gather_pixel_batch<KS, CN, (KS == 8 ? 4 : KS)>(src, w, h, src_pitch, 0, ix, iy, wreg, out, 0, 1);
    }
}

// Forward branch, pass 1: source pixel (x, y) with a non-zero flow claims the pixel it rounds to.  Of several sources
// on one target NumPy's fancy assignment keeps the last in row-major order = the largest y * w + x, which atomicMax
// finds whatever order the lanes arrive in.  The range test is made on the rounded double: NaN, infinities and
// positions beyond int never reach the conversion and are skipped.
template <typename T>
__global__ __launch_bounds__(256) void k_warp_forward_claim(const T* __restrict__ flow, size_t flow_stride, int w, int h,
                                                            int* __restrict__ winner)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (x >= w) return;
    const T* f = flow + (size_t)z * flow_stride + (size_t)y * w + x;
    const T fx = f[0], fy = f[(size_t)w * h];
    if (fx == (T)0 && fy == (T)0) return;  // flow.any(0): -0.0 is zero, NaN is not
    const double tx = rint(flow_position(x, fx, w)), ty = rint(flow_position(y, fy, h));  // np.round: half to even
    if (!(tx >= 0.0 && tx < (double)w && ty >= 0.0 && ty < (double)h)) return;
    atomicMax(winner + (size_t)z * w * h + (size_t)(int)ty * w + (int)tx, y * w + x);
}

// Forward branch, pass 2: target pixel (x, y) shows the source that won it, or itself where nobody did -- the map
// holds integers only, so every interpolation of cv2.remap copies that pixel of img1 (phase 0 of the tables) or
// gives 0 where it lies outside img1, whose size need not be the flow's.
template <int CN>
__global__ __launch_bounds__(256) void k_warp_forward_copy(const uint8_t* __restrict__ src, int sw, int sh,
                                                           size_t src_pitch, size_t src_stride,
                                                           const int* __restrict__ winner, uint8_t* __restrict__ dst,
                                                           int w, int h, size_t dst_pitch, size_t dst_stride)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (x >= w) return;
    const int own = y * w + x, won = winner[(size_t)z * w * h + own], s = won >= 0 ? won : own;
    const int sy = s / w, sx = s - sy * w;
    const bool ok = sx < sw && sy < sh;
    const uint8_t* p = src + (size_t)z * src_stride + (ok ? (size_t)sy * src_pitch + (size_t)sx * CN : 0);
    uint8_t* out = dst + (size_t)z * dst_stride + (size_t)y * dst_pitch + (size_t)x * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) out[c] = ok ? p[c] : 0;
}

static int check_warp(const char* fn, const void* img, int sw, int sh, int cn, size_t src_pitch, const void* flow,
                      int flow_type, const void* dst, int w, int h, size_t dst_pitch, int interp, int batch)
{
    if (!img || !flow || !dst || sw <= 0 || sh <= 0 || w <= 0 || h <= 0 || batch <= 0 || batch > 65535 ||
        !float_type_ok(flow_type)) {
        set_error("%s: bad arguments", fn);
        return CAMD_ERR_BAD_ARG;
    }
    if (cn != 1 && cn != 3) {
        set_error("%s: %d channels; images have 1 or 3", fn, cn);
        return CAMD_ERR_BAD_ARG;
    }
    if (src_pitch < (size_t)sw * cn || dst_pitch < (size_t)w * cn) {
        set_error("%s: a pitch is shorter than its row", fn);
        return CAMD_ERR_BAD_ARG;
    }
    if (sw >= 32768 || sh >= 32768 || w >= 32768 || h >= 32768) {
        set_error("%s: a side of %d x %d / %d x %d reaches 32768; cv2.remap's coordinates are shorts", fn, sw, sh, w, h);
        return CAMD_ERR_BAD_ARG;
    }
    if ((long long)w * h > 2147483647LL) {
        set_error("%s: %d x %d pixels; a pixel index must fit an int32", fn, w, h);
        return CAMD_ERR_BAD_ARG;
    }
    if (interp != CAMD_INTER_NEAREST && interp != CAMD_INTER_LINEAR && interp != CAMD_INTER_LANCZOS4) {
        set_error("%s: interpolation %d not implemented", fn, interp);
        return CAMD_ERR_UNSUPPORTED;
    }
    CAMD_NEED_DEVICE();
    return CAMD_OK;
}

template <typename T>
static int warp_backward(const uint8_t* img2, int cn, size_t src_pitch, size_t src_stride, const T* flow,
                         size_t flow_stride, uint8_t* dst, int w, int h, size_t dst_pitch, size_t dst_stride, int interp,
                         int batch, hipStream_t st)
{
    const int16_t *tl = nullptr, *tb = nullptr;
    const int rc = get_tables(&tl, &tb);
    if (rc != CAMD_OK) return rc;
    const dim3 grid(div_up(w, 256), h, batch), block(256);
#define WARP(KS, CN, TAB)                                                                                          \
    hipLaunchKernelGGL((k_warp_backward<KS, CN, T>), grid, block, 0, st, img2, src_pitch, src_stride, flow, flow_stride, \
                       dst, w, h, dst_pitch, dst_stride, TAB)
    if (interp == CAMD_INTER_LANCZOS4) {
        if (cn == 1) WARP(8, 1, tl);
        else WARP(8, 3, tl);
    } else if (interp == CAMD_INTER_LINEAR) {
        if (cn == 1) WARP(2, 1, tb);
        else WARP(2, 3, tb);
    } else {
        if (cn == 1) WARP(1, 1, tb);  // (nearest reads no table)
        else WARP(1, 3, tb);
    }
#undef WARP
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_warp_flow_backward_u8(const uint8_t* img2, int cn, size_t src_pitch, size_t src_stride, const void* flow,
                               int flow_type, size_t flow_stride, uint8_t* dst, int w, int h, size_t dst_pitch,
                               size_t dst_stride, int interp, int batch, void* stream)
{
    const int rc = check_warp("camd_warp_flow_backward_u8", img2, w, h, cn, src_pitch, flow, flow_type, dst, w, h, dst_pitch,
                              interp, batch);
    if (rc != CAMD_OK) return rc;
    return with_float(flow_type, [&](auto v) {
        using T = decltype(v);
        return warp_backward(img2, cn, src_pitch, src_stride, (const T*)flow, flow_stride, dst, w, h, dst_pitch, dst_stride,
                             interp, batch, (hipStream_t)stream);
    });
}

int camd_warp_flow_forward_u8(const uint8_t* img1, int sw, int sh, int cn, size_t src_pitch, size_t src_stride,
                              const void* flow, int flow_type, size_t flow_stride, uint8_t* dst, int w, int h,
                              size_t dst_pitch, size_t dst_stride, int interp, int32_t* winner_ws, int batch, void* stream)
{
    const int rc = check_warp("camd_warp_flow_forward_u8", img1, sw, sh, cn, src_pitch, flow, flow_type, dst, w, h, dst_pitch,
                              interp, batch);
    if (rc != CAMD_OK) return rc;
    if (!winner_ws) { set_error("camd_warp_flow_forward_u8: NULL workspace"); return CAMD_ERR_BAD_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(div_up(w, 256), h, batch), block(256);
    CAMD_HIP(hipMemsetAsync(winner_ws, 0xff, (size_t)batch * w * h * sizeof(int32_t), st));  // -1: nobody yet
    with_float(flow_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_warp_forward_claim<T>), grid, block, 0, st, (const T*)flow, flow_stride, w, h, winner_ws);
    });
    if (cn == 1)
        hipLaunchKernelGGL((k_warp_forward_copy<1>), grid, block, 0, st, img1, sw, sh, src_pitch, src_stride, winner_ws, dst, w,
                           h, dst_pitch, dst_stride);
    else
        hipLaunchKernelGGL((k_warp_forward_copy<3>), grid, block, 0, st, img1, sw, sh, src_pitch, src_stride, winner_ws, dst, w,
                           h, dst_pitch, dst_stride);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
