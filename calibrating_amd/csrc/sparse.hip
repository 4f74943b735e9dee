// sparse.hip -- sparse (u, v, z) samples <-> dense images: the family behind the reference's FeatureMatchingAsStereoMatching
// (stereo_matching.py:113-142) and MatchingByBoard:
//   utils.uvzs_to_arr2d        (utils.py:291-317)   scatter with NumPy's last-write-wins
//   utils.arr2d_to_uvzs        (utils.py:320-329)   image -> (x, y, value) rows, all pixels or the masked ones
//   utils.interpolate_uvzs     (utils.py:356-415)   "nearest": SciPy KDTree.query per pixel  -> bins + bounded window search
//                                                    "lstsq":   np.linalg.lstsq plane       -> nine sums + evaluation
//   epipolar_geometry.matched_xyz_normals_to_zs (:88-97) with uvs_to_xyz_noramls (:84-85): depth of matches along both rays
// float64 like the reference's NumPy; products and sums are individually rounded (-ffp-contract=off) except where a
// fused multiply-add is written out.  Nothing here depends on the order in which atomics are served: the scatter keeps
// an integer maximum, the bins are filled in any order and searched by the key (distance, index), the plane sums are
// reduced in a fixed order without float atomics.
#include "common.hpp"
#include "compact.hpp"
#include "nearest.hpp"
#include "triangulate.hpp"

#include <cmath>

namespace camd {

// ---- a. scatter ------------------------------------------------------------------------------------------------------
// xs, ys = np.int32(uvs.round()) (half to even); rows outside the image -- NaN and inf among them -- are dropped (:312-313)
__device__ __forceinline__ bool sp_pixel(const double* __restrict__ uv, size_t i, int stride, int w, int h, size_t* pix)
{
    const double ru = rint(uv[i * stride]), rv = rint(uv[i * stride + 1]);
    if (!(ru >= 0.0 && ru < (double)w && rv >= 0.0 && rv < (double)h)) return false;
    *pix = (size_t)(int)rv * w + (int)ru;
    return true;
}

// owner[pix] = 1 + the largest row index landing there: arr2d[ys, xs] = values assigns in row order, the last one stays
__global__ __launch_bounds__(256) void k_sp_owner(const double* __restrict__ uv, size_t n, int stride, int w, int h,
                                                  uint32_t* __restrict__ owner)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    size_t pix;
    if (sp_pixel(uv, i, stride, w, h, &pix)) atomicMax(owner + pix, (uint32_t)i + 1u);
}

// ---- b. arr2d_to_uvzs ------------------------------------------------------------------------------------------------
// np.array([xs, ys, arr2d]).T.reshape(-1, 3): row r = x * h + y holds (x, y, arr2d[y, x]).  O = double or int64: what
// NumPy's promotion of the int64 grids with arr2d gives; the caller hands arr2d over in that type.
template <typename O>
__global__ __launch_bounds__(256) void k_sp_all_rows(const O* __restrict__ arr, int w, int h, O* __restrict__ rows)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (size_t)w * h) return;
    const int x = (int)(r / (size_t)h), y = (int)(r % (size_t)h);
    rows[r * 3 + 0] = (O)x;
    rows[r * 3 + 1] = (O)y;
    rows[r * 3 + 2] = arr[(size_t)y * w + x];
}

// np.array([xs[mask], ys[mask], arr2d[mask]]).T: the masked pixels in row-major order, as a compaction (compact.hpp)
template <typename O>
struct MaskRows : MaskOn {
    const O* arr;
    O* rows;
    __device__ __forceinline__ void emit(int x, int y, unsigned long long pos) const
    {
        rows[pos * 3 + 0] = (O)x;
        rows[pos * 3 + 1] = (O)y;
        rows[pos * 3 + 2] = arr[(size_t)y * w + x];
    }
};

// ---- c. nearest fill -------------------------------------------------------------------------------------------------
// (the bins, SpBins, and the search of one pixel through them, sp_nearest_value, live in nearest.hpp: lidar.hip searches too)
__device__ __forceinline__ bool sp_cell(const double* __restrict__ uv, size_t i, int stride, const SpBins& b, uint32_t* cell)
{
    const double fu = floor(uv[i * stride]), fv = floor(uv[i * stride + 1]);
    if (!(fu >= (double)-b.R && fu <= (double)(b.w + b.R - 2) && fv >= (double)-b.R && fv <= (double)(b.h + b.R - 2)))
        return false;  // (also NaN / inf)
    *cell = (uint32_t)((int)fv + b.R) * (uint32_t)b.bw + (uint32_t)((int)fu + b.R);
    return true;
}

__global__ __launch_bounds__(256) void k_sp_bin_count(const double* __restrict__ uv, size_t n, int stride, SpBins b,
                                                      uint32_t* __restrict__ counts)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t cell;
    if (sp_cell(uv, i, stride, b, &cell)) atomicAdd(counts + cell, 1u);
}

// cursor starts as the exclusive scan of the counts; the slot order inside a cell is whatever the atomics give
__global__ __launch_bounds__(256) void k_sp_bin_fill(const double* __restrict__ uv, size_t n, int stride, SpBins b,
                                                     uint32_t* __restrict__ cursor, size_t capacity,
                                                     double* __restrict__ sorted_uv, uint32_t* __restrict__ sorted_idx)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t cell;
    if (!sp_cell(uv, i, stride, b, &cell)) return;
    const uint32_t slot = atomicAdd(cursor + cell, 1u);
    if (slot >= capacity) return;
    sorted_uv[(size_t)slot * 2 + 0] = uv[i * stride];
    sorted_uv[(size_t)slot * 2 + 1] = uv[i * stride + 1];
    sorted_idx[slot] = (uint32_t)i;
}

struct SpOut {
    int ow, oh;        // the image written; == the grid unless upsized
    int scaled;
    double ifx, ify;   // cv2.resize(INTER_NEAREST): sx = min(floor(x * ifx), w - 1), as pc_sample in pointcloud.hip
    float mul, div;    // stereo_matching.py:139: disparity * hw[1] / resize_shape[1], two float32 roundings
};

// One thread per output pixel, a wave = 64 consecutive pixels of a row: neighbouring lanes walk the same cells.
template <typename Z>
__global__ __launch_bounds__(256) void k_sp_nearest(const double* __restrict__ sorted_uv, const uint32_t* __restrict__ sorted_idx,
                                                    const uint32_t* __restrict__ start, const Z* __restrict__ z, SpBins b,
                                                    double distance, SpOut o, float* __restrict__ out)
{
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y;
    if (X >= o.ow) return;
    int x = X, y = Y;
    if (o.scaled) {
        x = min((int)floor(X * o.ifx), b.w - 1);
        y = min((int)floor(Y * o.ify), b.h - 1);
    }
    float v = sp_nearest_value(sorted_uv, sorted_idx, start, z, 1, b, distance, x, y);
    if (o.scaled) v = __fdiv_rn(__fmul_rn(v, o.mul), o.div);
    out[(size_t)Y * o.ow + X] = v;
}

// ---- d. plane fit ----------------------------------------------------------------------------------------------------
// sums: 0 uu  1 uv  2 u  3 vv  4 v  5 n  6 uz  7 vz  8 z.  Thread t of block g adds rows g*256+t, +G*256, ... in that
// order; the block adds its 256 threads by a fixed tree (block_tree, compact.hpp); k_sp_plane_final adds the G partials in index order.
template <typename Z>
__global__ __launch_bounds__(256) void k_sp_plane_partials(const double* __restrict__ uv, int stride, const Z* __restrict__ z,
                                                           size_t n, double* __restrict__ partials)
{
    __shared__ double sh[256];
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double u = uv[i * stride], v = uv[i * stride + 1], zz = (double)z[i];
        s[0] += u * u; s[1] += u * v; s[2] += u;
        s[3] += v * v; s[4] += v;     s[5] += 1.0;
        s[6] += u * zz; s[7] += v * zz; s[8] += zz;
    }
    block_tree<9>(s, sh, partials + (size_t)blockIdx.x * 9);
}

__global__ __launch_bounds__(64) void k_sp_plane_final(const double* __restrict__ partials, int nblocks, double* __restrict__ sums)
{
    if (threadIdx.x >= 9) return;
    double a = 0.0;
    for (int g = 0; g < nblocks; g++) a += partials[(size_t)g * 9 + threadIdx.x];
    sums[threadIdx.x] = a;
}

// utils.py:394-396: float32 of the float64 product (x, y, 1) @ abc
__global__ __launch_bounds__(256) void k_sp_plane_eval(double a, double bb, double c, int w, float* __restrict__ out)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    out[(size_t)y * w + x] = (float)__fma_rn(1.0, c, __fma_rn((double)y, bb, __dmul_rn((double)x, a)));
}

// ---- e. triangulation of matches -------------------------------------------------------------------------------------
struct SpTri {
    double k1[9], k2[9], R[9], t[3];
};

// the per-match solve lives in triangulate.hpp: camd_epipolar_sums (epipolar.hip) evaluates the same function
__global__ __launch_bounds__(256) void k_sp_triangulate(const double* __restrict__ uv1, const double* __restrict__ uv2,
                                                        size_t n, SpTri m, double* __restrict__ zs1, double* __restrict__ zs2)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double u1 = uv1[i * 2], v1 = uv1[i * 2 + 1], u2 = uv2[i * 2], v2 = uv2[i * 2 + 1];
    double x1[3], b[3];
    tri_rays(m.k1, m.k2, u1, v1, u2, v2, x1, b);
    tri_solve(x1, b, m.R, m.t, zs1 + i, zs2 + i);
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_uvzs_to_arr2d(const double* uv, size_t n, int uv_stride, int w, int h, const void* values, int channels,
                       int value_type, double bg_value, int keep, void* out, uint32_t* owner_ws, void* stream)
{
    if (!out || !owner_ws || w <= 0 || h <= 0 || uv_stride < 2 || channels < 1 || (n && (!uv || !values))) {
        set_error("camd_uvzs_to_arr2d: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    if (!float_u8_type_ok(value_type)) {
        set_error("camd_uvzs_to_arr2d: value_type %d is none of float64 / float32 / uint8", value_type);
        return CAMD_ERR_BAD_ARG;
    }
    if (value_type == CAMD_VALUE_U8 && !keep && !(bg_value >= 0.0 && bg_value <= 255.0 && bg_value == (double)(uint8_t)bg_value)) {
        set_error("camd_uvzs_to_arr2d: bg_value %g is not a uint8", bg_value);
        return CAMD_ERR_BAD_ARG;
    }
    if ((unsigned long long)n >= 0xffffffffull) {
        set_error("camd_uvzs_to_arr2d: %zu rows do not fit the 32-bit owner index", n);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)w * h;
    fill(owner_ws, npix, 0u, nullptr, st);
    if (n) hipLaunchKernelGGL(k_sp_owner, dim3(div_up((long long)n, 256)), dim3(256), 0, st, uv, n, uv_stride, w, h, owner_ws);
    owner_gather(value_type, owner_ws, npix, values, channels, bg_value, keep, out, st);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_arr2d_to_uvzs(const void* arr2d, int w, int h, int as_int64, void* rows, void* stream)
{
    if (!arr2d || !rows || w <= 0 || h <= 0) { set_error("camd_arr2d_to_uvzs: bad arguments"); return CAMD_ERR_BAD_ARG; }
    CAMD_NEED_DEVICE();
    const dim3 grid(div_up((long long)w * h, 256));
    if (as_int64)
        hipLaunchKernelGGL((k_sp_all_rows<long long>), grid, dim3(256), 0, (hipStream_t)stream, (const long long*)arr2d, w, h,
                           (long long*)rows);
    else
        hipLaunchKernelGGL((k_sp_all_rows<double>), grid, dim3(256), 0, (hipStream_t)stream, (const double*)arr2d, w, h,
                           (double*)rows);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

size_t camd_arr2d_mask_workspace_bytes(int h) { return RowWorkspace::bytes(h); }

int camd_arr2d_to_uvzs_masked(const void* arr2d, const uint8_t* mask, int w, int h, int as_int64, void* rows,
                              size_t capacity, unsigned long long* count, void* workspace, void* stream)
{
    if (!arr2d || !mask || !rows || !count || !workspace || w <= 0 || h <= 0) {
        set_error("camd_arr2d_to_uvzs_masked: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const RowWorkspace ws(workspace, h);
    const MaskOn on = {mask, w};
    mask_row_count(on, h, ws.rowcount, st);
    row_scan(ws.rowcount, h, ws.rowoff, count, st);
    if (as_int64)
        row_emit(MaskRows<long long>{on, (const long long*)arr2d, (long long*)rows}, w, h, ws.rowoff, capacity, nullptr, st);
    else
        row_emit(MaskRows<double>{on, (const double*)arr2d, (double*)rows}, w, h, ws.rowoff, capacity, nullptr, st);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_sparse_bin_grid(int w, int h, double distance, int* radius, int* bins_w, int* bins_h)
{
    SpBins b;
    int rc = make_bins(&b, w, h, distance, "camd_sparse_bin_grid");
    if (rc != CAMD_OK) return rc;
    if (radius) *radius = b.R;
    if (bins_w) *bins_w = b.bw;
    if (bins_h) *bins_h = b.bh;
    return CAMD_OK;
}

int camd_sparse_bin_count(const double* uv, size_t n, int uv_stride, int w, int h, double distance, uint32_t* counts,
                          void* stream)
{
    SpBins b;
    int rc = make_bins(&b, w, h, distance, "camd_sparse_bin_count");
    if (rc != CAMD_OK) return rc;
    if (!counts || uv_stride < 2 || (n && !uv) || (unsigned long long)n >= 0xffffffffull) {
        set_error("camd_sparse_bin_count: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const size_t ncell = (size_t)b.bw * b.bh;
    fill(counts, ncell, 0u, nullptr, st);
    if (n) hipLaunchKernelGGL(k_sp_bin_count, dim3(div_up((long long)n, 256)), dim3(256), 0, st, uv, n, uv_stride, b, counts);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_sparse_bin_fill(const double* uv, size_t n, int uv_stride, int w, int h, double distance, uint32_t* cursor,
                         size_t capacity, double* sorted_uv, uint32_t* sorted_idx, void* stream)
{
    SpBins b;
    int rc = make_bins(&b, w, h, distance, "camd_sparse_bin_fill");
    if (rc != CAMD_OK) return rc;
    if (!cursor || uv_stride < 2 || (n && (!uv || !sorted_uv || !sorted_idx)) || (unsigned long long)n >= 0xffffffffull) {
        set_error("camd_sparse_bin_fill: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    if (n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_sp_bin_fill, dim3(div_up((long long)n, 256)), dim3(256), 0, (hipStream_t)stream, uv, n, uv_stride, b,
                       cursor, capacity, sorted_uv, sorted_idx);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_nearest_fill(const double* sorted_uv, const uint32_t* sorted_idx, const uint32_t* start, const void* z, int z_type,
                      int w, int h, double distance, float* out, int out_w, int out_h, void* stream)
{
    SpBins b;
    int rc = make_bins(&b, w, h, distance, "camd_nearest_fill");
    if (rc != CAMD_OK) return rc;
    if (!start || !out || out_w <= 0 || out_h <= 0 || out_h > 65535 || !float_type_ok(z_type)) {
        set_error("camd_nearest_fill: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    SpOut o;
    o.ow = out_w; o.oh = out_h;
    o.scaled = (out_w != w || out_h != h) ? 1 : 0;
    o.ifx = 1.0 / ((double)out_w / w);  // cv2.resize: inv_scale = dsize / ssize, ifx = 1 / inv_scale
    o.ify = 1.0 / ((double)out_h / h);
    o.mul = (float)out_w; o.div = (float)w;
    const dim3 grid(div_up(out_w, 256), out_h);
    with_float(z_type, [&](auto v) {
        using Z = decltype(v);
        hipLaunchKernelGGL((k_sp_nearest<Z>), grid, dim3(256), 0, (hipStream_t)stream, sorted_uv, sorted_idx, start,
                           (const Z*)z, b, distance, o, out);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_plane_sums_blocks(size_t n) { return sum_blocks(n); }

int camd_plane_sums(const double* uv, int uv_stride, const void* z, int z_type, size_t n, double* partials_ws, double* sums,
                    void* stream)
{
    if (!uv || !z || !partials_ws || !sums || n == 0 || uv_stride < 2 || !float_type_ok(z_type)) {
        set_error("camd_plane_sums: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const int g = sum_blocks(n);
    with_float(z_type, [&](auto v) {
        using Z = decltype(v);
        hipLaunchKernelGGL((k_sp_plane_partials<Z>), dim3(g), dim3(256), 0, st, uv, uv_stride, (const Z*)z, n, partials_ws);
    });
    hipLaunchKernelGGL(k_sp_plane_final, dim3(1), dim3(64), 0, st, partials_ws, g, sums);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_plane_eval(double a, double b, double c, int w, int h, float* out, void* stream)
{
    if (!out || w <= 0 || h <= 0 || h > 65535) { set_error("camd_plane_eval: bad arguments"); return CAMD_ERR_BAD_ARG; }
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_sp_plane_eval, dim3(div_up(w, 256), h), dim3(256), 0, (hipStream_t)stream, a, b, c, w, out);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_matched_uvs_to_zs(const double* uv1, const double* uv2, size_t n, const double K1inv[9], const double K2inv[9],
                           const double T_1to2[16], double* zs1, double* zs2, void* stream)
{
    if (!K1inv || !K2inv || !T_1to2 || (n && (!uv1 || !uv2 || !zs1 || !zs2))) {
        set_error("camd_matched_uvs_to_zs: NULL argument");
        return CAMD_ERR_BAD_ARG;
    }
    if (n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    SpTri m;
    for (int i = 0; i < 9; i++) { m.k1[i] = K1inv[i]; m.k2[i] = K2inv[i]; m.R[i] = T_1to2[(i / 3) * 4 + i % 3]; }
    for (int i = 0; i < 3; i++) m.t[i] = T_1to2[i * 4 + 3];
    hipLaunchKernelGGL(k_sp_triangulate, dim3(div_up((long long)n, 256)), dim3(256), 0, (hipStream_t)stream, uv1, uv2, n, m,
                       zs1, zs2);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
