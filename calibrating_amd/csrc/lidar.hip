// lidar.hip -- a LiDAR cloud as a dense depth image of a camera: the device side of xyzs_to_dense_depth in the reference's
// example/calibrate_lidar2cam_by_PnP/calibrate_lidar2cam_pnp.py:13-42.
//   a  camd_cloud_to_uvzs          cloud -> (T) -> K -> the rows inside the image, scaled, compacted in input order
//   b  camd_hull_row_range,        the convex hull of ANY number of samples: a point set and its per-row extremes have the
//      camd_hull_extremes          same hull, so an integer min / max table per pixel row stands for the cloud; its
//                                  non-empty rows go to camd_hull_fit (hull.hip) as candidates, in rounds (sparse.py)
//   c  camd_nearest_fill_in_hull   the search of camd_nearest_fill (nearest.hpp), only where the pixel is inside the hull
// Nothing depends on the order in which atomics are served: integer minima, maxima, sums and ors only.  The mask contract
// is hull.hip's own (UNPINNED against cv2.convexHull / drawContours).
#include "compact.hpp"
#include "hull_common.hpp"
#include "nearest.hpp"

namespace camd {

static inline bool doubles_at(const void* p) { return p && (uintptr_t)p % 8 == 0; }

// ---- a. cloud -> rows ------------------------------------------------------------------------------------------------
struct CloudArgs {
    const void* xyz;
    size_t n;
    int stride, chunk;  // elements between two points; points per compaction row (a multiple of 256)
    int has_T;
    double R[9], t[3], K[9];
    double w, h, rate;
};

struct CloudRow {
    double u, v, z;
    bool positive, keep;
};

// The arithmetic of one point, float64, every product and sum rounded on its own and in this order:
//   X' = ((R0 x + R1 y) + R2 z) + t       (rows of T; without T: X' = X)
//   p  = (K0 X' + K1 Y') + K2 Z'          (rows of K, all nine entries)
//   u = p0 / p2, v = p1 / p2;   kept iff p2 > 0, u >= 0, v >= 0, u < w, v < h  (NaN and inf fail a comparison)
// count and emit call this one function, so the pass that writes a row sees the bits the pass that counted it saw.
template <typename T>
__device__ __forceinline__ CloudRow cloud_row(const CloudArgs& a, size_t i)
{
    const T* p = (const T*)a.xyz + i * (size_t)a.stride;
    double X = (double)p[0], Y = (double)p[1], Z = (double)p[2];
    if (a.has_T) {
        const double x = X, y = Y, z = Z;
        X = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.R[0], x), __dmul_rn(a.R[1], y)), __dmul_rn(a.R[2], z)), a.t[0]);
        Y = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.R[3], x), __dmul_rn(a.R[4], y)), __dmul_rn(a.R[5], z)), a.t[1]);
        Z = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.R[6], x), __dmul_rn(a.R[7], y)), __dmul_rn(a.R[8], z)), a.t[2]);
    }
    const double p0 = __dadd_rn(__dadd_rn(__dmul_rn(a.K[0], X), __dmul_rn(a.K[1], Y)), __dmul_rn(a.K[2], Z));
    const double p1 = __dadd_rn(__dadd_rn(__dmul_rn(a.K[3], X), __dmul_rn(a.K[4], Y)), __dmul_rn(a.K[5], Z));
    const double p2 = __dadd_rn(__dadd_rn(__dmul_rn(a.K[6], X), __dmul_rn(a.K[7], Y)), __dmul_rn(a.K[8], Z));
    CloudRow r;
    r.u = __ddiv_rn(p0, p2), r.v = __ddiv_rn(p1, p2), r.z = Z;
    r.positive = p2 > 0.0;
    r.keep = r.positive && r.u >= 0.0 && r.v >= 0.0 && r.u < a.w && r.v < a.h;
    return r;
}

// The compaction of compact.hpp over the cloud cut into rows of `chunk` points: element x of row y is point y * chunk + x.
// One lane per point; rowcount[y] = the kept points of row y; *n_positive += the points with p2 > 0 (an integer sum).
template <typename T>
__global__ __launch_bounds__(256) void k_cloud_count(CloudArgs a, uint32_t* __restrict__ rowcount,
                                                     unsigned long long* __restrict__ n_positive)
{
    __shared__ uint32_t part[4];
    const int y = blockIdx.x;
    uint32_t kept = 0, positive = 0;
    for (int x = threadIdx.x; x < a.chunk; x += 256) {
        const size_t i = (size_t)y * a.chunk + x;
        if (i < a.n) {
            const CloudRow r = cloud_row<T>(a, i);
            kept += r.keep ? 1u : 0u, positive += r.positive ? 1u : 0u;
        }
    }
    kept = block_total(wave_sum(kept), part);
    __syncthreads();  // (part is written again)
    positive = block_total(wave_sum(positive), part);
    if (threadIdx.x == 0) {
        rowcount[y] = kept;
        if (positive) atomicAdd(n_positive, (unsigned long long)positive);
    }
}

template <typename T>
struct CloudRows {
    CloudArgs a;
    double* rows;
    __device__ __forceinline__ bool on(int x, int y) const
    {
        const size_t i = (size_t)y * a.chunk + x;
        return i < a.n && cloud_row<T>(a, i).keep;
    }
    __device__ __forceinline__ void emit(int x, int y, unsigned long long pos) const
    {
        const CloudRow r = cloud_row<T>(a, (size_t)y * a.chunk + x);
        rows[pos * 3 + 0] = __dmul_rn(r.u, a.rate);
        rows[pos * 3 + 1] = __dmul_rn(r.v, a.rate);
        rows[pos * 3 + 2] = r.z;
    }
};

// points per compaction row: 256 while that leaves at most 2048 rows (one workgroup scans them), else the multiple of 256
// that does
static inline int cloud_chunk(size_t n)
{
    const size_t g = (n + (size_t)256 * 2048 - 1) / ((size_t)256 * 2048);
    return 256 * (int)(g < 1 ? 1 : g);
}
static inline int cloud_rows(size_t n) { return (int)((n + (size_t)cloud_chunk(n) - 1) / (size_t)cloud_chunk(n)); }

// ---- b. the hull of any number of samples -----------------------------------------------------------------------------
// the rounded pixel of a sample by k_hull_fit's rule (hull.hip): finite u, v; rint, half to even; within 2^20, else the
// status bit and no pixel
__device__ __forceinline__ bool hull_pixel(const double* __restrict__ uv, size_t i, int stride, int* x, int* y, int* status)
{
    const double u = uv[i * (size_t)stride], v = uv[i * (size_t)stride + 1];
    if (!(isfinite(u) && isfinite(v))) return false;
    const double ru = rint(u), rv = rint(v);
    if (!(fabs(ru) <= HULL_MAX_COORD && fabs(rv) <= HULL_MAX_COORD)) {
        *status |= HULL_OUT_OF_RANGE;
        return false;
    }
    *x = (int)ru, *y = (int)rv;
    return true;
}

__global__ void k_hull_range_init(int* __restrict__ range)
{
    if (threadIdx.x == 0) range[0] = INT_MAX, range[1] = INT_MIN, range[2] = 0;
}

// range[0] = the lowest, range[1] = the highest rounded v of the samples that have a pixel, range[2] |= their status bits.
// Every lane stays for the butterfly; lane 0 of a wave sends its wave's three numbers.
__global__ __launch_bounds__(256) void k_hull_row_range(const double* __restrict__ uv, size_t n, int stride, int* __restrict__ range)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int lo = INT_MAX, hi = INT_MIN, status = 0, x, y;
    if (i < n && hull_pixel(uv, i, stride, &x, &y, &status)) lo = hi = y;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        lo = min(lo, __shfl_xor(lo, m, 64));
        hi = max(hi, __shfl_xor(hi, m, 64));
        status |= __shfl_xor(status, m, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (lo <= hi) atomicMin(range + 0, lo), atomicMax(range + 1, hi);
        if (status) atomicOr(range + 2, status);
    }
}

// table: rows x 2 int32, (xmin, xmax) of pixel row y0 + r; empty: (INT_MAX, INT_MIN)
__global__ __launch_bounds__(256) void k_hull_table_clear(int* __restrict__ table, int rows, int* __restrict__ status)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < rows) table[(size_t)r * 2] = INT_MAX, table[(size_t)r * 2 + 1] = INT_MIN;
    if (r == 0) *status = 0;
}

// One lane per sample.  Minimum and maximum do not depend on the order they are taken in: the same table on every run.
// The plain read in front only spares an atomic that could not change the entry (entries only ever move outwards).
// A sample whose row is not one of the table's takes no part.
__global__ __launch_bounds__(256) void k_hull_extremes(const double* __restrict__ uv, size_t n, int stride, int y0, int rows,
                                                       int* table, int* __restrict__ status)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int x, y, st = 0;
    const bool ok = hull_pixel(uv, i, stride, &x, &y, &st);
    if (st) atomicOr(status, st);
    if (!ok) return;
    const long long r = (long long)y - y0;
    if (r < 0 || r >= rows) return;
    int* e = table + (size_t)r * 2;
    if (x < e[0]) atomicMin(e, x);
    if (x > e[1]) atomicMax(e + 1, x);
}

// The non-empty rows' (xmin, y), (xmax, y) as float64 candidate rows, in rising y, min before max; *count = their number.
// One workgroup walks the table 256 rows at a time (block_slot, compact.hpp).
__global__ __launch_bounds__(256) void k_hull_candidates(const int* __restrict__ table, int y0, int rows,
                                                         double* __restrict__ candidates, unsigned long long* __restrict__ count)
{
    __shared__ uint32_t wcnt[4];
    __shared__ unsigned long long run;
    if (threadIdx.x == 0) run = 0;
    __syncthreads();
    for (int base = 0; base < rows; base += 256) {
        const int r = base + threadIdx.x;
        int lo = INT_MAX, hi = INT_MIN;
        if (r < rows) lo = table[(size_t)r * 2], hi = table[(size_t)r * 2 + 1];
        const bool on = lo <= hi;
        const unsigned long long pos = block_slot(on, run, wcnt);
        if (on) {
            double* c = candidates + pos * 4;
            c[0] = (double)lo, c[1] = (double)(y0 + r), c[2] = (double)hi, c[3] = (double)(y0 + r);
        }
        __syncthreads();
        if (threadIdx.x == 0) run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = 2 * run;
}

// ---- c. the nearest sample, inside the hull only ------------------------------------------------------------------------
// A workgroup is 256 consecutive x of ONE row, so each of its waves owns one y and works its span out once, all 64 lanes
// together -- the lanes beyond the image too: they leave only after the butterfly.  A pixel outside the closed span
// [xl, xr] is 0 without a search; inside, the search of k_sp_nearest (nearest.hpp).
template <typename Z>
__global__ __launch_bounds__(256) void k_nearest_in_hull(const double* __restrict__ sorted_uv, const uint32_t* __restrict__ sorted_idx,
                                                         const uint32_t* __restrict__ start, const Z* __restrict__ z, size_t z_stride,
                                                         SpBins b, double distance, const int* __restrict__ vertices,
                                                         const int* __restrict__ hull_counts, int capacity, float* __restrict__ out)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, lane = threadIdx.x & 63;
    int count = hull_counts[0];
    count = count < 0 ? 0 : (count > capacity ? capacity : count);
    int xl, xr;
    hull_span(vertices, count, y, b.w, lane, &xl, &xr);
    if (x >= b.w) return;
    float v = 0.0f;
    if (x >= xl && x <= xr) v = sp_nearest_value(sorted_uv, sorted_idx, start, z, z_stride, b, distance, x, y);
    out[(size_t)y * b.w + x] = v;
}

}  // namespace camd

using namespace camd;

extern "C" {

size_t camd_cloud_workspace_bytes(size_t n) { return RowWorkspace::bytes(n ? cloud_rows(n) : 1); }

int camd_cloud_to_uvzs(const void* xyz, int xyz_type, size_t n, int xyz_stride, const double* T, const double K[9], int w, int h,
                       double rate, int stages, double* rows, size_t capacity, unsigned long long* counters, void* workspace,
                       void* stream)
{
    const bool count = (stages & 1) != 0, emit = (stages & 2) != 0;
    if (!K || !counters || (uintptr_t)counters % 8 != 0 || !workspace || (uintptr_t)workspace % 8 != 0 || w <= 0 || h <= 0 ||
        xyz_stride < 3 || !float_type_ok(xyz_type) || (n && !xyz) || n >= ((size_t)1 << 31) || !(count || emit) || (stages & ~3) ||
        (emit && (!(rate > 0.0) || !(rate < INFINITY) || (capacity && ((uintptr_t)rows % 8 != 0 || !rows))))) {
        set_error("camd_cloud_to_uvzs: bad arguments (xyz_type CAMD_VALUE_F64 or _F32; xyz_stride >= 3; fewer than 2^31 points; "
                  "w, h >= 1; stages 1, 2 or 3; to emit, a finite rate > 0)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    CloudArgs a = {};
    a.xyz = xyz, a.n = n, a.stride = xyz_stride, a.chunk = cloud_chunk(n), a.has_T = T ? 1 : 0;
    for (int i = 0; i < 9; i++) a.K[i] = K[i], a.R[i] = T ? T[(i / 3) * 4 + i % 3] : (i % 4 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 3; i++) a.t[i] = T ? T[i * 4 + 3] : 0.0;
    a.w = (double)w, a.h = (double)h, a.rate = rate;
    const int nrows = n ? cloud_rows(n) : 0;
    const RowWorkspace ws(workspace, nrows ? nrows : 1);
    if (count) {
        fill(ws.rowcount, (size_t)0, 0u, counters + 1, st);  // (nothing to fill: the launch that zeroes the second counter)
        if (nrows)
            with_float(xyz_type, [&](auto v) {
                using V = decltype(v);
                hipLaunchKernelGGL((k_cloud_count<V>), dim3(nrows), dim3(256), 0, st, a, ws.rowcount, counters + 1);
            });
        row_scan(ws.rowcount, nrows, ws.rowoff, counters, st);
    }
    if (emit && nrows)
        with_float(xyz_type, [&](auto v) {
            using V = decltype(v);
            row_emit(CloudRows<V>{a, rows}, a.chunk, nrows, ws.rowoff, capacity, nullptr, st);
        });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_hull_row_range(const double* uv, int uv_stride, size_t n, int* range, void* stream)
{
    if (!range || (uintptr_t)range % 4 != 0 || uv_stride < 2 || (n && !doubles_at(uv)) || n >= ((size_t)1 << 31)) {
        set_error("camd_hull_row_range: bad arguments (uv: aligned doubles, uv_stride >= 2, fewer than 2^31 rows; range: 3 int32)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_hull_range_init, dim3(1), dim3(64), 0, st, range);
    if (n) hipLaunchKernelGGL(k_hull_row_range, dim3(div_up((long long)n, 256)), dim3(256), 0, st, uv, n, uv_stride, range);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_hull_extremes(const double* uv, int uv_stride, size_t n, int y0, int rows, int* table, double* candidates,
                       unsigned long long* count, int* status, void* stream)
{
    if (!table || (uintptr_t)table % 4 != 0 || !doubles_at(candidates) || !count || (uintptr_t)count % 8 != 0 || !status ||
        (uintptr_t)status % 4 != 0 || uv_stride < 2 || (n && !doubles_at(uv)) || n >= ((size_t)1 << 31) || rows < 1 ||
        rows > (1 << 21) + 1 || y0 < -(1 << 20) || y0 > (1 << 20)) {
        set_error("camd_hull_extremes: bad arguments (uv: aligned doubles, uv_stride >= 2, fewer than 2^31 rows; 1 <= rows <= 2^21 + 1; "
                  "|y0| <= 2^20; table: rows x 2 int32; candidates: 2 rows x 2 float64)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_hull_table_clear, dim3(div_up(rows, 256)), dim3(256), 0, st, table, rows, status);
    if (n) hipLaunchKernelGGL(k_hull_extremes, dim3(div_up((long long)n, 256)), dim3(256), 0, st, uv, n, uv_stride, y0, rows, table, status);
    hipLaunchKernelGGL(k_hull_candidates, dim3(1), dim3(256), 0, st, table, y0, rows, candidates, count);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_nearest_fill_in_hull(const double* sorted_uv, const uint32_t* sorted_idx, const uint32_t* start, const void* z, int z_type,
                              size_t z_stride, int w, int h, double distance, const int* vertices, const int* hull_counts,
                              int vertex_capacity, float* out, void* stream)
{
    SpBins b;
    int rc = make_bins(&b, w, h, distance, "camd_nearest_fill_in_hull");
    if (rc != CAMD_OK) return rc;
    if (!start || !out || (uintptr_t)out % 4 != 0 || !float_type_ok(z_type) || z_stride < 1 || !vertices || !hull_counts ||
        (uintptr_t)vertices % 4 != 0 || (uintptr_t)hull_counts % 4 != 0 || vertex_capacity < 1 || vertex_capacity > HULL_MAX_POINTS) {
        set_error("camd_nearest_fill_in_hull: bad arguments (z_type CAMD_VALUE_F64 or _F32; z_stride >= 1; vertex_capacity 1 .. %d; "
                  "start, vertices, hull_counts, out: device arrays)", HULL_MAX_POINTS);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const dim3 grid(div_up(w, 256), h);
    with_float(z_type, [&](auto v) {
        using Z = decltype(v);
        hipLaunchKernelGGL((k_nearest_in_hull<Z>), grid, dim3(256), 0, (hipStream_t)stream, sorted_uv, sorted_idx, start,
                           (const Z*)z, z_stride, b, distance, vertices, hull_counts, vertex_capacity, out);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
