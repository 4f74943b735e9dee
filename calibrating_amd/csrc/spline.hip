// spline.hip -- the thin-plate spline through sparse (u, v, z) samples, evaluated at every pixel: the device side of the
// reference's interpolate_uvzs(inter_type="rbf"), i.e. scipy.interpolate.Rbf(u, v, z, function="thin_plate", smooth=s)
// (utils.py:373-388), batched over frames.  float64 throughout; every product and sum is rounded on its own
// (-ffp-contract=off) in the order the source gives, so tests/spline_ref.py restates each stage operation for operation
// and differs from it only where the device's log differs from np.log.  Three stages, each an entry of the C ABI:
//   camd_spline_assemble   A = Phi - smooth I of every frame, one lane per (i, j) with j <= i, mirrored
//   camd_spline_solve      A w = z by LU with partial pivoting, ONE workgroup per frame, the matrix in global memory
//   camd_spline_eval       sum_i w_i phi(|p - (u_i, v_i)|) at every pixel, samples staged through LDS in tiles of 256
// and camd_spline_upsize, the cv2.resize(INTER_NEAREST) of a coarse surface (FeatureMatchingAsStereoMatching's last step).
// A frame's rows are start[f] .. start[f + 1] of one ragged array; a frame's numbers depend on its own rows only, so it
// gets the same bits alone and anywhere in a batch.  No atomics, no grid-wide barrier, no cooperative launch.
#include "common.hpp"
#include "pnp_common.hpp"

#include <climits>
#include <cmath>

namespace camd {

constexpr int SPLINE_MAX_POINTS = CAMD_SPLINE_MAX_POINTS;
constexpr int SPLINE_TILE = 256;            // samples staged per round of the evaluation: u, v, w = 6 KB of LDS
constexpr int SPLINE_SOLVE_THREADS = 1024;  // the one workgroup of a frame's factorisation: 16 waves, a wave per row
static_assert(SPLINE_MAX_POINTS <= SPLINE_SOLVE_THREADS, "the right-hand side lives in LDS, one slot per thread at most");

// phi(r) = r^2 log r of r = sqrt(dx^2 + dy^2), phi(0) = 0: SciPy's xlogy(r**2, r)
__device__ __forceinline__ double spline_phi(double dx, double dy)
{
    const double r = sqrt(dx * dx + dy * dy);
    return r == 0.0 ? 0.0 : (r * r) * log(r);
}

// the rows of frame f: *first and the returned number.  A range that leaves the rows or is longer than the capacity is
// read nowhere and counts as a frame without rows (camd_hull_fit's rule)
__device__ __forceinline__ int spline_frame(const long long* __restrict__ start, int f, size_t rows, int capacity, long long* first)
{
    const long long a = start[f], b = start[f + 1];
    *first = a;
    if (a < 0 || b < a || (unsigned long long)b > rows || b - a > capacity) return 0;
    return (int)(b - a);
}

// ---- 1. assembly -----------------------------------------------------------------------------------------------------
// 16 x 16 lanes per tile of (i, j); tiles above the diagonal leave at once, lanes with j > i do nothing: each entry is
// computed once and stored twice, so the matrix is symmetric bit for bit.
__global__ __launch_bounds__(256) void k_spline_assemble(const double* __restrict__ uvz, int stride, size_t rows,
                                                         const long long* __restrict__ start, int capacity, double smooth,
                                                         double* __restrict__ A)
{
    if (blockIdx.x > blockIdx.y) return;
    const int f = blockIdx.z;
    long long first;
    const int n = spline_frame(start, f, rows, capacity, &first);
    const int i = blockIdx.y * 16 + threadIdx.y, j = blockIdx.x * 16 + threadIdx.x;
    if (i >= n || j > i) return;
    double* M = A + (size_t)f * capacity * capacity;
    if (i == j) {
        M[(size_t)i * capacity + i] = 0.0 - smooth;
        return;
    }
    const double* pi = uvz + (size_t)(first + i) * stride;
    const double* pj = uvz + (size_t)(first + j) * stride;
    const double v = spline_phi(pi[0] - pj[0], pi[1] - pj[1]);
    M[(size_t)i * capacity + j] = v;
    M[(size_t)j * capacity + i] = v;
}

// ---- 2. solve --------------------------------------------------------------------------------------------------------
// Step k: the pivot is the row i >= k with the largest |a[i][k]|, of equal ones the lowest (a non-finite entry counts as
// +inf and ends the frame); rows k and p are exchanged from column k on; then for every i > k, a wave per row:
//   m = a[i][k] / a[k][k],   a[i][j] = a[i][j] - m * a[k][j]  (j > k),   b[i] = b[i] - m * b[k]
// (column k below the diagonal is left as it was: nothing reads it again).  Every element is updated by one thread from
// values no thread writes in that step, so the bits do not depend on who does what.  The pivot search is a thread's
// strided scan, then a binary tree over the 1024 threads (the shape of compact.hpp's block_tree; (key, row) under a total
// order, so the winner is unique).  Back-substitution by columns, k = n - 1 ... 0:
//   x[k] = b[k] / a[k][k],   b[i] = b[i] - a[i][k] * x[k]  (i < k)
// -- each b[i] takes its subtractions in falling k.  The right-hand side lives in LDS.
__global__ __launch_bounds__(SPLINE_SOLVE_THREADS) void k_spline_solve(const double* __restrict__ z, int z_stride, size_t rows,
                                                                       const long long* __restrict__ start, int capacity,
                                                                       double* __restrict__ A, double* __restrict__ weights,
                                                                       int* __restrict__ status)
{
    constexpr int T = SPLINE_SOLVE_THREADS;
    __shared__ double rhs[SPLINE_MAX_POINTS];
    __shared__ double key[T];
    __shared__ int arg[T];
    __shared__ int flag;
    const int f = blockIdx.x, t = threadIdx.x;
    long long first;
    const int n = spline_frame(start, f, rows, capacity, &first);
    double* M = A + (size_t)f * capacity * capacity;
    double* w = weights + (size_t)f * capacity;
    if (n == 0) {  // (the whole workgroup)
        if (t == 0) status[f] = CAMD_SPLINE_NO_SAMPLE;
        return;
    }
    if (t == 0) flag = 0;
    __syncthreads();
    bool bad = false;
    for (int i = t; i < n; i += T) {
        const double v = z[(size_t)(first + i) * z_stride];
        rhs[i] = v;
        bad |= !isfinite(v);
    }
    for (int i = 0; i < n; i++)
        for (int j = t; j < n; j += T) bad |= !isfinite(M[(size_t)i * capacity + j]);
    if (bad) flag = 1;  // (every writer stores the same word)
    __syncthreads();
    int failed = flag ? CAMD_SPLINE_NON_FINITE : 0;

    for (int k = 0; k < n && !failed; k++) {
        double best = -1.0;
        int bi = INT_MAX;
        for (int i = k + t; i < n; i += T) {
            double a = fabs(M[(size_t)i * capacity + k]);
            if (!isfinite(a)) a = INFINITY;
            if (a > best) best = a, bi = i;
        }
        key[t] = best, arg[t] = bi;
        __syncthreads();
        for (int o = T / 2; o > 0; o >>= 1) {
            if (t < o && (key[t + o] > key[t] || (key[t + o] == key[t] && arg[t + o] < arg[t]))) key[t] = key[t + o], arg[t] = arg[t + o];
            __syncthreads();
        }
        const int p = arg[0];
        const double pk = key[0];
        __syncthreads();  // (key, arg are free again)
        if (!(pk > 0.0) || pk == INFINITY) {
            failed = CAMD_SPLINE_SINGULAR;
            break;
        }
        if (p != k) {
            for (int j = k + t; j < n; j += T) {
                const double a = M[(size_t)k * capacity + j], b = M[(size_t)p * capacity + j];
                M[(size_t)k * capacity + j] = b, M[(size_t)p * capacity + j] = a;
            }
            if (t == 0) {
                const double a = rhs[k];
                rhs[k] = rhs[p], rhs[p] = a;
            }
        }
        __syncthreads();
        const double* rowk = M + (size_t)k * capacity;
        const double piv = rowk[k], bk = rhs[k];
        const int lane = t & 63;
        for (int i = k + 1 + (t >> 6); i < n; i += T / 64) {
            double* rowi = M + (size_t)i * capacity;
            const double m = rowi[k] / piv;
            for (int j = k + 1 + lane; j < n; j += 64) rowi[j] = rowi[j] - m * rowk[j];
            if (lane == 0) rhs[i] = rhs[i] - m * bk;
        }
        __syncthreads();
    }
    if (failed) {
        for (int i = t; i < n; i += T) w[i] = NAN;
        if (t == 0) status[f] = failed;
        return;
    }
    for (int k = n - 1; k >= 0; k--) {
        if (t == 0) rhs[k] = rhs[k] / M[(size_t)k * capacity + k];
        __syncthreads();
        const double x = rhs[k];
        for (int i = t; i < k; i += T) rhs[i] = rhs[i] - M[(size_t)i * capacity + k] * x;
        __syncthreads();
    }
    for (int i = t; i < n; i += T) w[i] = rhs[i];
    if (t == 0) status[f] = 0;
}

// ---- 3. evaluation ---------------------------------------------------------------------------------------------------
// One lane per pixel of the (oh, ow) image, which stands at (x * step, y * step) of the samples' frame.  The samples go
// through LDS SPLINE_TILE at a time; a lane adds  s = s + w_i * phi_i  in rising i, so a pixel's bits depend on neither the
// launch geometry nor the frame's place in the batch.  A workgroup none of whose pixels is inside the mask stages nothing.
__global__ __launch_bounds__(256) void k_spline_eval(const double* __restrict__ uvz, int stride, size_t rows,
                                                     const long long* __restrict__ start, int capacity,
                                                     const double* __restrict__ weights, const uint8_t* __restrict__ mask, int ow,
                                                     int oh, int step, double* __restrict__ out)
{
    __shared__ double su[SPLINE_TILE], sv[SPLINE_TILE], sw[SPLINE_TILE];
    const int f = blockIdx.y;
    const size_t npix = (size_t)ow * oh, pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool inside = pix < npix;
    const bool on = inside && (!mask || mask[(size_t)f * npix + pix] != 0);
    if (!__syncthreads_or(on ? 1 : 0)) {
        if (inside) out[(size_t)f * npix + pix] = 0.0;
        return;
    }
    long long first;
    const int n = spline_frame(start, f, rows, capacity, &first);
    const double x = (double)((int)(pix % (size_t)ow) * step), y = (double)((int)(pix / (size_t)ow) * step);
    double s = 0.0;
    for (int base = 0; base < n; base += SPLINE_TILE) {
        const int i = base + (int)threadIdx.x;
        if (i < n) {
            const double* p = uvz + (size_t)(first + i) * stride;
            su[threadIdx.x] = p[0], sv[threadIdx.x] = p[1], sw[threadIdx.x] = weights[(size_t)f * capacity + i];
        }
        __syncthreads();
        if (on) {
            const int m = n - base < SPLINE_TILE ? n - base : SPLINE_TILE;
            for (int q = 0; q < m; q++) s = s + sw[q] * spline_phi(x - su[q], y - sv[q]);
        }
        __syncthreads();
    }
    if (inside) out[(size_t)f * npix + pix] = on ? s : 0.0;
}

// cv2.resize(INTER_NEAREST) of (src * mul) / div: sx = min(floor(X * ifx), w - 1), as k_sp_nearest in sparse.hip
__global__ __launch_bounds__(256) void k_spline_upsize(const double* __restrict__ src, int w, int h, double ifx, double ify,
                                                       double mul, double div, int ow, int oh, double* __restrict__ out)
{
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y, f = blockIdx.z;
    if (X >= ow) return;
    const int x = min((int)floor(X * ifx), w - 1), y = min((int)floor(Y * ify), h - 1);
    out[((size_t)f * oh + Y) * ow + X] = (src[((size_t)f * h + y) * w + x] * mul) / div;
}

static int spline_rows_ok(const double* rows_ptr, int stride, size_t rows, const long long* start, int frames, int capacity,
                          const char* who)
{
    if (frames < 1 || frames > 65535 || stride < 1 || capacity < 1 || capacity > SPLINE_MAX_POINTS || !start ||
        (uintptr_t)start % 8 != 0 || (rows && !doubles_ok(rows_ptr)) || rows >= ((size_t)1 << 40)) {
        set_error("%s: bad arguments (frames 1 .. 65535; capacity 1 .. %d; start: frames + 1 int64 on the device; the rows: "
                  "aligned doubles)", who, SPLINE_MAX_POINTS);
        return CAMD_ERR_BAD_ARG;
    }
    return CAMD_OK;
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_spline_assemble(const double* uvz, int uvz_stride, size_t rows, const long long* start, int frames, int capacity,
                         double smooth, double* A, void* queue)
{
    int rc = spline_rows_ok(uvz, uvz_stride, rows, start, frames, capacity, "camd_spline_assemble");
    if (rc != CAMD_OK) return rc;
    if (uvz_stride < 2 || !doubles_ok(A) || smooth != smooth) {
        set_error("camd_spline_assemble: bad arguments (uvz_stride >= 2; A: aligned device doubles; smooth is a number)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const int tiles = div_up(capacity, 16);
    hipLaunchKernelGGL(k_spline_assemble, dim3(tiles, tiles, frames), dim3(16, 16), 0, (hipStream_t)queue, uvz, uvz_stride, rows,
                       start, capacity, smooth, A);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_spline_solve(const double* z, int z_stride, size_t rows, const long long* start, int frames, int capacity, double* A,
                      double* weights, int* status, void* queue)
{
    int rc = spline_rows_ok(z, z_stride, rows, start, frames, capacity, "camd_spline_solve");
    if (rc != CAMD_OK) return rc;
    if (!doubles_ok(A) || !doubles_ok(weights) || !status || (uintptr_t)status % 4 != 0) {
        set_error("camd_spline_solve: bad arguments (A, weights: aligned device doubles; status: device int32)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_spline_solve, dim3(frames), dim3(SPLINE_SOLVE_THREADS), 0, (hipStream_t)queue, z, z_stride, rows, start,
                       capacity, A, weights, status);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_spline_eval(const double* uvz, int uvz_stride, size_t rows, const long long* start, int frames, int capacity,
                     const double* weights, const uint8_t* mask, int out_w, int out_h, int grid_step, double* out, void* queue)
{
    int rc = spline_rows_ok(uvz, uvz_stride, rows, start, frames, capacity, "camd_spline_eval");
    if (rc != CAMD_OK) return rc;
    if (uvz_stride < 2 || !doubles_ok(weights) || !doubles_ok(out) || out_w <= 0 || out_h <= 0 || grid_step < 1 ||
        (long long)out_w * grid_step > INT_MAX || (long long)out_h * grid_step > INT_MAX ||
        ((long long)out_w * out_h + 255) / 256 > INT_MAX) {
        set_error("camd_spline_eval: bad arguments (uvz_stride >= 2; weights, out: aligned device doubles; out_w, out_h, grid_step "
                  ">= 1 with out_w * grid_step, out_h * grid_step < 2^31)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const unsigned groups = (unsigned)(((long long)out_w * out_h + 255) / 256);
    hipLaunchKernelGGL(k_spline_eval, dim3(groups, frames), dim3(256), 0, (hipStream_t)queue, uvz, uvz_stride, rows, start,
                       capacity, weights, mask, out_w, out_h, grid_step, out);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_spline_upsize(const double* src, int w, int h, int frames, double* out, int out_w, int out_h, void* queue)
{
    if (!doubles_ok(src) || !doubles_ok(out) || src == out || w <= 0 || h <= 0 || out_w <= 0 || out_h <= 0 || out_h > 65535 ||
        frames < 1 || frames > 65535) {
        set_error("camd_spline_upsize: bad arguments (src, out: distinct aligned device doubles; sizes >= 1; out_h, frames <= 65535)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const double ifx = 1.0 / ((double)out_w / w), ify = 1.0 / ((double)out_h / h);  // cv2.resize: ifx = 1 / (dsize / ssize)
    hipLaunchKernelGGL(k_spline_upsize, dim3(div_up(out_w, 256), out_h, frames), dim3(256), 0, (hipStream_t)queue, src, w, h, ifx,
                       ify, (double)out_w, (double)w, out_w, out_h, out);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
