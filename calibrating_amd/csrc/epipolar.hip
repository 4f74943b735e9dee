// epipolar.hip -- the device side of calibrating_amd/epipolar_geometry.py: what the reference's epipolar_geometry.py,
// flow_utils.py and ReconstructionExtrinsics.build_set2ds_by_flowds do per point or per pixel in NumPy
//   matching_uvs_in_one_img   np.unique(cells, axis=0, return_index=True) x2 + np.intersect1d -> first-index grids + intersection
//   filter_overlap_uvs        np.unique(..., return_counts, return_inverse) x2 + uvs[mask]    -> population grids + compaction
//   EssentialMatrixStereo     the mean depth of every match under each of the four candidate poses -> one fused pass
//   align_scale_with          zs[idx].mean()                                                  -> gathered fixed-order sum
//   build_set2ds_by_flowds    xys_abs[mask], (flow_abs + xys_abs)[mask]                       -> masked compaction
//   flow_abs_to_normal / flow_normal_to_abs
// Integer atomics only (min / add commute, so the grids do not depend on the order they are served in); every float sum
// is reduced in a fixed order.  Compactions and block sums are the pieces of compact.hpp; where the C header says so the
// scan is the caller's.  Products and sums are individually rounded (-ffp-contract=off).
#include "common.hpp"
#include "compact.hpp"
#include "triangulate.hpp"

#include <cmath>

namespace camd {

constexpr uint32_t EP_EMPTY = 0xffffffffu;
constexpr unsigned long long EP_MAX_CELLS = 1ull << 28;

struct EpWin {
    int cu0, cv0, cw, ch;  // cells cu0 .. cu0 + cw - 1, cv0 .. cv0 + ch - 1; stored u-major: [(cu - cu0) * ch + (cv - cv0)]
};

__device__ __forceinline__ double ep_div(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float ep_div(float a, float b) { return __fdiv_rn(a, b); }

// np.int32((uv / d).round()): the division in the rows' own type, round half to even.  rintf(x) == rint((double)x).
template <typename T>
__device__ __forceinline__ bool ep_cell(const T* __restrict__ uv, size_t i, int stride, T d, const EpWin& w, size_t* cell)
{
    const double ru = rint((double)ep_div(uv[i * stride], d)), rv = rint((double)ep_div(uv[i * stride + 1], d));
    if (!(ru >= (double)w.cu0 && ru < (double)w.cu0 + (double)w.cw && rv >= (double)w.cv0 && rv < (double)w.cv0 + (double)w.ch))
        return false;  // (also NaN / inf)
    *cell = (size_t)((long long)ru - w.cu0) * (size_t)w.ch + (size_t)((long long)rv - w.cv0);
    return true;
}

// FIRST: grid[cell] = min(row index) -- np.unique(return_index=True) reports the first occurrence, the smallest index.
// !FIRST: grid[cell] += 1 -- np.unique(return_counts=True)[inverse].
template <typename T, bool FIRST>
__global__ __launch_bounds__(256) void k_ep_cells(const T* __restrict__ uv, size_t n, int stride, T d, EpWin w,
                                                  uint32_t* __restrict__ grid, unsigned long long* __restrict__ outside)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    size_t cell;
    if (!ep_cell(uv, i, stride, d, w, &cell)) { atomicAdd(outside, 1ull); return; }
    if (FIRST) atomicMin(grid + cell, (uint32_t)i);
    else atomicAdd(grid + cell, 1u);
}

// ---- the intersection --------------------------------------------------------------------------------------------------
// np.unique(axis=0) sorts the (u, v) cell rows lexicographically as signed integers and np.intersect1d keeps that order:
// ascending u cell, then v cell -- the linear order of the u-major grid.  A compaction (compact.hpp) whose rows are the u
// columns.
struct EpIsect {
    const uint32_t *f1, *f2;
    int ch;
    long long *idx1, *idx2;
    __device__ __forceinline__ bool on(int v, int cu) const
    {
        const size_t c = (size_t)cu * ch + v;
        return f1[c] != EP_EMPTY && f2[c] != EP_EMPTY;
    }
    __device__ __forceinline__ void emit(int v, int cu, unsigned long long pos) const
    {
        const size_t c = (size_t)cu * ch + v;
        idx1[pos] = (long long)f1[c];
        idx2[pos] = (long long)f2[c];
    }
};

// ---- the overlap filter ------------------------------------------------------------------------------------------------
// keep[i] = both pixels of match i are hit once; blockcount[b] = how many of rows 256 b .. 256 b + 255 are kept
template <typename T>
__global__ __launch_bounds__(256) void k_ep_overlap_keep(const T* __restrict__ uv1, const T* __restrict__ uv2, size_t n, int stride,
                                                         EpWin w, const uint32_t* __restrict__ cnt1,
                                                         const uint32_t* __restrict__ cnt2, uint8_t* __restrict__ keep,
                                                         uint32_t* __restrict__ blockcount)
{
    __shared__ uint32_t part[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    if (i < n) {
        size_t c1, c2;
        on = ep_cell(uv1, i, stride, (T)1, w, &c1) && ep_cell(uv2, i, stride, (T)1, w, &c2) && cnt1[c1] <= 1u && cnt2[c2] <= 1u;
        keep[i] = on ? 1 : 0;
    }
    const uint32_t c = block_count(on, part);
    if (threadIdx.x == 0) blockcount[blockIdx.x] = c;
}

// uvs[mask]: the kept rows in their own order
template <typename T>
__global__ __launch_bounds__(256) void k_ep_overlap_emit(const T* __restrict__ uv1, const T* __restrict__ uv2, size_t n, int stride,
                                                         const uint8_t* __restrict__ keep, const long long* __restrict__ start,
                                                         T* __restrict__ out1, T* __restrict__ out2, size_t capacity,
                                                         unsigned long long* __restrict__ count)
{
    __shared__ uint32_t wcnt[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *count = (unsigned long long)start[gridDim.x];
    const bool on = i < n && keep[i] != 0;
    const unsigned long long pos = block_slot(on, (unsigned long long)start[blockIdx.x], wcnt);
    if (on && pos < capacity) {
        out1[pos * 2] = uv1[i * stride]; out1[pos * 2 + 1] = uv1[i * stride + 1];
        out2[pos * 2] = uv2[i * stride]; out2[pos * 2 + 1] = uv2[i * stride + 1];
    }
}

// ---- fixed-order sums --------------------------------------------------------------------------------------------------
// Q running sums per thread; thread t of block g adds rows g*256+t, +G*256, ... in that order (at most
// m = ceil(n / (256 G)) terms); block_tree (compact.hpp) adds the block's 256 threads (8 levels) and stores Q partials;
// k_ep_final (compact.hpp, shared with essential.hip): thread t adds partials t, t+256, t+512, t+768 as (p0 + p1) + (p2 + p3)
// (2 levels; absent ones are 0), then the same 8-level tree: d = 18 levels above the serial part, whatever n is.

struct EpPoses {
    double k1[9], k2[9], R[4][9], t[4][3];
};

// sums[c * 2 + 0 / 1] = sum of zs1 / zs2 over all matches under candidate c: each match is read once
__global__ __launch_bounds__(256) void k_ep_pose_partials(const double* __restrict__ uv1, const double* __restrict__ uv2, size_t n,
                                                          EpPoses m, double* __restrict__ partials)
{
    __shared__ double sh[256];
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        double x1[3], b[3];
        tri_rays(m.k1, m.k2, uv1[i * 2], uv1[i * 2 + 1], uv2[i * 2], uv2[i * 2 + 1], x1, b);
        for (int c = 0; c < 4; c++) {
            double z1, z2;
            tri_solve(x1, b, m.R[c], m.t[c], &z1, &z2);
            s[c * 2] += z1;
            s[c * 2 + 1] += z2;
        }
    }
    block_tree<8>(s, sh, partials + (size_t)blockIdx.x * 8);
}

// s[0] = sum of z[i] (idx == NULL) or of z[idx[i]]; s[1] = how many idx[i] lie outside [0, z_len) (they add nothing)
__global__ __launch_bounds__(256) void k_ep_vector_partials(const double* __restrict__ z, const long long* __restrict__ idx, size_t n,
                                                            size_t z_len, double* __restrict__ partials)
{
    __shared__ double sh[256];
    double s[2] = {0, 0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        if (!idx) { s[0] += z[i]; continue; }
        const long long j = idx[i];
        if (j >= 0 && (unsigned long long)j < z_len) s[0] += z[j];
        else s[1] += 1.0;
    }
    block_tree<2>(s, sh, partials + (size_t)blockIdx.x * 2);
}

// ---- flow ------------------------------------------------------------------------------------------------------------
// xys_abs = (np.mgrid[:h, :w] + 0.5 - 1e-8)[::-1]: the float64 sum (x + 0.5) - 1e-8; uvs_to = float64(flow) + xys_abs
template <typename F>
struct FlowRows : MaskOn {
    const F* flow;
    double *from, *to;
    __device__ __forceinline__ void emit(int x, int y, unsigned long long pos) const
    {
        const double fx = ((double)x + 0.5) - 1e-8, fy = ((double)y + 0.5) - 1e-8;
        const size_t p = ((size_t)y * w + x) * 2;
        from[pos * 2] = fx;
        from[pos * 2 + 1] = fy;
        to[pos * 2] = (double)flow[p] + fx;
        to[pos * 2 + 1] = (double)flow[p + 1] + fy;
    }
};

// np.float32(flow_abs.transpose(2, 0, 1) / [[[w]], [[h]]]): the quotient in float64, then the cast
template <typename F>
__global__ __launch_bounds__(256) void k_ep_flow_abs_to_normal(const F* __restrict__ flow, int w, int h, float* __restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x, npix = (size_t)w * h;
    if (p >= npix) return;
    out[p] = (float)__ddiv_rn((double)flow[p * 2], (double)w);
    out[npix + p] = (float)__ddiv_rn((double)flow[p * 2 + 1], (double)h);
}

// (flow * [[[tw]], [[th]]]).transpose(1, 2, 0): float64 products
template <typename F>
__global__ __launch_bounds__(256) void k_ep_flow_normal_to_abs(const F* __restrict__ flow, int w, int h, double tw, double th,
                                                               double* __restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x, npix = (size_t)w * h;
    if (p >= npix) return;
    out[p * 2] = (double)flow[p] * tw;
    out[p * 2 + 1] = (double)flow[npix + p] * th;
}

// ---- all triples of a reconstruction in one pass (calibrating_amd/reconstruction_epipolar_geometry.py) ------------------
// The same cells, grids and compaction as above, with blockIdx.y choosing the point set / the triple from a descriptor
// table in device memory.  Grids of several windows lie in one buffer at their grid_offset; the columns of all triples
// lie in one flat count / start array at their column_offset, so ONE scan serves all and a triple's pairs come out
// contiguous, at start[column_offset], in the order the single call gives them.
constexpr int EP_BOUNDS_BLOCKS = 32;

template <typename T>
__device__ __forceinline__ void ep_bounds_rows(const T* __restrict__ uv, size_t n, double* lo, double* hi, int* nan)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)EP_BOUNDS_BLOCKS * 256)
        for (int k = 0; k < 2; k++) {
            const double x = (double)uv[i * 2 + k];
            if (x != x) *nan = 1;
            lo[k] = fmin(lo[k], x);
            hi[k] = fmax(hi[k], x);
        }
}

// bounds[(set * EP_BOUNDS_BLOCKS + block) * 4 ..] = min u, min v, max u, max v of the block's rows (+inf / -inf where it
// has none, NaN where a coordinate is NaN): min and max commute, so the host's minimum over the blocks is exact
__global__ __launch_bounds__(256) void k_ep_bounds_batch(const camd_cell_set* __restrict__ sets, double* __restrict__ bounds)
{
    __shared__ double sh[4][4];
    const camd_cell_set s = sets[blockIdx.y];
    double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    int nan = 0;
    with_float(s.uv_type, [&](auto v) { ep_bounds_rows((const decltype(v)*)s.uv, (size_t)s.n, lo, hi, &nan); });
    double v[4] = {lo[0], lo[1], -hi[0], -hi[1]};  // four minima
    for (int k = 0; k < 4; k++) {
        for (int o = 32; o > 0; o >>= 1) v[k] = fmin(v[k], __shfl_down(v[k], o));
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = v[k];
    }
    nan = __syncthreads_or(nan);
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        const double m = fmin(fmin(sh[0][k], sh[1][k]), fmin(sh[2][k], sh[3][k]));
        bounds[((size_t)blockIdx.y * EP_BOUNDS_BLOCKS + blockIdx.x) * 4 + k] = nan ? NAN : (k < 2 ? m : -m);
    }
}

__global__ __launch_bounds__(256) void k_ep_first_batch(const camd_cell_set* __restrict__ sets, double d,
                                                        uint32_t* __restrict__ grids, unsigned long long* __restrict__ outside)
{
    const camd_cell_set s = sets[blockIdx.y];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n) return;
    const EpWin w = {s.cu0, s.cv0, s.cells_w, s.cells_h};
    size_t cell;
    const bool in = with_float(s.uv_type, [&](auto v) {
        using T = decltype(v);
        return ep_cell((const T*)s.uv, i, 2, (T)d, w, &cell);
    });
    if (!in) { atomicAdd(outside, 1ull); return; }
    atomicMin(grids + s.grid_offset + cell, (uint32_t)i);
}

// one workgroup per (u column, triple): k_row_count / k_row_emit of compact.hpp with the triple's grids
__global__ __launch_bounds__(256) void k_ep_isect_count_batch(const camd_cell_triple* __restrict__ triples,
                                                              const uint32_t* __restrict__ grids, uint32_t* __restrict__ colcount)
{
    __shared__ uint32_t part[4];
    const camd_cell_triple t = triples[blockIdx.y];
    const int cu = blockIdx.x;
    if (cu >= t.cells_w) return;
    const EpIsect f = {grids + t.grid_offset1, grids + t.grid_offset2, t.cells_h, nullptr, nullptr};
    uint32_t c = 0;
    for (int v = threadIdx.x; v < t.cells_h; v += 256) c += f.on(v, cu) ? 1u : 0u;
    c = block_total(wave_sum(c), part);
    if (threadIdx.x == 0) colcount[t.column_offset + cu] = c;
}

__global__ __launch_bounds__(256) void k_ep_isect_emit_batch(const camd_cell_triple* __restrict__ triples,
                                                             const uint32_t* __restrict__ grids,
                                                             const unsigned long long* __restrict__ start, long long* idx1,
                                                             long long* idx2, size_t capacity, unsigned long long* __restrict__ counts)
{
    __shared__ uint32_t wcnt[4];
    __shared__ unsigned long long run;
    const camd_cell_triple t = triples[blockIdx.y];
    const int cu = blockIdx.x;
    if (cu >= t.cells_w) return;
    const EpIsect f = {grids + t.grid_offset1, grids + t.grid_offset2, t.cells_h, idx1, idx2};
    if (threadIdx.x == 0) {
        run = start[t.column_offset + cu];
        if (cu == 0) counts[blockIdx.y] = start[t.column_offset + t.cells_w] - start[t.column_offset];
    }
    __syncthreads();
    for (int base = 0; base < t.cells_h; base += 256) {
        const int v = base + threadIdx.x;
        const bool on = v < t.cells_h && f.on(v, cu);
        const unsigned long long pos = block_slot(on, run, wcnt);
        if (on && pos < capacity) f.emit(v, cu, pos);
        __syncthreads();
        if (threadIdx.x == 0) run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

// ---- the per-view depth rows [u, v, z, other view] ---------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_ep_uvzi_pack(const T* __restrict__ uv, const double* __restrict__ z, size_t n, double view,
                                                      double* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i * 4] = (double)uv[i * 2];
    out[i * 4 + 1] = (double)uv[i * 2 + 1];
    out[i * 4 + 2] = z[i];
    out[i * 4 + 3] = view;
}

// s[0] = sum of a[i * stride], i < n: the shape of k_ep_vector_partials
__global__ __launch_bounds__(256) void k_ep_column_partials(const double* __restrict__ a, size_t n, int stride,
                                                            double* __restrict__ partials)
{
    __shared__ double sh[256];
    double s[1] = {0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) s[0] += a[i * stride];
    block_tree<1>(s, sh, partials + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_ep_column_scale(double* __restrict__ a, size_t n, int stride, double rate)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i * stride] *= rate;
}

static int make_window(EpWin* w, int cu0, int cv0, int cells_w, int cells_h, const char* who)
{
    if (cells_w <= 0 || cells_h <= 0 || (unsigned long long)cells_w * (unsigned long long)cells_h > EP_MAX_CELLS) {
        set_error("%s: a window of %d x %d cells is empty or beyond 2^28 cells", who, cells_w, cells_h);
        return CAMD_ERR_BAD_ARG;
    }
    if ((long long)cu0 + cells_w > 0x7fffffffll || (long long)cv0 + cells_h > 0x7fffffffll) {
        set_error("%s: the window leaves the int32 cell range", who);
        return CAMD_ERR_BAD_ARG;
    }
    w->cu0 = cu0; w->cv0 = cv0; w->cw = cells_w; w->ch = cells_h;
    return CAMD_OK;
}


template <bool FIRST>
static int cells_entry(const char* who, const void* uv, int uv_type, size_t n, int uv_stride, double d, int cu0, int cv0,
                       int cells_w, int cells_h, uint32_t* grid, unsigned long long* outside, void* stream)
{
    EpWin w;
    int rc = make_window(&w, cu0, cv0, cells_w, cells_h, who);
    if (rc != CAMD_OK) return rc;
    if (!grid || !outside || uv_stride < 2 || (n && !uv) || !float_type_ok(uv_type) || !(d > 0.0) || (unsigned long long)n >= 0xffffffffull) {
        set_error("%s: bad arguments", who);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const size_t ncell = (size_t)cells_w * cells_h;
    fill(grid, ncell, FIRST ? EP_EMPTY : 0u, outside, st);
    if (n) {
        const dim3 g(div_up((long long)n, 256));
        with_float(uv_type, [&](auto v) {
            using T = decltype(v);
            hipLaunchKernelGGL((k_ep_cells<T, FIRST>), g, dim3(256), 0, st, (const T*)uv, n, uv_stride, (T)d, w, grid, outside);
        });
    }
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}


// the tables are checked on the host, entry by entry, before anything indexes device memory with them
static int upload(const void* host, size_t bytes, void* dev, hipStream_t st, const char* who)
{
    const hipError_t e = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { set_error("%s: hipMemcpyAsync: %s", who, hipGetErrorString(e)); return CAMD_ERR_HIP; }
    return CAMD_OK;
}

static int check_sets(const char* who, const camd_cell_set* sets, int nsets, const void* sets_dev, bool windows, size_t grid_cells,
                      size_t* max_n)
{
    if (!sets || !sets_dev || nsets <= 0 || nsets > 65535) {
        set_error("%s: 1 .. 65535 sets and both tables are required", who);
        return CAMD_ERR_BAD_ARG;
    }
    *max_n = 0;
    for (int k = 0; k < nsets; k++) {
        const camd_cell_set& s = sets[k];
        if (!float_type_ok(s.uv_type) || s.n >= 0xffffffffull || (s.n && !s.uv)) {
            set_error("%s: set %d: bad type, rows or pointer", who, k);
            return CAMD_ERR_BAD_ARG;
        }
        if (windows) {
            EpWin w;
            const int rc = make_window(&w, s.cu0, s.cv0, s.cells_w, s.cells_h, who);
            if (rc != CAMD_OK) return rc;
            if (s.grid_offset > grid_cells || (size_t)s.cells_w * s.cells_h > grid_cells - s.grid_offset) {
                set_error("%s: set %d: its grid leaves the %zu cells given", who, k, grid_cells);
                return CAMD_ERR_BAD_ARG;
            }
        }
        if (s.n > *max_n) *max_n = (size_t)s.n;
    }
    return CAMD_OK;
}

static int check_triples(const char* who, const camd_cell_triple* triples, int ntriples, const void* triples_dev, size_t grid_cells,
                         size_t ncols, int* max_w)
{
    if (!triples || !triples_dev || ntriples <= 0 || ntriples > 65535) {
        set_error("%s: 1 .. 65535 triples and both tables are required", who);
        return CAMD_ERR_BAD_ARG;
    }
    *max_w = 0;
    for (int k = 0; k < ntriples; k++) {
        const camd_cell_triple& t = triples[k];
        EpWin w;
        const int rc = make_window(&w, 0, 0, t.cells_w, t.cells_h, who);
        if (rc != CAMD_OK) return rc;
        const size_t cells = (size_t)t.cells_w * t.cells_h;
        if (t.grid_offset1 > grid_cells || cells > grid_cells - t.grid_offset1 || t.grid_offset2 > grid_cells ||
            cells > grid_cells - t.grid_offset2 || t.column_offset > ncols || (size_t)t.cells_w > ncols - t.column_offset) {
            set_error("%s: triple %d: its grids or columns leave the %zu cells / %zu columns given", who, k, grid_cells, ncols);
            return CAMD_ERR_BAD_ARG;
        }
        if (t.cells_w > *max_w) *max_w = t.cells_w;
    }
    return CAMD_OK;
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_cell_first_index(const void* uv, int uv_type, size_t n, int uv_stride, double max_distance, int cu0, int cv0,
                          int cells_w, int cells_h, uint32_t* first, unsigned long long* outside, void* stream)
{
    return cells_entry<true>("camd_cell_first_index", uv, uv_type, n, uv_stride, max_distance, cu0, cv0, cells_w, cells_h, first,
                             outside, stream);
}

int camd_cell_population(const void* uv, int uv_type, size_t n, int uv_stride, int cu0, int cv0, int cells_w, int cells_h,
                         uint32_t* population, unsigned long long* outside, void* stream)
{
    return cells_entry<false>("camd_cell_population", uv, uv_type, n, uv_stride, 1.0, cu0, cv0, cells_w, cells_h, population,
                              outside, stream);
}

int camd_cell_intersect_count(const uint32_t* first1, const uint32_t* first2, int cells_w, int cells_h, uint32_t* colcount,
                              void* stream)
{
    EpWin w;
    int rc = make_window(&w, 0, 0, cells_w, cells_h, "camd_cell_intersect_count");
    if (rc != CAMD_OK) return rc;
    if (!first1 || !first2 || !colcount) { set_error("camd_cell_intersect_count: NULL argument"); return CAMD_ERR_BAD_ARG; }
    CAMD_NEED_DEVICE();
    row_count(EpIsect{first1, first2, cells_h, nullptr, nullptr}, cells_h, cells_w, colcount, (hipStream_t)stream);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_cell_intersect_emit(const uint32_t* first1, const uint32_t* first2, int cells_w, int cells_h, const long long* start,
                             long long* idx1, long long* idx2, size_t capacity, unsigned long long* count, void* stream)
{
    EpWin w;
    int rc = make_window(&w, 0, 0, cells_w, cells_h, "camd_cell_intersect_emit");
    if (rc != CAMD_OK) return rc;
    if (!first1 || !first2 || !start || !count || (capacity && (!idx1 || !idx2))) {
        set_error("camd_cell_intersect_emit: NULL argument");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    row_emit(EpIsect{first1, first2, cells_h, idx1, idx2}, cells_h, cells_w, (const unsigned long long*)start, capacity, count,
             (hipStream_t)stream);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_overlap_blocks(size_t n) { return div_up((long long)n, 256); }

int camd_overlap_keep(const void* uv1, const void* uv2, int uv_type, size_t n, int uv_stride, int cu0, int cv0, int cells_w,
                      int cells_h, const uint32_t* population1, const uint32_t* population2, uint8_t* keep,
                      uint32_t* blockcount, void* stream)
{
    EpWin w;
    int rc = make_window(&w, cu0, cv0, cells_w, cells_h, "camd_overlap_keep");
    if (rc != CAMD_OK) return rc;
    if (!population1 || !population2 || uv_stride < 2 || !float_type_ok(uv_type) || (unsigned long long)n >= 0xffffffffull ||
        (n && (!uv1 || !uv2 || !keep || !blockcount))) {
        set_error("camd_overlap_keep: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    if (n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    const dim3 g(camd_overlap_blocks(n));
    with_float(uv_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_ep_overlap_keep<T>), g, dim3(256), 0, (hipStream_t)stream, (const T*)uv1, (const T*)uv2, n,
                           uv_stride, w, population1, population2, keep, blockcount);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_overlap_emit(const void* uv1, const void* uv2, int uv_type, size_t n, int uv_stride, const uint8_t* keep,
                      const long long* start, void* out1, void* out2, size_t capacity, unsigned long long* count, void* stream)
{
    if (!count || uv_stride < 2 || !float_type_ok(uv_type) || (unsigned long long)n >= 0xffffffffull ||
        (n && (!uv1 || !uv2 || !keep || !start)) || (capacity && (!out1 || !out2))) {
        set_error("camd_overlap_emit: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        fill((uint32_t*)nullptr, 0, 0u, count, st);
    } else {
        const dim3 g(camd_overlap_blocks(n));
        with_float(uv_type, [&](auto v) {
            using T = decltype(v);
            hipLaunchKernelGGL((k_ep_overlap_emit<T>), g, dim3(256), 0, st, (const T*)uv1, (const T*)uv2, n, uv_stride, keep,
                               start, (T*)out1, (T*)out2, capacity, count);
        });
    }
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_epipolar_sums_blocks(size_t n) { return sum_blocks(n); }

int camd_epipolar_sums(const double* uv1, const double* uv2, size_t n, const double K1inv[9], const double K2inv[9],
                       const double T_1to2[64], double* partials_ws, double* sums, void* stream)
{
    if (!uv1 || !uv2 || !K1inv || !K2inv || !T_1to2 || !partials_ws || !sums || n == 0) {
        set_error("camd_epipolar_sums: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    EpPoses m;
    for (int i = 0; i < 9; i++) { m.k1[i] = K1inv[i]; m.k2[i] = K2inv[i]; }
    for (int c = 0; c < 4; c++) {
        for (int i = 0; i < 9; i++) m.R[c][i] = T_1to2[c * 16 + (i / 3) * 4 + i % 3];
        for (int i = 0; i < 3; i++) m.t[c][i] = T_1to2[c * 16 + i * 4 + 3];
    }
    hipStream_t st = (hipStream_t)stream;
    const int g = sum_blocks(n);
    hipLaunchKernelGGL(k_ep_pose_partials, dim3(g), dim3(256), 0, st, uv1, uv2, n, m, partials_ws);
    hipLaunchKernelGGL((k_ep_final<8>), dim3(1), dim3(256), 0, st, partials_ws, g, sums);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_vector_sum_blocks(size_t n) { return sum_blocks(n); }

int camd_vector_sum(const double* z, size_t z_len, const long long* idx, size_t n, double* partials_ws, double* sums,
                    void* stream)
{
    if (!z || !partials_ws || !sums || n == 0 || (!idx && n > z_len)) {
        set_error("camd_vector_sum: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const int g = sum_blocks(n);
    hipLaunchKernelGGL(k_ep_vector_partials, dim3(g), dim3(256), 0, st, z, idx, n, z_len, partials_ws);
    hipLaunchKernelGGL((k_ep_final<2>), dim3(1), dim3(256), 0, st, partials_ws, g, sums);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_flow_to_matched_uvs(const void* flow_abs, int flow_type, const uint8_t* mask, int w, int h, double* uvs_from,
                             double* uvs_to, size_t capacity, unsigned long long* count, void* workspace, void* stream)
{
    if (!flow_abs || !mask || !count || !workspace || w <= 0 || h <= 0 || !float_type_ok(flow_type) ||
        (capacity && (!uvs_from || !uvs_to))) {
        set_error("camd_flow_to_matched_uvs: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const RowWorkspace ws(workspace, h);
    const MaskOn on = {mask, w};
    mask_row_count(on, h, ws.rowcount, st);
    row_scan(ws.rowcount, h, ws.rowoff, count, st);
    with_float(flow_type, [&](auto v) {
        using T = decltype(v);
        row_emit(FlowRows<T>{on, (const T*)flow_abs, uvs_from, uvs_to}, w, h, ws.rowoff, capacity, nullptr, st);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_flow_abs_to_normal(const void* flow_abs, int flow_type, int w, int h, float* flow_normal, void* stream)
{
    if (!flow_abs || !flow_normal || w <= 0 || h <= 0 || !float_type_ok(flow_type)) {
        set_error("camd_flow_abs_to_normal: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const dim3 g(div_up((long long)w * h, 256));
    with_float(flow_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_ep_flow_abs_to_normal<T>), g, dim3(256), 0, (hipStream_t)stream, (const T*)flow_abs, w, h,
                           flow_normal);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_flow_normal_to_abs(const void* flow_normal, int flow_type, int w, int h, double target_w, double target_h,
                            double* flow_abs, void* stream)
{
    if (!flow_normal || !flow_abs || w <= 0 || h <= 0 || !float_type_ok(flow_type)) {
        set_error("camd_flow_normal_to_abs: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const dim3 g(div_up((long long)w * h, 256));
    with_float(flow_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_ep_flow_normal_to_abs<T>), g, dim3(256), 0, (hipStream_t)stream, (const T*)flow_normal, w, h,
                           target_w, target_h, flow_abs);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_uv_bounds_blocks(void) { return EP_BOUNDS_BLOCKS; }

int camd_uv_bounds_batch(const camd_cell_set* sets_host, int nsets, camd_cell_set* sets_dev, double* bounds, void* stream)
{
    size_t max_n;
    int rc = check_sets("camd_uv_bounds_batch", sets_host, nsets, sets_dev, false, 0, &max_n);
    if (rc != CAMD_OK) return rc;
    if (!bounds) { set_error("camd_uv_bounds_batch: NULL argument"); return CAMD_ERR_BAD_ARG; }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    rc = upload(sets_host, sizeof(camd_cell_set) * nsets, sets_dev, st, "camd_uv_bounds_batch");
    if (rc != CAMD_OK) return rc;
    hipLaunchKernelGGL(k_ep_bounds_batch, dim3(EP_BOUNDS_BLOCKS, nsets), dim3(256), 0, st, sets_dev, bounds);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_cell_first_index_batch(const camd_cell_set* sets_host, int nsets, camd_cell_set* sets_dev, double max_distance,
                                uint32_t* grids, size_t grid_cells, unsigned long long* outside, void* stream)
{
    size_t max_n;
    int rc = check_sets("camd_cell_first_index_batch", sets_host, nsets, sets_dev, true, grid_cells, &max_n);
    if (rc != CAMD_OK) return rc;
    if (!grids || !outside || !(max_distance > 0.0)) { set_error("camd_cell_first_index_batch: bad arguments"); return CAMD_ERR_BAD_ARG; }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    rc = upload(sets_host, sizeof(camd_cell_set) * nsets, sets_dev, st, "camd_cell_first_index_batch");
    if (rc != CAMD_OK) return rc;
    fill(grids, grid_cells, EP_EMPTY, outside, st);
    if (max_n)
        hipLaunchKernelGGL(k_ep_first_batch, dim3(div_up((long long)max_n, 256), nsets), dim3(256), 0, st, sets_dev, max_distance,
                           grids, outside);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_cell_intersect_count_batch(const uint32_t* grids, size_t grid_cells, const camd_cell_triple* triples_host, int ntriples,
                                    camd_cell_triple* triples_dev, uint32_t* colcount, size_t ncols, void* stream)
{
    int max_w;
    int rc = check_triples("camd_cell_intersect_count_batch", triples_host, ntriples, triples_dev, grid_cells, ncols, &max_w);
    if (rc != CAMD_OK) return rc;
    if (!grids || !colcount) { set_error("camd_cell_intersect_count_batch: NULL argument"); return CAMD_ERR_BAD_ARG; }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    rc = upload(triples_host, sizeof(camd_cell_triple) * ntriples, triples_dev, st, "camd_cell_intersect_count_batch");
    if (rc != CAMD_OK) return rc;
    hipLaunchKernelGGL(k_ep_isect_count_batch, dim3(max_w, ntriples), dim3(256), 0, st, triples_dev, grids, colcount);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_cell_intersect_emit_batch(const uint32_t* grids, size_t grid_cells, const camd_cell_triple* triples_host, int ntriples,
                                   camd_cell_triple* triples_dev, const long long* start, size_t ncols, long long* idx1,
                                   long long* idx2, size_t capacity, unsigned long long* counts, void* stream)
{
    int max_w;
    int rc = check_triples("camd_cell_intersect_emit_batch", triples_host, ntriples, triples_dev, grid_cells, ncols, &max_w);
    if (rc != CAMD_OK) return rc;
    if (!grids || !start || !counts || (capacity && (!idx1 || !idx2))) {
        set_error("camd_cell_intersect_emit_batch: NULL argument");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    rc = upload(triples_host, sizeof(camd_cell_triple) * ntriples, triples_dev, st, "camd_cell_intersect_emit_batch");
    if (rc != CAMD_OK) return rc;
    hipLaunchKernelGGL(k_ep_isect_emit_batch, dim3(max_w, ntriples), dim3(256), 0, st, triples_dev, grids,
                       (const unsigned long long*)start, idx1, idx2, capacity, counts);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_uvzi_pack(const void* uv, int uv_type, const double* z, size_t n, double other_view, double* rows, size_t rows_total,
                   size_t row_offset, void* stream)
{
    if (!rows || !float_type_ok(uv_type) || row_offset > rows_total || n > rows_total - row_offset || (n && (!uv || !z))) {
        set_error("camd_uvzi_pack: bad arguments (rows %zu + %zu of %zu)", row_offset, n, rows_total);
        return CAMD_ERR_BAD_ARG;
    }
    if (n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    const dim3 g(div_up((long long)n, 256));
    double* out = rows + row_offset * 4;
    with_float(uv_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_ep_uvzi_pack<T>), g, dim3(256), 0, (hipStream_t)stream, (const T*)uv, z, n, other_view, out);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

static bool column_range_ok(size_t rows_total, int columns, int column, size_t row_offset, size_t n)
{
    return columns > 0 && column >= 0 && column < columns && row_offset <= rows_total && n <= rows_total - row_offset;
}

int camd_column_sum_blocks(size_t n) { return sum_blocks(n); }

int camd_column_sum(const double* rows, size_t rows_total, int columns, int column, size_t row_offset, size_t n,
                    double* partials_ws, double* sum, void* stream)
{
    if (!rows || !partials_ws || !sum || n == 0 || !column_range_ok(rows_total, columns, column, row_offset, n)) {
        set_error("camd_column_sum: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const int g = sum_blocks(n);
    hipLaunchKernelGGL(k_ep_column_partials, dim3(g), dim3(256), 0, st, rows + row_offset * columns + column, n, columns, partials_ws);
    hipLaunchKernelGGL((k_ep_final<1>), dim3(1), dim3(256), 0, st, partials_ws, g, sum);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_column_scale(double* rows, size_t rows_total, int columns, int column, size_t row_offset, size_t n, double rate,
                      void* stream)
{
    if (!rows || !column_range_ok(rows_total, columns, column, row_offset, n)) {
        set_error("camd_column_scale: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    if (n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_ep_column_scale, dim3(div_up((long long)n, 256)), dim3(256), 0, (hipStream_t)stream,
                       rows + row_offset * columns + column, n, columns, rate);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
