// compact.hpp -- the building blocks that pointcloud.hip, sparse.hip and epipolar.hip share: order-preserving compaction
// (count -> exclusive scan -> emit), the fixed-order block sum, the owner gather, the typed fill, and (with vis.hip) the
// wave reductions and the order key of a double.  Every block here is 256 threads = 4 waves of 64.
//
// A compaction writes the elements that pass a predicate, in their own order, to consecutive slots:
//   1  k_row_count   rowcount[y] = how many elements of row y pass               (one workgroup per row)
//   2  row_scan      rowoff = exclusive scan of rowcount, *total = the sum       (compact.hip, or the caller's cumsum)
//   3  k_row_emit    element x of row y goes to slot rowoff[y] + (passing elements before x in its row)
// Slots at or beyond `capacity` are not written; the total is reported in full whatever the capacity is.
// Kernels that more than one file launches are compiled once, in compact.hip, behind the host launchers declared below.
#pragma once

#include "common.hpp"

namespace camd {

// ---- counting -------------------------------------------------------------------------------------------------------
// the sum of the lanes' numbers, valid in lane 0 of the wave
__device__ __forceinline__ uint32_t wave_sum(uint32_t c)
{
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    return c;
}
// likewise the largest / the smallest of the lanes' numbers
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_down(v, o);
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_down(v, o);
        v = u < v ? u : v;
    }
    return v;
}

// order-preserving map double -> u64 and back (total order of the reals; -0.0 < +0.0): doubles as keys of the integer
// atomicMin / atomicMax, which are exact whatever order they are served in
__device__ __forceinline__ unsigned long long order_key(double d)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double order_value(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}

// the four waves' numbers (lane 0 of each holds its wave's) added up, returned to every thread.  part: __shared__
// uint32_t[4], free to be reused after the next barrier
__device__ __forceinline__ uint32_t block_total(uint32_t wave_n, uint32_t* part)
{
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = wave_n;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// how many threads of the block pass (every thread of the block must arrive)
__device__ __forceinline__ uint32_t block_count(bool on, uint32_t* part) { return block_total(__popcll(__ballot(on)), part); }

// position of this thread's element among the `on` elements of the block's current 256, after `run`.  Leaves the
// waves' counts in wcnt (__shared__ uint32_t[4]): the caller adds them to `run` behind a barrier before the next call.
__device__ __forceinline__ unsigned long long block_slot(bool on, unsigned long long run, uint32_t* wcnt)
{
    const unsigned long long bal = __ballot(on);
    const uint32_t below = __popcll(bal & ((1ull << (threadIdx.x & 63)) - 1ull));
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    unsigned long long pos = run + below;
    for (int k = 0; k < (int)(threadIdx.x >> 6); k++) pos += wcnt[k];
    return pos;
}

// On: bool on(int x, int y) const -- does element x of row y pass?
template <typename On>
__global__ __launch_bounds__(256) void k_row_count(On f, int w, uint32_t* __restrict__ rowcount)
{
    __shared__ uint32_t part[4];
    const int y = blockIdx.x;
    uint32_t c = 0;
    for (int x = threadIdx.x; x < w; x += 256) c += f.on(x, y) ? 1u : 0u;  // (independent loads: they overlap)
    c = block_total(wave_sum(c), part);
    if (threadIdx.x == 0) rowcount[y] = c;
}

// F: an On with void emit(int x, int y, unsigned long long pos) const, called for the passing elements whose slot is
// below capacity.  rowoff[y] is where row y starts; total != NULL: *total = rowoff[number of rows] (a scan the caller
// made has its sum there; row_scan reports the sum itself).
template <typename F>
__global__ __launch_bounds__(256) void k_row_emit(F f, int w, const unsigned long long* __restrict__ rowoff, size_t capacity,
                                                  unsigned long long* __restrict__ total)
{
    __shared__ uint32_t wcnt[4];
    __shared__ unsigned long long run;
    const int y = blockIdx.x;
    if (threadIdx.x == 0) {
        run = rowoff[y];
        if (total && y == 0) *total = rowoff[gridDim.x];
    }
    __syncthreads();
    for (int base = 0; base < w; base += 256) {
        const int x = base + threadIdx.x;
        const bool on = x < w && f.on(x, y);
        const unsigned long long pos = block_slot(on, run, wcnt);
        if (on && pos < capacity) f.emit(x, y, pos);
        __syncthreads();
        if (threadIdx.x == 0) run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

template <typename On>
void row_count(const On& f, int w, int rows, uint32_t* rowcount, hipStream_t st)
{
    hipLaunchKernelGGL((k_row_count<On>), dim3(rows), dim3(256), 0, st, f, w, rowcount);
}
template <typename F>
void row_emit(const F& f, int w, int rows, const unsigned long long* rowoff, size_t capacity, unsigned long long* total,
              hipStream_t st)
{
    hipLaunchKernelGGL((k_row_emit<F>), dim3(rows), dim3(256), 0, st, f, w, rowoff, capacity, total);
}

// a row-major uint8 mask as the predicate
struct MaskOn {
    const uint8_t* mask;
    int w;
    __device__ __forceinline__ bool on(int x, int y) const { return mask[(size_t)y * w + x] != 0; }
};

// the workspace of a compaction over `rows` rows: rowoff[rows] (u64), then rowcount[rows] (u32)
struct RowWorkspace {
    unsigned long long* rowoff;
    uint32_t* rowcount;
    RowWorkspace(void* ws, int rows)
        : rowoff(reinterpret_cast<unsigned long long*>(ws)), rowcount(reinterpret_cast<uint32_t*>(rowoff + rows)) {}
    static size_t bytes(int rows) { return rows > 0 ? (size_t)rows * (8 + 4) + 64 : 0; }
};

// ---- compiled once, in compact.hip ------------------------------------------------------------------------------------
// step 1 for a mask: row_count<MaskOn>, instantiated once (call this, not the template)
void mask_row_count(const MaskOn& f, int rows, uint32_t* rowcount, hipStream_t st);
// step 2: rowoff[i] = rowcount[0] + ... + rowcount[i - 1], *total = the sum of all n (one workgroup)
void row_scan(const uint32_t* rowcount, int n, unsigned long long* rowoff, unsigned long long* total, hipStream_t st);
// p[0 .. n) = v; zero != NULL: *zero = 0 in the same launch.  T = uint32_t or unsigned long long
template <typename T>
void fill(T* p, size_t n, T v, unsigned long long* zero, hipStream_t st);
// out[pix][c] = values[owner[pix] - 1][c]; where owner[pix] == 0: bg, or with keep != 0 what out held.
// value_type: CAMD_VALUE_F64 / F32 / U8 (the caller has checked it, and bg_value for uint8 unless keep)
void owner_gather(int value_type, const uint32_t* owner, size_t npix, const void* values, int channels, double bg_value,
                  int keep, void* out, hipStream_t st);

// ---- fixed-order sums -------------------------------------------------------------------------------------------------
// Q running sums per thread, the block adds its 256 threads by a binary tree (8 levels) and thread 0 stores dst[0 .. Q).
// sh: __shared__ double[256]
template <int Q>
__device__ __forceinline__ void block_tree(const double* s, double* sh, double* __restrict__ dst)
{
    for (int q = 0; q < Q; q++) {
        sh[threadIdx.x] = s[q];
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) dst[q] = sh[0];
        __syncthreads();
    }
}

constexpr int SUM_MAX_BLOCKS = 1024;  // partials of a fixed-order sum; k_ep_final adds four per thread

// blocks of a strided partial sum over n rows
static inline int sum_blocks(size_t n)
{
    const long long g = (long long)((n + 255) / 256);
    return (int)(g < 1 ? 1 : g > SUM_MAX_BLOCKS ? SUM_MAX_BLOCKS : g);
}

// the last step of such a sum (epipolar.hip, essential.hip), one workgroup: thread t adds the partials of blocks t, t + 256,
// t + 512, t + 768 as (p0 + p1) + (p2 + p3) (absent ones are 0), then the block's tree
template <int Q>
__device__ __forceinline__ void ep_final(const double* __restrict__ partials, int nblocks, double* __restrict__ sums, double* sh)
{
    double s[Q];
    for (int q = 0; q < Q; q++) {
        double p[4];
        for (int k = 0; k < 4; k++) {
            const int g = (int)threadIdx.x + 256 * k;
            p[k] = g < nblocks ? partials[(size_t)g * Q + q] : 0.0;
        }
        s[q] = (p[0] + p[1]) + (p[2] + p[3]);
    }
    block_tree<Q>(s, sh, sums);
}
template <int Q>
__global__ __launch_bounds__(256) void k_ep_final(const double* __restrict__ partials, int nblocks, double* __restrict__ sums)
{
    __shared__ double sh[256];
    ep_final<Q>(partials, nblocks, sums, sh);
}

}  // namespace camd
