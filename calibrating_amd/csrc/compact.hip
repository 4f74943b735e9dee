// compact.hip -- the kernels of compact.hpp that more than one translation unit launches, compiled once
#include "compact.hpp"

namespace camd {

// exclusive scan of the row counts (one workgroup; rows <= a few thousand): 256 counts per iteration, `carry` is the sum
// of the iterations before
__global__ __launch_bounds__(256) void k_row_scan(const uint32_t* __restrict__ rowcount, int n,
                                                  unsigned long long* __restrict__ rowoff,
                                                  unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long carry;
    __shared__ unsigned long long wsum[4];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        unsigned long long v = i < n ? rowcount[i] : 0ull, incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            unsigned long long t = __shfl_up(incl, o);
            if ((threadIdx.x & 63) >= o) incl += t;
        }
        if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
        __syncthreads();
        unsigned long long before = carry;
        for (int k = 0; k < (int)(threadIdx.x >> 6); k++) before += wsum[k];
        if (i < n) rowoff[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 255) carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

template <typename T>
__global__ __launch_bounds__(256) void k_fill(T* __restrict__ p, size_t n, T v, unsigned long long* zero)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
    if (i == 0 && zero) *zero = 0ull;
}

template <typename V>
__global__ __launch_bounds__(256) void k_owner_gather(const uint32_t* __restrict__ owner, size_t npix,
                                                      const V* __restrict__ values, int channels, V bg, int keep,
                                                      V* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const uint32_t o = owner[i];
    if (o) {
        const V* src = values + (size_t)(o - 1u) * channels;
        for (int c = 0; c < channels; c++) out[i * channels + c] = src[c];
    } else if (!keep) {
        for (int c = 0; c < channels; c++) out[i * channels + c] = bg;
    }
}

void mask_row_count(const MaskOn& f, int rows, uint32_t* rowcount, hipStream_t st) { row_count(f, f.w, rows, rowcount, st); }

void row_scan(const uint32_t* rowcount, int n, unsigned long long* rowoff, unsigned long long* total, hipStream_t st)
{
    hipLaunchKernelGGL(k_row_scan, dim3(1), dim3(256), 0, st, rowcount, n, rowoff, total);
}

template <typename T>
void fill(T* p, size_t n, T v, unsigned long long* zero, hipStream_t st)
{
    hipLaunchKernelGGL((k_fill<T>), dim3(n ? div_up((long long)n, 256) : 1), dim3(256), 0, st, p, n, v, zero);
}
template void fill<uint32_t>(uint32_t*, size_t, uint32_t, unsigned long long*, hipStream_t);
template void fill<unsigned long long>(unsigned long long*, size_t, unsigned long long, unsigned long long*, hipStream_t);

void owner_gather(int value_type, const uint32_t* owner, size_t npix, const void* values, int channels, double bg_value,
                  int keep, void* out, hipStream_t st)
{
    with_float_u8(value_type, [&](auto v) {
        using V = decltype(v);
        const V bg = keep ? V(0) : (V)bg_value;  // (unread with keep, and unchecked then: it need not fit a uint8)
        hipLaunchKernelGGL((k_owner_gather<V>), dim3(div_up((long long)npix, 256)), dim3(256), 0, st, owner, npix,
                           (const V*)values, channels, bg, keep, (V*)out);
    });
}

}  // namespace camd
