// chess_wave.hpp -- what the one-wavefront-per-frame stages of chessboard.hip and charuco.hip share: the butterflies that
// leave the same value in every lane, the nearest candidate by (squared distance, index), a lattice cell packed into an
// int.  The LDS fence of a wave's own slice (wave_lds_fence) and `uniform` come with pnp_common.hpp.
#pragma once
#include "pnp_common.hpp"

namespace camd {

constexpr unsigned long long CHESS_NONE = ~0ull;

__device__ __forceinline__ int pack_cell(int i, int j) { return (i + 1024) << 16 | (j + 1024); }

__device__ __forceinline__ unsigned long long wave_min_all(unsigned long long v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ long long wave_sum_all_i64(long long v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ int wave_max_all(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

// D: long long d(int k) -- the squared distance of candidate k, or -1 where it does not take part.  The least
// (distance, index) of the m candidates as distance << 10 | index, the same in every lane; CHESS_NONE where none takes part
template <typename D>
__device__ __forceinline__ unsigned long long nearest(int m, int lane, D d)
{
    unsigned long long best = CHESS_NONE;
    for (int k = lane; k < m; k += 64) {
        const long long v = d(k);
        const unsigned long long key = (unsigned long long)v << 10 | (unsigned)k;
        if (v >= 0 && key < best) best = key;
    }
    return wave_min_all(best);
}

}  // namespace camd
