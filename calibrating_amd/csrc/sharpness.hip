// sharpness.hip -- the sums behind the variance of a picture's Laplacian, for every frame of a batch.
//
//   reconstruction_with_board.py:9-12   cv2.Laplacian(gray, cv2.CV_64F).var()   -> camd_laplacian_sums
// The 3 x 3 Laplacian [0 1 0; 1 -4 1; 0 1 0] with reflect-101 borders; per frame the integer sums S1 = sum L and S2 = sum
// L^2 (include/calibrating_amd.h).  |L| <= 1020, so a frame of up to 2^31 pixels keeps S2 below
// 2^52.  Integers add in any order to the same bits: a thread sums its pixels, a wave meets in a butterfly and its first lane
// adds to the frame's two sums with an atomic.  No barrier, no LDS.
#include <algorithm>

#include "chess_wave.hpp"

namespace camd {

__global__ __launch_bounds__(256) void k_laplacian_sums(const uint8_t* __restrict__ gray, int w, int h, size_t pitch, size_t stride,
                                                       unsigned long long* __restrict__ sums)
{
    const uint8_t* img = gray + (size_t)blockIdx.y * stride;
    const long long pixels = (long long)w * h;
    long long s1 = 0, s2 = 0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long long)gridDim.x * 256) {
        const int y = (int)(p / w), x = (int)(p - (long long)y * w);
        const int xl = x == 0 ? 1 : x - 1, xr = x == w - 1 ? w - 2 : x + 1, yu = y == 0 ? 1 : y - 1, yd = y == h - 1 ? h - 2 : y + 1;
        const uint8_t* row = img + (size_t)y * pitch;
        const int l = row[xl] + row[xr] + img[(size_t)yu * pitch + x] + img[(size_t)yd * pitch + x] - 4 * row[x];
        s1 += l, s2 += l * l;
    }
    s1 = wave_sum_all_i64(s1), s2 = wave_sum_all_i64(s2);
    if ((threadIdx.x & 63) == 0) {  // (two's complement: the unsigned sum of S1's parts is S1)
        atomicAdd(&sums[2 * (size_t)blockIdx.y], (unsigned long long)s1);
        atomicAdd(&sums[2 * (size_t)blockIdx.y + 1], (unsigned long long)s2);
    }
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_laplacian_sums(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, long long* sums, void* queue)
{
    if (w < 2 || h < 2) {
        set_error("camd_laplacian_sums: an image of %d x %d; the mirrored border takes sides from 2", w, h);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (!gray || !sums || frames < 1 || frames > 65535 || (long long)w * h > (1ll << 31) || pitch < (size_t)w ||
        (frames > 1 && stride < (size_t)(h - 1) * pitch + (size_t)w) || (uintptr_t)sums % 8 != 0) {
        set_error("camd_laplacian_sums: bad arguments (gray, sums: device arrays, sums aligned to 8; frames 1 .. 65535; w h <= 2^31; "
                  "pitch >= w, stride >= an image)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    CAMD_HIP(hipMemsetAsync(sums, 0, (size_t)frames * 2 * sizeof(long long), (hipStream_t)queue));
    const int blocks = (int)std::min<long long>(div_up((long long)w * h, 256 * 8), 1024);
    hipLaunchKernelGGL(k_laplacian_sums, dim3(blocks, frames), dim3(256), 0, (hipStream_t)queue, gray, w, h, pitch, stride,
                       (unsigned long long*)sums);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
