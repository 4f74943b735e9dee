// marker_decode.hpp -- the marker inside four corners, by one wavefront: what charuco.hip (a lattice cell, the marker a
// share num / den of it) and markers.hip (a stand-alone marker's own outline, num / den = 1 / 1) share.  Integers only.
#pragma once
#include <climits>

#include "chess_wave.hpp"

namespace camd {

constexpr int CHARUCO_MIN_CONTRAST = 40;  // gray levels between a marker's darkest and brightest cell

struct MarkerImage {
    const uint8_t* img;  // the frame
    int w, h;
    size_t pitch;
};

// The marker of s x s bits in the cell with corners (x00, y00), (x10, y10) one step along i, (x01, y01) along j and
// (x11, y11): (s + 2)^2 samples placed by the fixed-point bilinear blend of the corners, 3 x 3 sums, thresholded midway
// between their extremes, a black ring, the bits matched in four turns against words[0 .. n_ids).  -> errors << 16 | id <<
// 2 | turn of the least (errors, id, turn) within max_errors, or CHESS_NONE; the same in every lane.  Lane l takes samples
// l and l + 64 (s <= 8: at most 100).
__device__ __forceinline__ unsigned long long decode_marker(const MarkerImage& B, int s, int num, int den,
                                                            const unsigned long long* __restrict__ words, int n_ids,
                                                            int max_errors, int lane, long long x00, long long y00,
                                                            long long x10, long long y10, long long x01, long long y01,
                                                            long long x11, long long y11)
{
    const int c = s + 2, cells = c * c;
    const long long D = 2 * den * c, DD = D * D;
    int val[2], lo = INT_MAX, hi = INT_MIN;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int idx = lane + 64 * r;
        val[r] = -1;
        if (idx < cells) {
            const int b = idx / c, a = idx - b * c;
            const long long wx = den * c + num * (2 * a + 1 - c), wy = den * c + num * (2 * b + 1 - c);
            const long long w00 = (D - wx) * (D - wy), w10 = wx * (D - wy), w01 = (D - wx) * wy, w11 = wx * wy;
            int px = (int)((w00 * x00 + w10 * x10 + w01 * x01 + w11 * x11 + DD / 2) / DD);
            int py = (int)((w00 * y00 + w10 * y10 + w01 * y01 + w11 * y11 + DD / 2) / DD);
            px = px < 1 ? 1 : px > B.w - 2 ? B.w - 2 : px;  // (a blend of corners 5 px inside the image is inside it: this only
            py = py < 1 ? 1 : py > B.h - 2 ? B.h - 2 : py;  //  keeps a caller's own peaks from reading outside the frame)
            int sum = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const uint8_t* row = B.img + (size_t)(py + dy) * B.pitch + px;
                sum += row[-1] + row[0] + row[1];
            }
            val[r] = sum;
            lo = sum < lo ? sum : lo, hi = sum > hi ? sum : hi;
        }
    }
    lo = -wave_max_all(-lo), hi = wave_max_all(hi);
    if (hi - lo < 9 * CHARUCO_MIN_CONTRAST) return CHESS_NONE;
    const unsigned long long f0 = __ballot(val[0] >= 0 && 2 * val[0] > lo + hi), f1 = __ballot(val[1] >= 0 && 2 * val[1] > lo + hi);
    auto bit = [&](int idx) { return (int)((idx < 64 ? f0 >> idx : f1 >> (idx - 64)) & 1ull); };
    int ring = 0;
    for (int a = 0; a < c; a++) ring |= bit(a) | bit((c - 1) * c + a) | bit(a * c) | bit(a * c + c - 1);
    if (ring) return CHESS_NONE;
    unsigned long long word[4] = {0, 0, 0, 0};  // the bits turned 0 .. 3 quarter turns, as np.rot90 turns them
    for (int r = 0; r < s; r++)
        for (int q = 0; q < s; q++) {
            word[0] = word[0] << 1 | (unsigned)bit((r + 1) * c + q + 1);
            word[1] = word[1] << 1 | (unsigned)bit((q + 1) * c + s - r);
            word[2] = word[2] << 1 | (unsigned)bit((s - r) * c + s - q);
            word[3] = word[3] << 1 | (unsigned)bit((s - q) * c + r + 1);
        }
    unsigned long long best = CHESS_NONE;
    for (int id = lane; id < n_ids; id += 64) {
        const unsigned long long dw = words[id];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int err = __popcll(word[k] ^ dw);
            const unsigned long long key = (unsigned long long)err << 16 | (unsigned)(id << 2 | k);
            if (err <= max_errors && key < best) best = key;
        }
    }
    return wave_min_all(best);
}

}  // namespace camd
