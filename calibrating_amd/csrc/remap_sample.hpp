// remap_sample.hpp -- the one restatement of cv2's 8-bit fixed-point sampling, shared by the kernels that sample through
// a float map (remap.hip: the map comes from memory; flow.hip: the map is formed from a flow in registers).
// Arithmetic follows OpenCV's 8-bit fixed-point remap: 1/32-pixel phases, 15-bit int16 weights from a 32x32-entry table
// (sum forced to 32768), int32 accumulate, (sum + 16384) >> 15, BORDER_CONSTANT 0.
#pragma once

#include "common.hpp"

namespace camd {

enum { COEF_BITS = 15, COEF_SCALE = 1 << 15 };

// device copies of the Lanczos-4 / bilinear weight tables of the current device, created on first use (remap.hip)
int get_tables(const int16_t** lanczos, const int16_t** bilinear);

// RemapInvoker: float map * 32 in float, cvRound (half to even), split into the phase entry `a` and the cell, which
// becomes the window's first tap (ix, iy)
template <int KS>
__device__ __forceinline__ void map_to_window(float mx, float my, int& a, int& ix, int& iy)
{
    const int sx = __float2int_rn(mx * (float)INTER_TAB_SIZE);
    const int sy = __float2int_rn(my * (float)INTER_TAB_SIZE);
    a = (sy & (INTER_TAB_SIZE - 1)) * INTER_TAB_SIZE + (sx & (INTER_TAB_SIZE - 1));
    ix = min(max(sx >> INTER_BITS, -32768), 32767) - (KS / 2 - 1);
    iy = min(max(sy >> INTER_BITS, -32768), 32767) - (KS / 2 - 1);
}

// INTER_NEAREST: cvRound of the map, saturated to cv2's short coordinates
__device__ __forceinline__ void map_to_nearest(float mx, float my, int& sx, int& sy)
{
    sx = min(max(__float2int_rn(mx), -32768), 32767);
    sy = min(max(__float2int_rn(my), -32768), 32767);
}

// One row of a KS-wide window that starts `shb` bytes into raw[0]: funnel-shift the dwords into place
// (v_alignbyte), expand byte pairs to int16 pairs with one v_perm each and feed v_dot2_i32_i16 with the table's
// weight pairs -- 2 MACs per op instead of a byte load + mad per tap.
// MASKED: only window bytes [lo, hi) lie inside the image row; the rest become the constant border 0.
template <int KS, int CN, bool MASKED = false>
__device__ __forceinline__ void mac_window_row(const uint32_t (&raw)[(KS * CN + 3) / 4 + 1], uint32_t shb,
                                               const int16_t* __restrict__ wrow, int (&acc)[CN], int lo = 0,
                                               int hi = KS * CN)
{
    constexpr int NW = (KS * CN + 3) / 4;
    uint32_t win[NW + 1];
#pragma unroll
    for (int j = 0; j < NW; j++) {
        win[j] = __builtin_amdgcn_alignbyte(raw[j + 1], raw[j], shb);
        if (MASKED) {
            const int nlo = min(max(lo - 4 * j, 0), 4), nhi = min(max(hi - 4 * j, 0), 4);
            win[j] &= (uint32_t)((1ull << (8 * nhi)) - 1) & ~(uint32_t)((1ull << (8 * nlo)) - 1);
        }
    }
    win[NW] = 0;
    const uint32_t* wr = reinterpret_cast<const uint32_t*>(wrow);  // KS/2 weight pairs
#pragma unroll
    for (int q = 0; q < KS / 2; q++) {
        const uint32_t wq = wr[q];
#pragma unroll
        for (int c = 0; c < CN; c++) {
            const int b0 = (2 * q) * CN + c, j0 = b0 / 4, o0 = b0 % 4, o1 = o0 + CN;  // compile-time after unrolling
            const uint32_t sel = 0x0c000c00u | (uint32_t)o0 | ((uint32_t)o1 << 16);
            const uint32_t pr = __builtin_amdgcn_perm(win[j0 + 1], win[j0], sel);    // (tap 2q | tap 2q+1 << 16)
            acc[c] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2_t, pr), __builtin_bit_cast(s16x2_t, wq), acc[c],
                                            false);
        }
    }
}

template <int CN>
__device__ __forceinline__ void store_rounded(const int (&acc)[CN], uint8_t* out)
{
#ifdef CAMD_REMAP_DBG_NOSTORE  // measurement only (tools/microtests/remap_bench.hip): keep the arithmetic, drop the stores
    if (acc[0] != 0x12345678) return;
#endif
#pragma unroll
    for (int c = 0; c < CN; c++) {
        int v = (acc[c] + (1 << (COEF_BITS - 1))) >> COEF_BITS;
        out[c] = (uint8_t)min(max(v, 0), 255);
    }
}

// One row of a KS-wide window whose first byte is win[0]'s byte 0 (the interior path fetches the row from its own
// byte address, so nothing has to be shifted into place); weights come from registers.
template <int KS, int CN>
__device__ __forceinline__ void mac_row_regs(const uint32_t (&win)[(KS * CN + 3) / 4 + 1], const uint32_t* wq,
                                             int (&acc)[CN])
{
#pragma unroll
    for (int q = 0; q < KS / 2; q++) {
#pragma unroll
        for (int c = 0; c < CN; c++) {
            const int b0 = (2 * q) * CN + c, j0 = b0 / 4, o0 = b0 % 4, o1 = o0 + CN;  // compile-time after unrolling
            const uint32_t sel = 0x0c000c00u | (uint32_t)o0 | ((uint32_t)o1 << 16);
            const uint32_t pr = __builtin_amdgcn_perm(win[j0 + 1], win[j0], sel);    // (tap 2q | tap 2q+1 << 16)
            acc[c] = __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2_t, pr), __builtin_bit_cast(s16x2_t, wq[q]),
                                            acc[c], false);
        }
    }
}

// One destination pixel of `nz` images that share a map (a batch of one rig): KS x KS taps at (ix, iy) ..
// (ix+KS-1, iy+KS-1).  Everything that depends only on the map -- cell, phase, the weight entry (in registers:
// wreg), the interior test, the byte offset of the window -- is worked out once and applied to every image.
// A window row is fetched as aligned dwords (x4 + x3) and funnel-shifted into place; HR rows are requested at a time
// (KS / 2 for Lanczos: with the entry in registers and half the rows in flight the kernel needs 80 VGPRs and no LDS
// while it walks the images, so six waves per SIMD cover the gather's latency).
// Measured on 64 1080p RGB images, 16 images per workgroup (tools/microtests/remap_bench.hip; one image per workgroup
// and the entry behind an LDS slab, round 2's form: 2.95 ms): entry in LDS / registers at 117 VGPRs and 4 waves per
// SIMD 2.06 ms; registers, all 8 rows at once (97 VGPRs) 1.63; 4 rows at a time, 6 waves per SIMD 1.48; 2 rows at a
// time, 7 waves 1.68.  Slower and dropped: byte-exact misaligned row fetches 3.17, prefetching the next image's rows
// 2.56 (7 ms when capped at 128 VGPRs), staging the source box in LDS through registers 2.16 or by global_load_lds 3.5.
template <int KS, int CN, int HR>
__device__ __forceinline__ void gather_pixel_batch(const uint8_t* __restrict__ src, int sw, int sh, size_t pitch,
                                                   size_t src_stride, int ix, int iy,
                                                   const uint32_t (&wreg)[KS * KS / 2], uint8_t* out, size_t dst_stride,
                                                   int nz)
{
    constexpr int NB = KS * CN, NW = (NB + 3) / 4, NL = NW + 1;
    constexpr int OVER = (4 * (NW + 1) - NB + CN - 1) / CN, UNDER = (3 + CN - 1) / CN;
    const bool interior = ix >= UNDER && iy >= 0 && ix + KS + OVER <= sw && iy + KS <= sh;
    if (__all(interior)) {
        const uint8_t* pw = src + (size_t)iy * pitch + (size_t)ix * CN;
        const uint32_t shb = (uint32_t)(reinterpret_cast<uintptr_t>(pw) & 3);
        const uint8_t* p0 = pw - shb;
        uint32_t raw[HR][NL];
#pragma unroll 1
        for (int z = 0; z < nz; z++, p0 += src_stride, out += dst_stride) {
            int acc[CN];
#pragma unroll
            for (int c = 0; c < CN; c++) acc[c] = 0;
#pragma unroll
            for (int r0 = 0; r0 < KS; r0 += HR) {
#pragma unroll
                for (int r = 0; r < HR; r++) __builtin_memcpy(raw[r], p0 + (size_t)(r0 + r) * pitch, 4 * NL);
#pragma unroll
                for (int r = 0; r < HR; r++) {
                    uint32_t win[NW + 1];
#pragma unroll
                    for (int j = 0; j < NW; j++) win[j] = __builtin_amdgcn_alignbyte(raw[r][j + 1], raw[r][j], shb);
                    win[NW] = 0;
                    mac_row_regs<KS, CN>(win, wreg + (r0 + r) * (KS / 2), acc);
                }
                if (HR < KS) __builtin_amdgcn_sched_barrier(0);  // keep the next portion's loads behind this portion's use
            }
            store_rounded<CN>(acc, out);
        }
        return;
    }
    const bool touches = !(ix >= sw || ix + KS <= 0 || iy >= sh || iy + KS <= 0);
    const int lo = max(0, -ix * CN), hi = min(KS * CN, (sw - ix) * CN);
#pragma unroll 1
    for (int z = 0; z < nz; z++, src += src_stride, out += dst_stride) {
        int acc[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) acc[c] = 0;
        if (touches) {
            const uintptr_t img_lo = reinterpret_cast<uintptr_t>(src);
            const uintptr_t img_hi = img_lo + (size_t)(sh - 1) * pitch + (size_t)sw * CN;
#pragma unroll
            for (int r = 0; r < KS; r++) {  // (unrolled: the weights are registers, their index must be static)
                const int yy = iy + r;
                if (yy < 0 || yy >= sh) continue;
                const uintptr_t pa = img_lo + (uintptr_t)((long long)yy * (long long)pitch + (long long)ix * CN);
                const uintptr_t b = pa & ~(uintptr_t)3;
                uint32_t rw[NW + 1];
                if (b >= img_lo && b + 4 * (NW + 1) <= img_hi) {
#pragma unroll
                    for (int j = 0; j <= NW; j++) rw[j] = reinterpret_cast<const uint32_t*>(b)[j];
                } else {
#pragma unroll
                    for (int j = 0; j <= NW; j++) {
                        uint32_t v = 0;
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const uintptr_t q = b + 4 * j + k;
                            if (q >= img_lo && q < img_hi) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(q) << (8 * k);
                        }
                        rw[j] = v;
                    }
                }
                mac_window_row<KS, CN, true>(rw, (uint32_t)(pa & 3), reinterpret_cast<const int16_t*>(wreg + r * (KS / 2)), acc,
                                             lo, hi);
            }
        }
        store_rounded<CN>(acc, out);
    }
}

// The weight entry `a` of every lane, into registers.  Call it with all 256 lanes of the block (lanes without a pixel
// pass a = 0).  What bounded the Lanczos case first was fetching each pixel's own 128-byte weight entry: eight 16-byte
// loads per lane, every one touching 64 different cache lines.  So a wave fetches its 64 entries cooperatively into a
// wave-private LDS slab and every lane reads its own entry back -- in two halves of 64 bytes (four lanes per half
// entry: 64 contiguous bytes; slab stride 80 B: conflict-free ds_read_b128), 5 KB of LDS per wave, none of it needed
// once the entry is in registers.
template <int KS>
__device__ __forceinline__ void fetch_weight_entry(const int16_t* __restrict__ tab, int a, uint32_t (&wreg)[KS * KS / 2])
{
    if constexpr (KS == 8) {
        constexpr int HS = 80;
        __shared__ __attribute__((aligned(16))) uint8_t s_h[4][64 * HS];
        const int lane = threadIdx.x & 63;
        uint8_t* slab = s_h[threadIdx.x >> 6];
#pragma unroll
        for (int half = 0; half < 2; half++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int e = i * 16 + (lane >> 2);  // the lane whose half entry this group of four lanes fetches
                const int ae = __shfl(a, e);
                const uint4 v = *reinterpret_cast<const uint4*>(tab + (size_t)ae * 64 + half * 32 + (lane & 3) * 8);
                *reinterpret_cast<uint4*>(slab + e * HS + (lane & 3) * 16) = v;
            }
            // the slab is private to this wave and LDS executes a wave's operations in order: only the compiler
            // has to be kept from moving the reads above the writes (and the next half's writes above the reads)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint4 v = *reinterpret_cast<const uint4*>(slab + lane * HS + q * 16);
                wreg[half * 16 + 4 * q] = v.x;
                wreg[half * 16 + 4 * q + 1] = v.y;
                wreg[half * 16 + 4 * q + 2] = v.z;
                wreg[half * 16 + 4 * q + 3] = v.w;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    } else {
#pragma unroll
        for (int i = 0; i < KS * KS / 2; i++) wreg[i] = reinterpret_cast<const uint32_t*>(tab + (size_t)a * (KS * KS))[i];
    }
}

}  // namespace camd
