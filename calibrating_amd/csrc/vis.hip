// vis.hip -- the pictures of utils.py for gfx950: depth error (vis_depth_l1), depth through a colour table (vis_depth)
// and the lined tiles of vis_stereo / vis_align.
//
// Replaces (file:line in the reference's calibrating/):
//   utils.py:486-575   vis_depth_l1: mask, l1, colour bar, the limit (np.partition), the colouring
//   utils.py:463-483   vis_depth: clip / normalise / slice / table lookup / zero mask        (camera.py:317-319 likewise)
//   utils.py:673-719   vis_stereo, vis_align: the coloured lines over two pictures
// Float64 arithmetic is NumPy's: every product, sum and quotient rounded once (__dmul_rn & co., never contracted).
// The limit of vis_depth_l1 is an exact selection: |l1| >= 0, so its bit pattern orders as an unsigned 64-bit integer,
// and a most-significant-digit radix select over 8 digits of 8 bits finds the key at a descending rank without a sort
// and without a host read: per digit one histogram kernel (LDS, then the non-empty bins to memory with integer
// atomics) and one pick kernel per image that fixes the digit and the rank left inside its bucket.
#include "compact.hpp"

namespace camd {

constexpr int SELECT_PASSES = 8, SELECT_BINS = 256;
constexpr int REDUCE_MAX_BLOCKS = 1024;  // blocks per image of a kernel that ends in one atomic per block
constexpr int HIST_MAX_BLOCKS = 256;     // blocks per image of the histogram (each flushes up to 256 bins)

struct SelectState {  // per image
    unsigned long long prefix;  // the digits fixed so far, in place
    unsigned long long rank;    // descending rank still to go inside the prefix' bucket
    unsigned long long valid_num;
    unsigned long long done;    // valid_num == 0: the limit is 1.0, nothing to select
};

struct L1Bar {  // the colour bar's rectangle [x0, x0 + bw) x [y0, y0 + bh); its values run along x or along y
    int x0, y0, bw, bh, along_x, length;
};

__device__ __forceinline__ double load_f64(const double* p, size_t i) { return p[i]; }
__device__ __forceinline__ double load_f64(const float* p, size_t i) { return (double)p[i]; }
__device__ __forceinline__ double load_f64(const uint16_t* p, size_t i) { return (double)p[i]; }

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // (false for NaN)

// np.linspace(-m * 1.1, m * 1.1, L)[i] in NumPy's arithmetic: arange * step + start, the last element set to the stop;
// a step that underflows to 0 takes NumPy's other branch (arange / div * delta), L == 1 has no step at all.
__device__ __forceinline__ double bar_value(int i, int L, double m)
{
    const double stop = __dmul_rn(m, 1.1), start = -stop;
    if (L > 1 && i == L - 1) return stop;
    const double delta = __dsub_rn(stop, start);
    if (L <= 1) return __dadd_rn(__dmul_rn((double)i, delta), start);
    const double div = (double)(L - 1), step = __ddiv_rn(delta, div);
    const double y = step == 0.0 ? __dmul_rn(__ddiv_rn((double)i, div), delta) : __dmul_rn((double)i, step);
    return __dadd_rn(y, start);
}

__device__ __forceinline__ bool in_bar(const L1Bar& b, int x, int y)
{
    return x >= b.x0 && x < b.x0 + b.bw && y >= b.y0 && y < b.y0 + b.bh;
}

// ---- vis_depth_l1, error pass ----------------------------------------------------------------------------------------
// l1 = (re - gt) * mask_valid, the bar written over it when its limit is known on the host (paint), the largest |l1| of
// the image (bits, atomicMax: exact whatever the order) and the count of non-finite inputs.  gt == NULL: the number
// gt_value everywhere.
template <typename T>
__global__ __launch_bounds__(256) void k_l1_error(const T* __restrict__ re, const T* __restrict__ gt, double gt_value, int w,
                                                  size_t npix, L1Bar bar, int paint, double bar_m, double* __restrict__ l1,
                                                  uint8_t* __restrict__ valid, unsigned long long* __restrict__ maxkey,
                                                  unsigned int* __restrict__ nonfinite)
{
    __shared__ uint32_t part[4];
    __shared__ unsigned long long wmax[4];
    const int z = blockIdx.y;
    const size_t base = (size_t)z * npix;
    unsigned long long top = 0;
    uint32_t bad = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        const double r = load_f64(re, base + i), g = gt ? load_f64(gt, base + i) : gt_value;
        bad += (!is_finite(r) || !is_finite(g)) ? 1u : 0u;
        bool ok = r != 0.0 && g != 0.0;
        double e = __dmul_rn(__dsub_rn(r, g), ok ? 1.0 : 0.0);
        if (paint) {
            const int y = (int)(i / (size_t)w), x = (int)(i - (size_t)y * w);
            if (in_bar(bar, x, y)) {
                e = bar_value(bar.along_x ? x - bar.x0 : y - bar.y0, bar.length, bar_m);
                ok = true;
            }
        }
        l1[base + i] = e;
        valid[base + i] = ok ? 1 : 0;
        const unsigned long long key = (unsigned long long)__double_as_longlong(fabs(e));
        top = key > top ? key : top;
    }
    top = wave_max(top);
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = top;
    bad = block_total(wave_sum(bad), part);  // (its barrier publishes wmax too)
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; k++) top = wmax[k] > top ? wmax[k] : top;
        if (top) atomicMax(maxkey + z, top);
        if (bad) atomicAdd(nonfinite, bad);
    }
}

// the bar painted after the limit was resolved on the device (max_l1=None with a colour bar); one lane per bar pixel
__global__ __launch_bounds__(256) void k_l1_bar(double* __restrict__ l1, uint8_t* __restrict__ valid, int w, size_t npix,
                                                L1Bar bar, const double* __restrict__ limit)
{
    const int z = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)bar.bw * bar.bh) return;
    const int by = (int)(i / (size_t)bar.bw), bx = (int)(i - (size_t)by * bar.bw);
    const size_t p = (size_t)z * npix + (size_t)(bar.y0 + by) * w + (bar.x0 + bx);
    l1[p] = bar_value(bar.along_x ? bx : by, bar.length, limit[z]);
    valid[p] = 1;
}

// ---- vis_depth_l1, the limit -------------------------------------------------------------------------------------------
__global__ void k_limit_fixed(double* __restrict__ limit, int batch, double m)
{
    const int z = blockIdx.x * 256 + threadIdx.x;
    if (z < batch) limit[z] = m;
}
__global__ void k_limit_from_max(double* __restrict__ limit, int batch, const unsigned long long* __restrict__ maxkey)
{
    const int z = blockIdx.x * 256 + threadIdx.x;
    if (z < batch) limit[z] = __longlong_as_double((long long)maxkey[z]);
}

// One digit's histogram among the valid keys that carry the prefix found so far.  A wave whose lanes mostly agree on
// the digit (the exponent digits of a depth error do) adds the leader's group with one LDS atomic.
__global__ __launch_bounds__(256) void k_select_hist(const double* __restrict__ l1, const uint8_t* __restrict__ valid,
                                                     size_t npix, int pass, const SelectState* __restrict__ state,
                                                     uint32_t* __restrict__ hist)
{
    __shared__ uint32_t bins[SELECT_BINS];
    const int z = blockIdx.y;
    const int shift = 64 - 8 * (pass + 1);
    const unsigned long long prefix = pass ? state[z].prefix >> (shift + 8) : 0;
    bins[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)z * npix;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(fabs(l1[base + i]));
        const bool on = valid[base + i] != 0 && (pass == 0 || (key >> (shift + 8)) == prefix);
        if (on) {
            const uint32_t d = (uint32_t)(key >> shift) & 0xffu;
            const uint32_t lead = __builtin_amdgcn_readfirstlane(d);
            const unsigned long long same = __ballot(d == lead);  // among the lanes inside this branch
            if (d != lead) atomicAdd(&bins[d], 1u);
            else if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(&bins[lead], (uint32_t)__popcll(same));
        }
    }
    __syncthreads();
    const uint32_t c = bins[threadIdx.x];
    if (c) atomicAdd(hist + ((size_t)z * SELECT_PASSES + pass) * SELECT_BINS + threadIdx.x, c);
}

// One workgroup per image: thread t owns bin 255 - t, so an inclusive scan over the threads counts the keys from the
// largest digit down; the bin where that count passes the rank is the digit, the rest of the rank goes to the next pass.
// Pass 0 also learns valid_num (the histogram's total) and from it k = int(frac * valid_num); the last pass has all 64
// bits of the key and writes the limit.
__global__ __launch_bounds__(256) void k_select_pick(const uint32_t* __restrict__ hist, int pass, double frac,
                                                     SelectState* __restrict__ state, double* __restrict__ limit)
{
    __shared__ uint32_t part[4];
    const int z = blockIdx.x, bin = SELECT_BINS - 1 - (int)threadIdx.x, lane = threadIdx.x & 63;
    const SelectState s = state[z];
    if (pass && s.done) return;
    const uint32_t c = hist[((size_t)z * SELECT_PASSES + pass) * SELECT_BINS + bin];
    uint32_t incl = c;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    const uint32_t total = block_total(__shfl(incl, 63), part);  // (pixels of one image: below 2^31, the entry checks)
    for (int k = 0; k < (int)(threadIdx.x >> 6); k++) incl += part[k];
    unsigned long long rank = s.rank, prefix = s.prefix;
    if (pass == 0) {
        prefix = 0;
        if (total == 0) {
            if (threadIdx.x == 0) {
                state[z] = SelectState{0, 0, 0, 1};
                limit[z] = 1.0;
            }
            return;
        }
        rank = (unsigned long long)__dmul_rn(frac, (double)total);  // int(-max_l1 * valid_num): truncation
        if (rank > total - 1) rank = total - 1;
    }
    const uint32_t excl = incl - c;
    if (rank >= excl && rank < incl) {  // exactly one thread: rank < total
        prefix |= (unsigned long long)bin << (64 - 8 * (pass + 1));
        state[z] = SelectState{prefix, rank - excl, pass ? s.valid_num : total, 0};
        if (pass == SELECT_PASSES - 1) limit[z] = __longlong_as_double((long long)prefix);
    }
}

// ---- vis_depth_l1, colour pass -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_l1_colour(const double* __restrict__ l1, const uint8_t* __restrict__ valid,
                                                   size_t npix, const double* __restrict__ limit, int overexposed,
                                                   uint8_t* __restrict__ dst)
{
    const int z = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const double e = l1[(size_t)z * npix + i], m = limit[z];
    const double mask = valid[(size_t)z * npix + i] ? 1.0 : 0.0;
    const bool pos = e > 0.0, neg = e < 0.0;
    const double ch[3] = {pos ? e : 0.0, neg ? -e : 0.0, 0.0};
    uint8_t px[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        // clip(0, m) / m; a limit of 0 is defined as the normalised value 0 (NumPy has 0 / 0 there)
        const double n = m == 0.0 ? 0.0 : __ddiv_rn(fmin(fmax(ch[c], 0.0), m), m);
        const double v = __dmul_rn(__dmul_rn(__dadd_rn(__dmul_rn(n, 1.0 - 0.1), 0.1), mask), 255.0);
        px[c] = (uint8_t)(int)v;  // 0 <= v <= 255: the cast truncates as np.uint8 does
    }
    if (overexposed && fabs(e) > m) {
        if (pos) px[1] = 255, px[2] = 0;
        if (neg) px[0] = 230, px[2] = 230;
    }
    uint8_t* o = dst + ((size_t)z * npix + i) * 3;
    o[0] = px[0], o[1] = px[1], o[2] = px[2];
}

// ---- vis_depth ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double depth_value(double d, double divisor, double clip_lo, double clip_hi, bool* zero)
{
    if (divisor != 1.0) d = __ddiv_rn(d, divisor);
    *zero = d == 0.0;
    return fmin(fmax(d, clip_lo), clip_hi);
}

__global__ void k_range_init(unsigned long long* __restrict__ keys, int batch)
{
    const int z = blockIdx.x * 256 + threadIdx.x;
    if (z < batch) keys[2 * z] = ~0ull, keys[2 * z + 1] = 0ull;
}

// keys[z] = {min, max} of image z's clipped values as order keys; NaN takes no part
template <typename T>
__global__ __launch_bounds__(256) void k_depth_range(const T* __restrict__ depth, size_t npix, double divisor, double clip_lo,
                                                     double clip_hi, unsigned long long* __restrict__ keys)
{
    __shared__ unsigned long long wlo[4], whi[4];
    const int z = blockIdx.y;
    unsigned long long lo = ~0ull, hi = 0ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        bool zero;
        const double d = depth_value(load_f64(depth, (size_t)z * npix + i), divisor, clip_lo, clip_hi, &zero);
        if (d == d) {
            const unsigned long long k = order_key(d);
            lo = k < lo ? k : lo;
            hi = k > hi ? k : hi;
        }
    }
    lo = wave_min(lo), hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) wlo[threadIdx.x >> 6] = lo, whi[threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; k++) lo = wlo[k] < lo ? wlo[k] : lo, hi = whi[k] > hi ? whi[k] : hi;
        atomicMin(keys + 2 * z, lo);
        atomicMax(keys + 2 * z + 1, hi);
    }
}

// range_mode 0: lo / den are the arguments; 1: lo = min, den = max - min of keys (norma); 2: lo = 0, den = max (d / d.max())
template <typename T>
__global__ __launch_bounds__(256) void k_vis_depth(const T* __restrict__ depth, size_t npix, double divisor, double clip_lo,
                                                   double clip_hi, double lo, double den,
                                                   const unsigned long long* __restrict__ keys, int range_mode, double slicen,
                                                   double scale, const uint8_t* __restrict__ table, int zero_mask,
                                                   uint8_t* __restrict__ dst)
{
    const int z = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    if (range_mode) {
        const double mn = order_value(keys[2 * z]), mx = order_value(keys[2 * z + 1]);
        lo = range_mode == 1 ? mn : 0.0;
        den = range_mode == 1 ? __dsub_rn(mx, mn) : mx;
    }
    bool zero;
    const double d = depth_value(load_f64(depth, (size_t)z * npix + i), divisor, clip_lo, clip_hi, &zero);
    double n = __ddiv_rn(__dsub_rn(d, lo), den);
    if (slicen != 0.0) {
        n = __dmul_rn(n, slicen);
        n = __dsub_rn(n, floor(n));  // np.mod(n, 1)
    }
    const double v = __dmul_rn(n, scale);
    const int idx = (v >= 0.0 && v < 256.0) ? (int)v : 0;  // (0 / 0 of a constant image, NaN: index 0)
    const uint8_t* t = table + 3 * idx;
    const bool black = zero_mask && zero;
    uint8_t* o = dst + ((size_t)z * npix + i) * 3;
    o[0] = black ? 0 : t[0], o[1] = black ? 0 : t[1], o[2] = black ? 0 : t[2];
}

// ---- vis_stereo / vis_align --------------------------------------------------------------------------------------------
__constant__ uint8_t LINE_COLOURS[6][3] = {{255, 0, 0}, {0, 255, 255}, {0, 255, 0}, {255, 0, 255}, {0, 0, 255}, {255, 255, 0}};

// Tile t of image z: 0 = img1, 1 = img2 (to its right), 2 = img2, 3 = img1 (the second row of vis_align).  rows[y] /
// cols[x + (t & 1) * w]: the colour index of the line through that row / column of the mosaic, -1 for none; columns are
// painted last in the reference, so they win.
__global__ __launch_bounds__(256) void k_vis_lines(const uint8_t* __restrict__ img1, int cn1, const uint8_t* __restrict__ img2,
                                                   int cn2, int w, size_t npix, const int8_t* __restrict__ rows,
                                                   const int8_t* __restrict__ cols, uint8_t* __restrict__ dst,
                                                   size_t dst_pitch, size_t tile_stride, size_t image_stride)
{
    const int z = blockIdx.y, t = blockIdx.z;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const int y = (int)(i / (size_t)w), x = (int)(i - (size_t)y * w);
    int c = cols ? cols[x + (t & 1) * w] : -1;
    if (c < 0) c = rows[y];
    uint8_t px[3];
    if (c >= 0) {
        px[0] = LINE_COLOURS[c][0], px[1] = LINE_COLOURS[c][1], px[2] = LINE_COLOURS[c][2];
    } else {
        const bool first = t == 0 || t == 3;
        const int cn = first ? cn1 : cn2;
        const uint8_t* s = (first ? img1 : img2) + ((size_t)z * npix + i) * cn;
        px[0] = s[0], px[1] = s[cn == 3 ? 1 : 0], px[2] = s[cn == 3 ? 2 : 0];
    }
    uint8_t* o = dst + (size_t)z * image_stride + (size_t)t * tile_stride + (size_t)y * dst_pitch + (size_t)x * 3;
    o[0] = px[0], o[1] = px[1], o[2] = px[2];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static int check_plane(const char* fn, int w, int h, int batch)
{
    if (w <= 0 || h <= 0 || batch <= 0 || batch > 65535) {
        set_error("%s: bad size %d x %d, batch %d (1 .. 65535)", fn, w, h, batch);
        return CAMD_ERR_BAD_ARG;
    }
    if ((long long)w * h > 2147483647LL) {
        set_error("%s: %d x %d pixels; a pixel count must fit an int32", fn, w, h);
        return CAMD_ERR_BAD_ARG;
    }
    return CAMD_OK;
}

static int check_pixels(const char* fn, size_t npix, int batch)
{
    if (npix == 0 || npix > 2147483647ull || batch <= 0 || batch > 65535) {
        set_error("%s: bad size: %zu pixels (1 .. 2^31 - 1), batch %d (1 .. 65535)", fn, npix, batch);
        return CAMD_ERR_BAD_ARG;
    }
    return CAMD_OK;
}

// the bar's rectangle as utils.py:519-546 places it
static int make_bar(const char* fn, int place, int width, int w, int h, L1Bar* bar)
{
    const bool along_x = place == CAMD_BAR_UP || place == CAMD_BAR_DOWN;
    if (place < CAMD_BAR_UP || place > CAMD_BAR_RIGHT || width < 0 || width > (along_x ? h : w)) {
        set_error("%s: colour bar %d of width %d does not fit %d x %d", fn, place, width, w, h);
        return CAMD_ERR_BAD_ARG;
    }
    if (along_x) *bar = L1Bar{0, place == CAMD_BAR_UP ? 0 : h - width, w, width, 1, w};
    else *bar = L1Bar{place == CAMD_BAR_LEFT ? 0 : w - width, 0, width, h, 0, h};
    return CAMD_OK;
}

static int reduce_blocks(size_t npix, int cap)
{
    const size_t g = (npix + 256 * 8 - 1) / (256 * 8);
    return (int)(g < 1 ? 1 : g > (size_t)cap ? (size_t)cap : g);
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_vis_l1_error(const void* re, const void* gt, double gt_value, int value_type, int w, int h, int batch, int bar_place,
                      int bar_width, double bar_max_l1, double* l1, uint8_t* valid, unsigned long long* maxkey,
                      unsigned int* nonfinite, void* stream)
{
    static const char* fn = "camd_vis_l1_error";
    int rc = check_plane(fn, w, h, batch);
    if (rc != CAMD_OK) return rc;
    if (!re || !l1 || !valid || !maxkey || !nonfinite || !float_type_ok(value_type)) {
        set_error("%s: bad arguments", fn);
        return CAMD_ERR_BAD_ARG;
    }
    L1Bar bar{0, 0, 0, 0, 0, 0};
    if (bar_place != CAMD_BAR_NONE && (rc = make_bar(fn, bar_place, bar_width, w, h, &bar)) != CAMD_OK) return rc;
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)w * h;
    CAMD_HIP(hipMemsetAsync(maxkey, 0, (size_t)batch * sizeof(unsigned long long), st));
    CAMD_HIP(hipMemsetAsync(nonfinite, 0, sizeof(unsigned int), st));
    const dim3 grid(reduce_blocks(npix, REDUCE_MAX_BLOCKS), batch);
    const int paint = bar_place != CAMD_BAR_NONE && bar.bw > 0 && bar.bh > 0;
    with_float(value_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_l1_error<T>), grid, dim3(256), 0, st, (const T*)re, (const T*)gt, gt_value, w, npix, bar, paint,
                           bar_max_l1, l1, valid, maxkey, nonfinite);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_vis_l1_bar(double* l1, uint8_t* valid, int w, int h, int batch, int bar_place, int bar_width, const double* limit,
                    void* stream)
{
    static const char* fn = "camd_vis_l1_bar";
    int rc = check_plane(fn, w, h, batch);
    if (rc != CAMD_OK) return rc;
    if (!l1 || !valid || !limit) {
        set_error("%s: bad arguments", fn);
        return CAMD_ERR_BAD_ARG;
    }
    L1Bar bar;
    if ((rc = make_bar(fn, bar_place, bar_width, w, h, &bar)) != CAMD_OK) return rc;
    CAMD_NEED_DEVICE();
    const size_t nbar = (size_t)bar.bw * bar.bh;
    if (nbar == 0) return CAMD_OK;
    hipLaunchKernelGGL(k_l1_bar, dim3(div_up((long long)nbar, 256), batch), dim3(256), 0, (hipStream_t)stream, l1, valid, w,
                       (size_t)w * h, bar, limit);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

size_t camd_vis_l1_limit_workspace_bytes(int batch)
{
    return batch > 0 ? (size_t)batch * (SELECT_PASSES * SELECT_BINS * sizeof(uint32_t) + sizeof(SelectState)) : 0;
}

int camd_vis_l1_limit(const double* l1, const uint8_t* valid, size_t npix, int batch, int mode, double value,
                      const unsigned long long* maxkey, void* workspace, double* limit, void* stream)
{
    static const char* fn = "camd_vis_l1_limit";
    int rc = check_pixels(fn, npix, batch);
    if (rc != CAMD_OK) return rc;
    if (!limit || mode < CAMD_LIMIT_FIXED || mode > CAMD_LIMIT_TOP) {
        set_error("%s: bad arguments", fn);
        return CAMD_ERR_BAD_ARG;
    }
    if (mode == CAMD_LIMIT_FIXED && !(value > 0.0 && value <= 1.7976931348623157e308)) {
        set_error("%s: a fixed limit must be positive and finite", fn);
        return CAMD_ERR_BAD_ARG;
    }
    if (mode == CAMD_LIMIT_MAX && !maxkey) {
        set_error("%s: NULL maxkey", fn);
        return CAMD_ERR_BAD_ARG;
    }
    if (mode == CAMD_LIMIT_TOP && (!(value > 0.0 && value < 1.0) || !l1 || !valid || !workspace)) {
        set_error("%s: the top fraction must lie inside (0, 1), with planes and a workspace", fn);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    if (mode == CAMD_LIMIT_FIXED) {
        hipLaunchKernelGGL(k_limit_fixed, dim3(div_up(batch, 256)), dim3(256), 0, st, limit, batch, value);
    } else if (mode == CAMD_LIMIT_MAX) {
        hipLaunchKernelGGL(k_limit_from_max, dim3(div_up(batch, 256)), dim3(256), 0, st, limit, batch, maxkey);
    } else {
        uint32_t* hist = (uint32_t*)workspace;
        SelectState* state = (SelectState*)(hist + (size_t)batch * SELECT_PASSES * SELECT_BINS);
        CAMD_HIP(hipMemsetAsync(workspace, 0, camd_vis_l1_limit_workspace_bytes(batch), st));
        const dim3 grid(reduce_blocks(npix, HIST_MAX_BLOCKS), batch);
        for (int pass = 0; pass < SELECT_PASSES; pass++) {
            hipLaunchKernelGGL(k_select_hist, grid, dim3(256), 0, st, l1, valid, npix, pass, state, hist);
            hipLaunchKernelGGL(k_select_pick, dim3(batch), dim3(256), 0, st, hist, pass, value, state, limit);
        }
    }
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_vis_l1_colour(const double* l1, const uint8_t* valid, size_t npix, int batch, const double* limit, int overexposed,
                       uint8_t* dst, void* stream)
{
    static const char* fn = "camd_vis_l1_colour";
    int rc = check_pixels(fn, npix, batch);
    if (rc != CAMD_OK) return rc;
    if (!l1 || !valid || !limit || !dst) {
        set_error("%s: bad arguments", fn);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_l1_colour, dim3(div_up((long long)npix, 256), batch), dim3(256), 0, (hipStream_t)stream, l1, valid,
                       npix, limit, overexposed, dst);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_vis_depth_range(const void* depth, int value_type, size_t npix, int batch, double divisor, double clip_lo,
                         double clip_hi, unsigned long long* keys, void* stream)
{
    static const char* fn = "camd_vis_depth_range";
    int rc = check_pixels(fn, npix, batch);
    if (rc != CAMD_OK) return rc;
    if (!depth || !keys || !float_u16_type_ok(value_type) || !(divisor > 0.0) || !(clip_lo <= clip_hi)) {
        set_error("%s: bad arguments", fn);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_range_init, dim3(div_up(batch, 256)), dim3(256), 0, st, keys, batch);
    const dim3 grid(reduce_blocks(npix, REDUCE_MAX_BLOCKS), batch);
    with_float_u16(value_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_depth_range<T>), grid, dim3(256), 0, st, (const T*)depth, npix, divisor, clip_lo, clip_hi, keys);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_vis_depth(const void* depth, int value_type, size_t npix, int batch, double divisor, double clip_lo, double clip_hi,
                   double lo, double den, const unsigned long long* keys, int range_mode, double slicen, double scale,
                   const uint8_t* table, int zero_mask, uint8_t* dst, void* stream)
{
    static const char* fn = "camd_vis_depth";
    int rc = check_pixels(fn, npix, batch);
    if (rc != CAMD_OK) return rc;
    if (!depth || !table || !dst || !float_u16_type_ok(value_type) || !(divisor > 0.0) || !(clip_lo <= clip_hi) ||
        range_mode < CAMD_RANGE_GIVEN || range_mode > CAMD_RANGE_MAX || (range_mode != CAMD_RANGE_GIVEN && !keys) ||
        !(scale > 0.0 && scale < 256.0) || !(slicen >= 0.0)) {
        set_error("%s: bad arguments", fn);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const dim3 grid(div_up((long long)npix, 256), batch);
    with_float_u16(value_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_vis_depth<T>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)depth, npix, divisor, clip_lo,
                           clip_hi, lo, den, keys, range_mode, slicen, scale, table, zero_mask, dst);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_vis_lines(const uint8_t* img1, int cn1, const uint8_t* img2, int cn2, int w, int h, int batch, const int8_t* rows,
                   const int8_t* cols, int tiles, uint8_t* dst, size_t dst_pitch, size_t tile_stride, size_t image_stride,
                   void* stream)
{
    static const char* fn = "camd_vis_lines";
    int rc = check_plane(fn, w, h, batch);
    if (rc != CAMD_OK) return rc;
    if (!img1 || !img2 || !rows || !dst || (cn1 != 1 && cn1 != 3) || (cn2 != 1 && cn2 != 3) || (tiles != 2 && tiles != 4) ||
        dst_pitch < (size_t)w * 3) {
        set_error("%s: bad arguments (images have 1 or 3 channels, 2 or 4 tiles, a pitch of at least a row)", fn);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_vis_lines, dim3(div_up((long long)w * h, 256), batch, tiles), dim3(256), 0, (hipStream_t)stream, img1,
                       cn1, img2, cn2, w, (size_t)w * h, rows, cols, dst, dst_pitch, tile_stride, image_stride);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
