// markers.hip -- stand-alone ArUco markers by id, in every frame of a recording at once.
//
// Stands where the reference calls cv2.aruco.detectMarkers (boards.py:280, 551) with a contract of its own (INTEGRATION.md
// section J): a marker's outer corners are L-corners on a quiet zone, where the ChESS response of chessboard.hip is silent,
// so the front end is another one.  Integers from the image to the coarse corners, restated by tests/markers_ref.py:
//   1  k_dark_mask          a pixel is dark iff (gray + offset) * A < S, S and A the sum and the size of its (2r + 1)^2 window
//                           inside the image: a separable box sum through an LDS tile with an r-pixel apron
//   2  k_label_*            the 4-connected components of the mask, a pixel's label the least y * w + x of its component:
//                           label equivalence -- a tile labelled in LDS, the tiles merged along their borders by atomicMin
//                           on roots, one flattening pass.  Links only ever point to a lower index, so a root is its
//                           set's minimum, the fixed point is unique, and no thread waits for another: every loop walks
//                           down a strictly falling chain, bounded by the component's size
//   3  k_marker_stats, MarkerCandidate   box and pixel count of every component at its root (integer atomics: exact in any
//                           order), the components of a marker's size compacted per frame in pixel order (compact.hpp)
//   4, 5  k_marker_quad     one wavefront per candidate, four per workgroup, no barrier and no atomic but the last: the
//                           outline's four extreme pixels by packed integer keys, the marker decoded inside them
//                           (marker_decode.hpp), its key written to its id by one atomicMin
//   6  k_marker_by_id       the winner of every (frame, id) gathered
// The mask and labelling passes are memory-bound: 1 B read, 1 B + 4 B written per pixel, the labels revisited.
#include <climits>
#include <cmath>

#include "compact.hpp"
#include "marker_decode.hpp"

namespace camd {

constexpr int MARKER_MAX_SIDE = 16384;                // of an image: y * w + x stays below 2^28
constexpr int MARKER_MAX_RADIUS = 32, MARKER_MAX_BOX = 1024, MARKER_MAX_BITS = 8;
constexpr int MASK_TW = 64, MASK_TH = 32;             // a workgroup's tile of the mask
constexpr int MASK_RW = MASK_TW + 2 * MARKER_MAX_RADIUS, MASK_RH = MASK_TH + 2 * MARKER_MAX_RADIUS;
constexpr int LABEL_TW = 32, LABEL_TH = 32;           // a labelling tile: 1024 pixels, four per thread
enum { MARKER_OVERFLOW = 2 };
static_assert(MASK_RW * MASK_RH + 2 * MASK_RH * MASK_TW <= 64 * 1024, "the staged tile and its row sums fit a workgroup's LDS");
static_assert((2 * MARKER_MAX_RADIUS + 1) * 255 < 65536, "a row sum fits 16 bits");

// ---- stage 1 ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dark_mask(const uint8_t* __restrict__ gray, int w, int h, size_t pitch, size_t stride,
                                                  int frames, int r, int offset, uint8_t* __restrict__ mask)
{
    __shared__ uint8_t raw[MASK_RH * MASK_RW];
    __shared__ uint16_t hs[MASK_RH * MASK_TW];
    const int x0 = (int)blockIdx.x * MASK_TW, y0 = (int)blockIdx.y * MASK_TH;
    const int rw = MASK_TW + 2 * r, rh = MASK_TH + 2 * r;
    for (int f = blockIdx.z; f < frames; f += gridDim.z) {
        const uint8_t* img = gray + (size_t)f * stride;
        for (int k = threadIdx.x; k < rh * rw; k += 256) {
            const int row = k / rw, col = k - row * rw, y = y0 - r + row, x = x0 - r + col;
            raw[row * MASK_RW + col] = (y >= 0 && y < h && x >= 0 && x < w) ? img[(size_t)y * pitch + x] : 0;  // (0: no part of S)
        }
        __syncthreads();
        for (int k = threadIdx.x; k < rh * MASK_TW; k += 256) {
            const int row = k / MASK_TW, col = k - row * MASK_TW;
            const uint8_t* p = raw + row * MASK_RW + col;
            int s = 0;
            for (int d = 0; d <= 2 * r; d++) s += p[d];
            hs[k] = (uint16_t)s;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < MASK_TH * MASK_TW; k += 256) {
            const int ly = k / MASK_TW, lx = k - ly * MASK_TW, x = x0 + lx, y = y0 + ly;
            if (x >= w || y >= h) continue;
            int S = 0;
            for (int d = 0; d <= 2 * r; d++) S += hs[(ly + d) * MASK_TW + lx];
            const int xa = x - r < 0 ? 0 : x - r, xb = x + r > w - 1 ? w - 1 : x + r;
            const int ya = y - r < 0 ? 0 : y - r, yb = y + r > h - 1 ? h - 1 : y + r;
            const int A = (xb - xa + 1) * (yb - ya + 1), g = raw[(ly + r) * MASK_RW + lx + r];
            mask[((size_t)f * h + y) * w + x] = (g + offset) * A < S ? 1 : 0;
        }
        __syncthreads();  // (the next frame's tile)
    }
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------
// the root of x: down a chain of strictly falling indices (a link never points up), so at most the set's size steps
__device__ __forceinline__ int label_find(const int* L, int x)
{
    for (;;) {
        const int p = __atomic_load_n(L + x, __ATOMIC_RELAXED);
        if (p == x) return x;
        x = p;
    }
}
// the sets of a and b become one: the higher root is linked to the lower.  Lock-free: a failed atomicMin means another
// thread has linked that root lower already, and this thread goes on from where that link points -- its own progress
__device__ __forceinline__ void label_union(int* L, int a, int b)
{
    for (;;) {
        a = label_find(L, a), b = label_find(L, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicMin(L + b, a);  // b > a
        if (old == b) return;
        b = old;
    }
}

// a tile labelled in LDS, written out as frame-wide indices
__global__ __launch_bounds__(256) void k_label_tile(const uint8_t* __restrict__ mask, int w, int h, int frames, int* __restrict__ labels)
{
    __shared__ int L[LABEL_TW * LABEL_TH];
    const int x0 = (int)blockIdx.x * LABEL_TW, y0 = (int)blockIdx.y * LABEL_TH;
    const int lx = threadIdx.x & 31, ty = threadIdx.x >> 5, x = x0 + lx;
    for (int f = blockIdx.z; f < frames; f += gridDim.z) {
        const uint8_t* m = mask + (size_t)f * h * w;
#pragma unroll
        for (int k = 0; k < LABEL_TH / 8; k++) {
            const int ly = ty + 8 * k, y = y0 + ly, l = ly * LABEL_TW + lx;
            L[l] = (x < w && y < h && m[(size_t)y * w + x]) ? l : -1;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LABEL_TH / 8; k++) {
            const int ly = ty + 8 * k, l = ly * LABEL_TW + lx;
            if (__atomic_load_n(L + l, __ATOMIC_RELAXED) < 0) continue;
            if (lx > 0 && __atomic_load_n(L + l - 1, __ATOMIC_RELAXED) >= 0) label_union(L, l, l - 1);
            if (ly > 0 && __atomic_load_n(L + l - LABEL_TW, __ATOMIC_RELAXED) >= 0) label_union(L, l, l - LABEL_TW);
        }
        __syncthreads();
        int root[LABEL_TH / 8];
#pragma unroll
        for (int k = 0; k < LABEL_TH / 8; k++) {
            const int l = (ty + 8 * k) * LABEL_TW + lx;
            root[k] = L[l] < 0 ? -1 : label_find(L, l);
        }
#pragma unroll
        for (int k = 0; k < LABEL_TH / 8; k++) {
            const int y = y0 + ty + 8 * k;
            if (x >= w || y >= h) continue;
            const int rt = root[k];
            labels[((size_t)f * h + y) * w + x] = rt < 0 ? -1 : (y0 + rt / LABEL_TW) * w + x0 + rt % LABEL_TW;
        }
        __syncthreads();  // (the next frame's tile)
    }
}

// the pixels of a tile's first column and first row joined to their neighbours in the tile before.  Thread k of a frame:
// first the (w - 1) / TW inner vertical borders, h pixels each, then the (h - 1) / TH horizontal ones, w pixels each
__global__ __launch_bounds__(256) void k_label_merge(int w, int h, int frames, int* __restrict__ labels)
{
    const int nbx = (w - 1) / LABEL_TW, nby = (h - 1) / LABEL_TH;
    const long long nv = (long long)nbx * h, total = nv + (long long)nby * w;
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= total) return;
    int x, y, other;
    if (k < nv) {
        x = ((int)(k / h) + 1) * LABEL_TW, y = (int)(k % h);
        other = y * w + x - 1;
    } else {
        const long long q = k - nv;
        y = ((int)(q / w) + 1) * LABEL_TH, x = (int)(q % w);
        other = (y - 1) * w + x;
    }
    const int p = y * w + x;
    for (int f = blockIdx.y; f < frames; f += gridDim.y) {
        int* L = labels + (size_t)f * h * w;
        if (__atomic_load_n(L + p, __ATOMIC_RELAXED) >= 0 && __atomic_load_n(L + other, __ATOMIC_RELAXED) >= 0) label_union(L, p, other);
    }
}

// every pixel takes its root.  A pixel another thread has flattened already holds a root, which is as good a link
__global__ __launch_bounds__(256) void k_label_flatten(size_t plane, int frames, int* __restrict__ labels)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= plane) return;
    for (int f = blockIdx.y; f < frames; f += gridDim.y) {
        int* L = labels + (size_t)f * plane;
        if (__atomic_load_n(L + p, __ATOMIC_RELAXED) < 0) continue;
        const int rt = label_find(L, (int)p);
        __atomic_store_n(L + p, rt, __ATOMIC_RELAXED);
    }
}

// ---- stage 3 ------------------------------------------------------------------------------------------------------
// stats: one int4 per pixel, used at roots: least x, greatest x, greatest y, pixels (the least y is the root's own row).
// The first pixel of every horizontal run reports its run.
__global__ __launch_bounds__(256) void k_marker_stats_init(size_t n, const int* __restrict__ labels, int w, int4* __restrict__ stats)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    stats[p] = make_int4(INT_MAX, -1, -1, 0);
}
__global__ __launch_bounds__(256) void k_marker_stats(const int* __restrict__ labels, int w, int h, int frames, int4* __restrict__ stats)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    for (int f = blockIdx.z; f < frames; f += gridDim.z) {
        const int* row = labels + ((size_t)f * h + y) * w;
        const int rt = row[x];
        if (rt < 0 || (x > 0 && row[x - 1] >= 0)) continue;
        int e = x;
        while (e + 1 < w && row[e + 1] >= 0) e++;  // (4-connected: the run is of one component)
        int* s = (int*)(stats + (size_t)f * h * w + rt);
        atomicMin(s + 0, x), atomicMax(s + 1, e), atomicMax(s + 2, y), atomicAdd(s + 3, e - x + 1);
    }
}

// the predicate and the sink of the shared compaction: row = frame * h + y
struct MarkerCandidate {
    const int* labels;
    const int4* stats;
    int w, h, min_side, max_side;
    int* cand;
    const unsigned long long* rowoff;
    __device__ __forceinline__ bool on(int x, int row) const
    {
        const int f = row / h, y = row - f * h;
        const size_t p = (size_t)row * w + x;
        if (labels[p] != y * w + x) return false;  // a root
        const int4 s = stats[p];
        const int bw = s.y - s.x + 1, bh = s.z - y + 1;
        return bw >= min_side && bw <= max_side && bh >= min_side && bh <= max_side && s.x > 0 && y > 0 && s.y < w - 1 && s.z < h - 1;
    }
    __device__ __forceinline__ void emit(int x, int row, unsigned long long pos) const
    {
        const int f = row / h, y = row - f * h;
        const unsigned long long k = pos - rowoff[(size_t)f * h];
        if (k < (unsigned long long)CAMD_MARKER_CAPACITY) {
            const int4 s = stats[(size_t)row * w + x];
            int* o = cand + ((size_t)f * CAMD_MARKER_CAPACITY + k) * 6;
            o[0] = y * w + x, o[1] = s.x, o[2] = y, o[3] = s.y, o[4] = s.z, o[5] = s.w;
        }
    }
};

__global__ __launch_bounds__(256) void k_marker_counts(const unsigned long long* __restrict__ rowoff,
                                                      const unsigned long long* __restrict__ total, int h, int frames,
                                                      int* __restrict__ counts, int* __restrict__ status)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    const unsigned long long end = f + 1 < frames ? rowoff[(size_t)(f + 1) * h] : *total;
    const int c = (int)(end - rowoff[(size_t)f * h]);
    counts[f] = c, status[f] = c > CAMD_MARKER_CAPACITY ? MARKER_OVERFLOW : 0;
}

struct MarkerWorkspace {  // the total (padded to 64 bytes), the compaction's rows, then the stats (16-aligned)
    unsigned long long* total;
    RowWorkspace rows;
    int4* stats;
    static size_t head(int nrows) { return (64 + RowWorkspace::bytes(nrows) + 15) / 16 * 16; }
    MarkerWorkspace(void* ws, int nrows) : total((unsigned long long*)ws), rows((char*)ws + 64, nrows), stats((int4*)((char*)ws + head(nrows))) {}
    static size_t bytes(int nrows, int w) { return head(nrows) + (size_t)nrows * w * sizeof(int4); }
};

// ---- stages 4 and 5 -----------------------------------------------------------------------------------------------
// lane 0's value in every lane
__device__ __forceinline__ unsigned long long wave_first(unsigned long long v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (unsigned long long)hi << 32 | lo;
}
constexpr unsigned long long PIX_MASK = (1ull << 28) - 1;  // a pixel's y * w + x
constexpr long long CROSS_BIAS = 1ll << 22;                // |cross| <= 2 * 1023^2 < 2^22 inside a box of 1024

__global__ __launch_bounds__(256) void k_marker_quad(const uint8_t* __restrict__ gray, int w, int h, size_t pitch, size_t stride,
                                                    int frames, const int* __restrict__ labels, const int* __restrict__ cand,
                                                    const int* __restrict__ counts, int min_side,
                                                    const unsigned long long* __restrict__ words, int n_ids, int s, int max_errors,
                                                    int* __restrict__ quads, int* __restrict__ id_turn, unsigned* __restrict__ best)
{
    const int lane = threadIdx.x & 63, slot = blockIdx.x * 4 + (threadIdx.x >> 6), f = blockIdx.y;
    const int count = counts[f];
    if (slot >= CAMD_MARKER_CAPACITY) return;  // (the whole wave; there is no barrier to miss)
    int* q_out = quads + ((size_t)f * CAMD_MARKER_CAPACITY + slot) * 8;
    int* it_out = id_turn + (size_t)f * CAMD_MARKER_CAPACITY + slot;
    if (count > CAMD_MARKER_CAPACITY || slot >= count) {  // an overflowing frame has no markers
        if (lane < 8) q_out[lane] = -1;
        if (lane == 0) *it_out = -1;
        return;
    }
    const int* c = cand + ((size_t)f * CAMD_MARKER_CAPACITY + slot) * 6;
    const int root = c[0], bx0 = c[1], by0 = c[2], bx1 = c[3], by1 = c[4];
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1, n = bw * bh;
    const int* L = labels + (size_t)f * h * w;
    // a: the outline's pixel farthest from the box's centre, in doubled coordinates; ties to the least pixel index
    unsigned long long ka = 0;
    for (int k = lane; k < n; k += 64) {
        const int y = by0 + k / bw, x = bx0 + k % bw, p = y * w + x;
        if (L[p] != root) continue;
        const long long dx = 2 * x - (bx0 + bx1), dy = 2 * y - (by0 + by1);
        const unsigned long long key = (unsigned long long)(dx * dx + dy * dy) << 28 | (PIX_MASK - (unsigned)p);
        ka = key > ka ? key : ka;
    }
    ka = wave_first(wave_max(ka));
    const int pa = (int)(PIX_MASK - (ka & PIX_MASK)), ay = pa / w, ax = pa - ay * w;
    // b: farthest from a
    unsigned long long kb = 0;
    for (int k = lane; k < n; k += 64) {
        const int y = by0 + k / bw, x = bx0 + k % bw, p = y * w + x;
        if (L[p] != root) continue;
        const long long dx = x - ax, dy = y - ay;
        const unsigned long long key = (unsigned long long)(dx * dx + dy * dy) << 28 | (PIX_MASK - (unsigned)p);
        kb = key > kb ? key : kb;
    }
    kb = wave_first(wave_max(kb));
    const int pb = (int)(PIX_MASK - (kb & PIX_MASK)), by = pb / w, bx = pb - by * w;
    // c, d: the greatest and the least cross(b - a, p - a)
    const long long ux = bx - ax, uy = by - ay;
    unsigned long long kc = 0, kd = ~0ull;
    for (int k = lane; k < n; k += 64) {
        const int y = by0 + k / bw, x = bx0 + k % bw, p = y * w + x;
        if (L[p] != root) continue;
        const unsigned long long cr = (unsigned long long)(ux * (y - ay) - uy * (x - ax) + CROSS_BIAS);
        const unsigned long long hi = cr << 28 | (PIX_MASK - (unsigned)p), lo = cr << 28 | (unsigned)p;
        kc = hi > kc ? hi : kc, kd = lo < kd ? lo : kd;
    }
    kc = wave_first(wave_max(kc)), kd = wave_first(wave_min(kd));
    const int pc = (int)(PIX_MASK - (kc & PIX_MASK)), pd = (int)(kd & PIX_MASK);
    const long long cross_c = (long long)(kc >> 28) - CROSS_BIAS, cross_d = (long long)(kd >> 28) - CROSS_BIAS;
    // clockwise in image coordinates (x right, y down): a, d, b, c
    const int qx[4] = {ax, pd % w, bx, pc % w}, qy[4] = {ay, pd / w, by, pc / w};
    bool ok = cross_c > 0 && cross_d < 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long long ex = qx[(k + 1) & 3] - qx[k], ey = qy[(k + 1) & 3] - qy[k];
        const long long fx = qx[(k + 2) & 3] - qx[(k + 1) & 3], fy = qy[(k + 2) & 3] - qy[(k + 1) & 3];
        ok = ok && ex * fy - ey * fx > 0 && ex * ex + ey * ey >= (long long)min_side * min_side;
    }
    int got = -1;
    if (uniform(ok)) {
        const MarkerImage image = {gray + (size_t)f * stride, w, h, pitch};
        const unsigned long long key = decode_marker(image, s, 1, 1, words, n_ids, max_errors, lane, qx[0], qy[0], qx[1], qy[1],
                                                     qx[3], qy[3], qx[2], qy[2]);
        if (key != CHESS_NONE) {
            got = (int)(key & 0xffff);
            // 6: of a frame's candidates that decode to one id the least (errors, candidate) stands
            if (lane == 0) atomicMin(best + (size_t)f * n_ids + (got >> 2), (unsigned)(key >> 16) << 10 | (unsigned)slot);
        }
    }
    if (lane < 4) q_out[2 * lane] = ok ? qx[lane] : -1, q_out[2 * lane + 1] = ok ? qy[lane] : -1;
    if (lane == 0) *it_out = got;
}

// ---- stage 6 ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_marker_by_id(const unsigned* __restrict__ best, const int* __restrict__ quads,
                                                     const int* __restrict__ id_turn, int frames, int n_ids,
                                                     uint8_t* __restrict__ seen, float* __restrict__ corners)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (size_t)frames * n_ids) return;
    const unsigned key = best[k];
    float* o = corners + k * 8;
    seen[k] = key != ~0u;
    if (key == ~0u) {
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = NAN;
        return;
    }
    const size_t slot = k / n_ids * CAMD_MARKER_CAPACITY + (key & 1023);
    const int turn = id_turn[slot] & 3;
    const int* q = quads + slot * 8;
#pragma unroll
    for (int j = 0; j < 4; j++) {  // the marker's own top-left, top-right, bottom-right, bottom-left
        const int from = (j + turn) & 3;
        o[2 * j] = (float)q[2 * from], o[2 * j + 1] = (float)q[2 * from + 1];
    }
}

static bool marker_image_limits(const char* who, int w, int h, int frames)
{
    if (w > MARKER_MAX_SIDE || h > MARKER_MAX_SIDE) {
        set_error("%s: an image of %d x %d; the detector takes sides up to %d", who, w, h, MARKER_MAX_SIDE);
        return false;
    }
    return true;
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_dark_mask(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, int block_radius, int offset,
                   uint8_t* mask, void* queue)
{
    if (block_radius < 1 || block_radius > MARKER_MAX_RADIUS || offset < -255 || offset > 255) {
        set_error("camd_dark_mask: block_radius %d, offset %d: the mask takes block_radius 1 .. %d and offset -255 .. 255", block_radius,
                  offset, MARKER_MAX_RADIUS);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (!marker_image_limits("camd_dark_mask", w, h, frames)) return CAMD_ERR_UNSUPPORTED;
    if (!gray || !mask || w < 1 || h < 1 || frames < 1 || pitch < (size_t)w || (frames > 1 && stride < (size_t)(h - 1) * pitch + (size_t)w) ||
        (long long)frames * h >= (1LL << 31)) {
        set_error("camd_dark_mask: bad arguments (gray, mask: device arrays; w, h, frames > 0 with frames * h < 2^31; pitch >= w, "
                  "stride >= an image)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const dim3 grid(div_up(w, MASK_TW), div_up(h, MASK_TH), frames < 65535 ? frames : 65535);
    hipLaunchKernelGGL(k_dark_mask, grid, dim3(256), 0, (hipStream_t)queue, gray, w, h, pitch, stride, frames, block_radius, offset, mask);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_label_components(const uint8_t* mask, int w, int h, int frames, int* labels, void* queue)
{
    if (!marker_image_limits("camd_label_components", w, h, frames)) return CAMD_ERR_UNSUPPORTED;
    if (!mask || !labels || w < 1 || h < 1 || frames < 1 || (long long)frames * h >= (1LL << 31) || (uintptr_t)labels % 4 != 0) {
        set_error("camd_label_components: bad arguments (mask, labels: device arrays, aligned to an element; w, h, frames > 0 with "
                  "frames * h < 2^31)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    const int fz = frames < 65535 ? frames : 65535;
    hipLaunchKernelGGL(k_label_tile, dim3(div_up(w, LABEL_TW), div_up(h, LABEL_TH), fz), dim3(256), 0, st, mask, w, h, frames, labels);
    const long long borders = (long long)((w - 1) / LABEL_TW) * h + (long long)((h - 1) / LABEL_TH) * w;
    if (borders > 0)
        hipLaunchKernelGGL(k_label_merge, dim3(div_up(borders, 256), fz), dim3(256), 0, st, w, h, frames, labels);
    hipLaunchKernelGGL(k_label_flatten, dim3(div_up((long long)w * h, 256), fz), dim3(256), 0, st, (size_t)w * h, frames, labels);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

static bool marker_sides_ok(const char* who, int min_side, int max_side)
{
    if (min_side < 4 || min_side > max_side || max_side > MARKER_MAX_BOX) {
        set_error("%s: min_side %d, max_side %d: the detector takes 4 <= min_side <= max_side <= %d", who, min_side, max_side,
                  MARKER_MAX_BOX);
        return false;
    }
    return true;
}

size_t camd_marker_candidates_workspace_bytes(int w, int h, int frames)
{
    if (w < 1 || h < 1 || frames < 1 || (long long)frames * h >= (1LL << 31)) return 0;
    return MarkerWorkspace::bytes(frames * h, w);
}

int camd_marker_candidates(const int* labels, int w, int h, int frames, int min_side, int max_side, void* workspace,
                           int* candidates, int* counts, int* status, void* queue)
{
    if (!marker_sides_ok("camd_marker_candidates", min_side, max_side) || !marker_image_limits("camd_marker_candidates", w, h, frames))
        return CAMD_ERR_UNSUPPORTED;
    if (!labels || !workspace || !candidates || !counts || !status || w < 1 || h < 1 || frames < 1 ||
        (long long)frames * h >= (1LL << 31) || (uintptr_t)labels % 4 != 0 || (uintptr_t)workspace % 16 != 0 ||
        (uintptr_t)candidates % 4 != 0 || (uintptr_t)counts % 4 != 0 || (uintptr_t)status % 4 != 0) {
        set_error("camd_marker_candidates: bad arguments (labels, workspace, candidates, counts, status: device arrays, aligned to an "
                  "element, the workspace to 16 bytes; w, h, frames > 0 with frames * h < 2^31)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    const int rows = frames * h, fz = frames < 65535 ? frames : 65535;
    const MarkerWorkspace ws(workspace, rows);
    const size_t n = (size_t)rows * w;
    hipLaunchKernelGGL(k_marker_stats_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, labels, w, ws.stats);
    hipLaunchKernelGGL(k_marker_stats, dim3(div_up(w, 256), h, fz), dim3(256), 0, st, labels, w, h, frames, ws.stats);
    const MarkerCandidate f = {labels, ws.stats, w, h, min_side, max_side, candidates, ws.rows.rowoff};
    row_count(f, w, rows, ws.rows.rowcount, st);
    row_scan(ws.rows.rowcount, rows, ws.rows.rowoff, ws.total, st);
    row_emit(f, w, rows, ws.rows.rowoff, ~(size_t)0, nullptr, st);  // (the capacity is per frame: MarkerCandidate::emit holds it)
    hipLaunchKernelGGL(k_marker_counts, dim3(div_up(frames, 256)), dim3(256), 0, st, ws.rows.rowoff, ws.total, h, frames, counts, status);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_marker_decode(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, const int* labels,
                       const int* candidates, const int* counts, int min_side, const unsigned long long* dictionary_words,
                       int n_ids, int s, int max_bit_errors, int* quads, int* id_turn, unsigned* best, uint8_t* seen,
                       float* corners, void* queue)
{
    if (s < 4 || s > MARKER_MAX_BITS || n_ids < 1 || n_ids > CAMD_CHARUCO_MAX_IDS || max_bit_errors < 0 || max_bit_errors > s * s ||
        !marker_sides_ok("camd_marker_decode", min_side, MARKER_MAX_BOX)) {
        set_error("camd_marker_decode: markers of %d x %d bits, %d ids, max_bit_errors %d, min_side %d: the detector takes 4 .. %d "
                  "bits, up to %d ids, max_bit_errors 0 .. s*s, min_side 4 .. %d", s, s, n_ids, max_bit_errors, min_side,
                  MARKER_MAX_BITS, CAMD_CHARUCO_MAX_IDS, MARKER_MAX_BOX);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (!marker_image_limits("camd_marker_decode", w, h, frames)) return CAMD_ERR_UNSUPPORTED;
    if (!gray || !labels || !candidates || !counts || !dictionary_words || !quads || !id_turn || !best || !seen || !corners || w < 3 ||
        h < 3 || frames < 1 || frames > 65535 || pitch < (size_t)w || (frames > 1 && stride < (size_t)(h - 1) * pitch + (size_t)w) ||
        (uintptr_t)labels % 4 != 0 || (uintptr_t)candidates % 4 != 0 || (uintptr_t)counts % 4 != 0 ||
        (uintptr_t)dictionary_words % 8 != 0 || (uintptr_t)quads % 4 != 0 || (uintptr_t)id_turn % 4 != 0 || (uintptr_t)best % 4 != 0 ||
        (uintptr_t)corners % 4 != 0) {
        set_error("camd_marker_decode: bad arguments (gray, labels, candidates, counts, dictionary_words, quads, id_turn, best, seen, "
                  "corners: device arrays, aligned to an element; w, h >= 3, 0 < frames <= 65535; pitch >= w, stride >= an image)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    CAMD_HIP(hipMemsetAsync(best, 0xff, (size_t)frames * n_ids * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_marker_quad, dim3(CAMD_MARKER_CAPACITY / 4, frames), dim3(256), 0, st, gray, w, h, pitch, stride, frames, labels,
                       candidates, counts, min_side, dictionary_words, n_ids, s, max_bit_errors, quads, id_turn, best);
    hipLaunchKernelGGL(k_marker_by_id, dim3(div_up((long long)frames * n_ids, 256)), dim3(256), 0, st, best, quads, id_turn, frames, n_ids,
                       seen, corners);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
