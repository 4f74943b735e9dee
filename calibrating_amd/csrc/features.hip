// features.hip -- keypoints, binary descriptors and a brute-force Hamming matcher: matches from two pictures alone.
//
// A contract of this library's OWN (not cv2.ORB / cv2.BFMatcher: UNPINNED),
// integers end to end, every tie defined, restated in NumPy by tests/features_ref.py.  include/calibrating_amd.h states the
// order of every operation.
//   A  k_feat_score      the FAST-9 corner score of every pixel, uint8: a tile of 64 x 16 pixels and its 3 px halo in LDS
//      k_feat_cells      one wavefront per cell x cell block: the 3 x 3 peak of the largest key, reduced inside the wave --
//                        no global atomics; then the shared ordered compaction (compact.hpp) lists the blocks' winners
//   B  k_feat_describe   one wavefront per keypoint, four per workgroup, NO workgroup barrier (as subpix.hip): the 33 x 33
//                        patch and its 29 x 29 box sums live in the wave's own slice of LDS; the moments meet in a butterfly,
//                        lane l evaluates tests 64 j + l and one ballot per j is a finished 64-bit word of the descriptor
//   C  k_feat_search     256 queries per workgroup, one per lane, in 8 registers; the train rows stream through LDS in tiles
//                        of 256 (8 KB), every lane reads the same address (a broadcast): 8 xor + 8 popcount per pair
//      camd_feature_filter   distance limit, ratio test, cross-check, then the same ordered compaction
#include <climits>

#include "compact.hpp"
#include "pnp_common.hpp"  // wave_lds_fence, uniform

namespace camd {

constexpr int FEAT_BORDER = CAMD_FEATURE_BORDER;
constexpr int FEAT_MAX_SIDE = 16384;          // y * w + x stays below 2^28: the key's low word, int32 pixel indices
constexpr int FEAT_TW = 64, FEAT_TH = 16;     // stage A's tile: 64 threads across, 4 x 4 rows down
constexpr int FEAT_HALO = 3;                  // the ring's radius
constexpr int FEAT_LW = 72;                   // bytes of a staged row (64 + 2 * 3, padded)
constexpr int FEAT_LH = FEAT_TH + 2 * FEAT_HALO;
constexpr int FEAT_PATCH = 2 * FEAT_BORDER + 1;  // 33
constexpr int FEAT_BOX = FEAT_PATCH - 4;         // 29: box centres up to 14 from the keypoint
constexpr int FEAT_REACH = 14;
constexpr int FEAT_DISC = 13;
constexpr int FEAT_SLICE = 2784;              // a wave's LDS: 1089 patch bytes (padded to 1092), 841 uint16 box sums
static_assert(1092 + 2 * FEAT_BOX * FEAT_BOX <= FEAT_SLICE && FEAT_SLICE % 16 == 0, "slice layout");
constexpr int FEAT_MAX_RATIO = 1 << 20;       // d * den and num * 257 stay in int32

// rint(16384 cos(2 pi k / 32)); the sine is the cosine a quarter turn back
__constant__ int FEAT_COS[32] = {16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196, -6270, -9102, -11585, -13623,
                                 -15137, -16069, -16384, -16069, -15137, -13623, -11585, -9102, -6270, -3196, 0, 3196, 6270,
                                 9102, 11585, 13623, 15137, 16069};

// ---- stage A: the score plane ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_feat_score(const uint8_t* __restrict__ gray, int w, int h, size_t pitch, size_t stride,
                                                   int frames, int threshold, uint8_t* __restrict__ out)
{
    __shared__ uint8_t tile[FEAT_LH * FEAT_LW];
    const int x0 = (int)blockIdx.x * FEAT_TW, y0 = (int)blockIdx.y * FEAT_TH;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int f = blockIdx.z; f < frames; f += gridDim.z) {
        const uint8_t* img = gray + (size_t)f * stride;
        for (int k = threadIdx.x; k < FEAT_LH * FEAT_LW; k += 256) {
            const int row = k / FEAT_LW, col = k - row * FEAT_LW;
            const int y = y0 - FEAT_HALO + row, x = x0 - FEAT_HALO + col;
            // (outside the image: such a sample only reaches pixels whose score is 0 anyway)
            tile[k] = (y >= 0 && y < h && x >= 0 && x < w) ? img[(size_t)y * pitch + x] : (uint8_t)0;
        }
        __syncthreads();
        const int x = x0 + tx;
#pragma unroll
        for (int k = 0; k < FEAT_TH / 4; k++) {
            const int ly = ty + 4 * k, y = y0 + ly;
            if (y >= h || x >= w) continue;
            int score = 0;
            if (x >= FEAT_BORDER && x < w - FEAT_BORDER && y >= FEAT_BORDER && y < h - FEAT_BORDER) {
                const uint8_t* c = tile + (ly + FEAT_HALO) * FEAT_LW + tx + FEAT_HALO;
                const int v = c[0];
#define R(dx, dy) ((int)c[(dy) * FEAT_LW + (dx)] - v)
                const int d[16] = {R(0, -3), R(1, -3), R(2, -2), R(3, -1), R(3, 0),  R(3, 1),   R(2, 2),   R(1, 3),
                                   R(0, 3),  R(-1, 3), R(-2, 2), R(-3, 1), R(-3, 0), R(-3, -1), R(-2, -2), R(-1, -3)};
#undef R
                int best = 0;
#pragma unroll
                for (int s = 0; s < 16; s++) {
                    int lo = d[s], hi = d[s];
#pragma unroll
                    for (int j = 1; j < 9; j++) {
                        const int e = d[(s + j) & 15];
                        lo = e < lo ? e : lo;
                        hi = e > hi ? e : hi;
                    }
                    best = lo > best ? lo : best;    // the arc is brighter by at least lo
                    best = -hi > best ? -hi : best;  // ... darker by at least -hi
                }
                score = best >= threshold ? best : 0;
            }
            out[((size_t)f * h + y) * w + x] = (uint8_t)score;
        }
        __syncthreads();  // (the next frame's tile)
    }
}

// ---- stage A: the block winners ----------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long feat_key(int score, int index)
{
    return (unsigned long long)score << 32 | (unsigned long long)(0xFFFFFFFFu - (uint32_t)index);
}

// cellkey[(f * cells_h + cy) * cells_w + cx]: the largest key among the peaks of the block, 0 where it has none
__global__ __launch_bounds__(256) void k_feat_cells(const uint8_t* __restrict__ score, int w, int h, int cell, int cells_w,
                                                   int cells_h, unsigned long long ncells,
                                                   unsigned long long* __restrict__ cellkey)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long c = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= ncells) return;  // (the whole wave; there is no barrier to miss)
    const unsigned long long per = (unsigned long long)cells_w * cells_h;
    const unsigned long long f = c / per;
    const int r = (int)(c - f * per), cy = r / cells_w, cx = r - cy * cells_w;
    const uint8_t* plane = score + (size_t)f * h * w;
    unsigned long long best = 0;
    for (int p = lane; p < cell * cell; p += 64) {
        const int py = cy * cell + p / cell, px = cx * cell + p % cell;
        // (a score lies FEAT_BORDER inside the image; a plane that says otherwise is not believed, so the neighbours exist)
        if (px < FEAT_BORDER || px >= w - FEAT_BORDER || py < FEAT_BORDER || py >= h - FEAT_BORDER) continue;
        const int s = plane[(size_t)py * w + px];
        if (!s) continue;
        const unsigned long long key = feat_key(s, py * w + px);
        bool peak = true;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++)
                if (dx || dy) peak = peak && feat_key(plane[(size_t)(py + dy) * w + px + dx], (py + dy) * w + px + dx) < key;
        if (peak && key > best) best = key;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned long long o = __shfl_xor(best, m, 64);
        best = o > best ? o : best;
    }
    if (lane == 0) cellkey[c] = best;
}

// the predicate and the sink of the shared compaction over the blocks: row = frame * cells_h + cy, element = cx
struct FeatCell {
    const unsigned long long* cellkey;
    int w, cells_w, cells_h, capacity;
    int* xy;
    int* scores;
    const unsigned long long* rowoff;
    __device__ __forceinline__ bool on(int x, int row) const { return cellkey[(size_t)row * cells_w + x] != 0; }
    __device__ __forceinline__ void emit(int x, int row, unsigned long long pos) const
    {
        const int f = row / cells_h;
        const unsigned long long k = pos - rowoff[(size_t)f * cells_h];
        if (k >= (unsigned long long)capacity) return;  // (cannot happen: a block has one winner)
        const unsigned long long key = cellkey[(size_t)row * cells_w + x];
        const uint32_t index = 0xFFFFFFFFu - (uint32_t)key;
        int* o = xy + ((size_t)f * capacity + k) * 2;
        o[0] = (int)(index % (uint32_t)w), o[1] = (int)(index / (uint32_t)w);
        scores[(size_t)f * capacity + k] = (int)(key >> 32);
    }
};

// counts[g] = the passing elements of rows g * per .. (g + 1) * per - 1
__global__ __launch_bounds__(256) void k_feat_counts(const unsigned long long* __restrict__ rowoff,
                                                    const unsigned long long* __restrict__ total, int per, int groups,
                                                    int* __restrict__ counts)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const unsigned long long end = g + 1 < groups ? rowoff[(size_t)(g + 1) * per] : *total;
    counts[g] = (int)(end - rowoff[(size_t)g * per]);
}

// a compaction's workspace behind `head` bytes of the caller's own: the total (padded to 64 bytes), then the rows
struct FeatWorkspace {
    unsigned long long* total;
    RowWorkspace rows;
    FeatWorkspace(void* ws, size_t head, int nrows)
        : total((unsigned long long*)((char*)ws + head)), rows((char*)ws + head + 64, nrows) {}
    static size_t bytes(size_t head, int nrows) { return head + 64 + RowWorkspace::bytes(nrows); }
};
static inline size_t feat_key_bytes(unsigned long long ncells) { return (size_t)((ncells * 8 + 63) / 64 * 64); }

// ---- stage B -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_feat_describe(const uint8_t* __restrict__ gray, int w, int h, size_t pitch,
                                                      size_t stride, int frames, const int* __restrict__ xy,
                                                      const int* __restrict__ counts, int capacity,
                                                      const int8_t* __restrict__ pattern, uint8_t* __restrict__ desc,
                                                      int* __restrict__ bins)
{
    __shared__ __attribute__((aligned(16))) uint8_t slices[4 * FEAT_SLICE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long slot = (unsigned long long)blockIdx.x * 4 + wave;
    if (slot >= (unsigned long long)frames * capacity) return;  // (the whole wave; there is no barrier to miss)
    const int f = (int)(slot / (unsigned long long)capacity), k = (int)(slot - (unsigned long long)f * capacity);
    if (k >= counts[f]) return;  // (beyond the frame's keypoints: the caller's fill stays)
    const int x = xy[slot * 2], y = xy[slot * 2 + 1];
    unsigned long long* out = (unsigned long long*)(desc + slot * 32);
    // a point nearer a border than the patch reaches: nothing is read, the descriptor is zero and the bin -1
    if (!uniform(x >= FEAT_BORDER && x < w - FEAT_BORDER && y >= FEAT_BORDER && y < h - FEAT_BORDER)) {
        if (lane < 4) out[lane] = 0;
        if (lane == 0) bins[slot] = -1;
        return;
    }
    uint8_t* patch = slices + wave * FEAT_SLICE;
    uint16_t* box = (uint16_t*)(patch + 1092);
    const uint8_t* img = gray + (size_t)f * stride + (size_t)(y - FEAT_BORDER) * pitch + (x - FEAT_BORDER);
    for (int p = lane; p < FEAT_PATCH * FEAT_PATCH; p += 64) {
        const int i = p / FEAT_PATCH, j = p - i * FEAT_PATCH;
        patch[p] = img[(size_t)i * pitch + j];
    }
    wave_lds_fence();
    // the intensity centroid over the disc: integers, so the order of the sum does not show
    int m10 = 0, m01 = 0;
    for (int p = lane; p < (2 * FEAT_DISC + 1) * (2 * FEAT_DISC + 1); p += 64) {
        const int dy = p / (2 * FEAT_DISC + 1) - FEAT_DISC, dx = p % (2 * FEAT_DISC + 1) - FEAT_DISC;
        if (dx * dx + dy * dy <= FEAT_DISC * FEAT_DISC) {
            const int I = patch[(FEAT_BORDER + dy) * FEAT_PATCH + FEAT_BORDER + dx];
            m10 += dx * I, m01 += dy * I;
        }
    }
    for (int p = lane; p < FEAT_BOX * FEAT_BOX; p += 64) {
        const int by = p / FEAT_BOX, bx = p - by * FEAT_BOX;
        int s = 0;
#pragma unroll
        for (int i = 0; i < 5; i++)
#pragma unroll
            for (int j = 0; j < 5; j++) s += patch[(by + i) * FEAT_PATCH + bx + j];
        box[p] = (uint16_t)s;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) m10 += __shfl_xor(m10, m, 64), m01 += __shfl_xor(m01, m, 64);
    // the bin: lane k < 32 proposes itself, the largest (value, -k) wins
    long long v = lane < 32 ? (long long)m10 * FEAT_COS[lane & 31] + (long long)m01 * FEAT_COS[(lane + 24) & 31] : LLONG_MIN;
    int bin = lane;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const long long ov = __shfl_xor(v, m, 64);
        const int ob = __shfl_xor(bin, m, 64);
        if (ov > v || (ov == v && ob < bin)) v = ov, bin = ob;
    }
    bin = __builtin_amdgcn_readfirstlane(bin) & 31;
    wave_lds_fence();
    const int* tests = (const int*)pattern + bin * 256;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int t = tests[64 * j + lane];
        int c[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e = (int)(int8_t)(t >> (8 * q));
            c[q] = (e < -FEAT_REACH ? -FEAT_REACH : e > FEAT_REACH ? FEAT_REACH : e) + FEAT_REACH;  // (a table out of range reads no other memory)
        }
        const unsigned long long word = __ballot(box[c[1] * FEAT_BOX + c[0]] < box[c[3] * FEAT_BOX + c[2]]);
        if (lane == 0) out[j] = word;
    }
    if (lane == 0) bins[slot] = bin;
}

// ---- stage C: the search -----------------------------------------------------------------------------------------------
struct FeatSets {
    const uint8_t* desc[2];
    const int* counts[2];
    int frames[2], capacity[2];
    const int* pairs;
    int* best[2];
    int* dist[2];
};
__device__ __forceinline__ int feat_rows(const int* counts, int frames, int capacity, int f)
{
    if (f < 0 || f >= frames) return 0;  // (a pair outside the frames matches nothing)
    const int n = counts[f];
    return n < 0 ? 0 : n > capacity ? capacity : n;
}

__global__ __launch_bounds__(256) void k_feat_search(FeatSets a)
{
    __shared__ uint4 tile[256 * 2];
    const int dir = blockIdx.z, p = blockIdx.y, qs = dir, ts = 1 - dir;
    if ((int)blockIdx.x * 256 >= a.capacity[qs]) return;  // (the whole workgroup)
    const int fq = a.pairs[2 * p + qs], ft = a.pairs[2 * p + ts];
    const int nq = feat_rows(a.counts[qs], a.frames[qs], a.capacity[qs], fq);
    const int nt = feat_rows(a.counts[ts], a.frames[ts], a.capacity[ts], ft);
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    if (q < nq) {
        const uint4* src = (const uint4*)(a.desc[qs] + ((size_t)fq * a.capacity[qs] + q) * 32);
        q0 = src[0], q1 = src[1];
    }
    int best = -1, dbest = 257, dsecond = 257;
    for (int t0 = 0; t0 < nt; t0 += 256) {
        __syncthreads();  // (the tile of the round before is read out)
        const int t = t0 + (int)threadIdx.x;
        if (t < nt) {
            const uint4* src = (const uint4*)(a.desc[ts] + ((size_t)ft * a.capacity[ts] + t) * 32);
            tile[2 * threadIdx.x] = src[0], tile[2 * threadIdx.x + 1] = src[1];
        }
        __syncthreads();
        const int n = nt - t0 < 256 ? nt - t0 : 256;
        for (int j = 0; j < n; j++) {
            const uint4 u = tile[2 * j], v = tile[2 * j + 1];  // every lane reads the same address: a broadcast
            const int d = ((__popc(u.x ^ q0.x) + __popc(u.y ^ q0.y)) + (__popc(u.z ^ q0.z) + __popc(u.w ^ q0.w))) +
                          ((__popc(v.x ^ q1.x) + __popc(v.y ^ q1.y)) + (__popc(v.z ^ q1.z) + __popc(v.w ^ q1.w)));
            // rising train index: a strict < keeps the lowest index among equals
            if (d < dbest) dsecond = dbest, dbest = d, best = t0 + j;
            else if (d < dsecond) dsecond = d;
        }
    }
    if (q < a.capacity[qs]) {
        const size_t o = (size_t)p * a.capacity[qs] + q;
        const bool live = q < nq;
        a.best[dir][o] = live ? best : -1;
        a.dist[dir][2 * o] = live ? dbest : 257;
        a.dist[dir][2 * o + 1] = live ? dsecond : 257;
    }
}

// ---- stage C: the filter -----------------------------------------------------------------------------------------------
// the predicate and the sink of the shared compaction over the queries: row = pair, element = query
struct FeatMatch {
    const int* counts1;
    const int* pairs;
    const int* best12;
    const int* dist12;
    const int* best21;
    int frames1, capacity1, capacity2, max_distance, num, den, cross;
    int* matches;
    int* distances;
    const unsigned long long* rowoff;
    __device__ __forceinline__ bool on(int q, int p) const
    {
        if (q >= feat_rows(counts1, frames1, capacity1, pairs[2 * p])) return false;
        const size_t o = (size_t)p * capacity1 + q;
        const int b = best12[o], d = dist12[2 * o], d2 = dist12[2 * o + 1];
        if (b < 0 || b >= capacity2 || d > max_distance || (long long)d * den > (long long)num * d2) return false;
        return !cross || best21[(size_t)p * capacity2 + b] == q;
    }
    __device__ __forceinline__ void emit(int q, int p, unsigned long long pos) const
    {
        const unsigned long long k = pos - rowoff[p];
        if (k >= (unsigned long long)capacity1) return;  // (cannot happen: a query gives one match)
        const size_t o = (size_t)p * capacity1 + q, m = (size_t)p * capacity1 + k;
        matches[2 * m] = q, matches[2 * m + 1] = best12[o];
        distances[m] = dist12[2 * o];
    }
};

// CAMD_OK, or the status of images the stages A and B cannot take
static int feat_image(const char* who, const void* gray, int w, int h, size_t pitch, size_t stride, int frames)
{
    if (!gray || w < 1 || h < 1 || frames < 1 || pitch < (size_t)w || (frames > 1 && stride < (size_t)(h - 1) * pitch + (size_t)w)) {
        set_error("%s: bad arguments (gray: a device array; w, h, frames > 0; pitch >= w, stride >= an image)", who);
        return CAMD_ERR_BAD_ARG;
    }
    if (w > FEAT_MAX_SIDE || h > FEAT_MAX_SIDE || (long long)frames * h >= (1LL << 31)) {
        set_error("%s: %d frames of %d x %d; the detector takes sides up to %d and frames * h < 2^31", who, frames, w, h, FEAT_MAX_SIDE);
        return CAMD_ERR_UNSUPPORTED;
    }
    return CAMD_OK;
}

// cells across, down; false outside the limits
static bool feat_cells(const char* who, int w, int h, int frames, int cell, int* cells_w, int* cells_h)
{
    if (w < 1 || h < 1 || frames < 1 || w > FEAT_MAX_SIDE || h > FEAT_MAX_SIDE || (long long)frames * h >= (1LL << 31) || cell < 4 ||
        cell > 64) {
        set_error("%s: %d frames of %d x %d, cell %d; the detector takes sides 1 .. %d, frames * h < 2^31 and cell 4 .. 64", who, frames,
                  w, h, cell, FEAT_MAX_SIDE);
        return false;
    }
    *cells_w = div_up(w, cell), *cells_h = div_up(h, cell);
    return true;
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_feature_score(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, int threshold, uint8_t* score,
                       void* queue)
{
    const int rc = feat_image("camd_feature_score", gray, w, h, pitch, stride, frames);
    if (rc != CAMD_OK) return rc;
    if (!score || threshold < 1 || threshold > 255) {
        set_error("camd_feature_score: bad arguments (score: a device array; threshold 1 .. 255, got %d)", threshold);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const dim3 grid(div_up(w, FEAT_TW), div_up(h, FEAT_TH), frames < 65535 ? frames : 65535);
    hipLaunchKernelGGL(k_feat_score, grid, dim3(256), 0, (hipStream_t)queue, gray, w, h, pitch, stride, frames, threshold, score);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

size_t camd_feature_keypoints_workspace_bytes(int w, int h, int frames, int cell)
{
    int cw, ch;
    if (!feat_cells("camd_feature_keypoints_workspace_bytes", w, h, frames, cell, &cw, &ch)) return 0;
    return FeatWorkspace::bytes(feat_key_bytes((unsigned long long)frames * cw * ch), frames * ch);
}

int camd_feature_keypoints(const uint8_t* score, int w, int h, int frames, int cell, void* workspace, int* xy, int* scores,
                           int* counts, void* queue)
{
    int cw, ch;
    if (!feat_cells("camd_feature_keypoints", w, h, frames, cell, &cw, &ch)) return CAMD_ERR_UNSUPPORTED;
    if (!score || !workspace || !xy || !scores || !counts || (uintptr_t)workspace % 8 != 0 || (uintptr_t)xy % 4 != 0 ||
        (uintptr_t)scores % 4 != 0 || (uintptr_t)counts % 4 != 0) {
        set_error("camd_feature_keypoints: bad arguments (score, workspace, xy, scores, counts: device arrays, aligned to an element, "
                  "the workspace to 8 bytes)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    const unsigned long long ncells = (unsigned long long)frames * cw * ch;
    const int rows = frames * ch;
    unsigned long long* cellkey = (unsigned long long*)workspace;
    const FeatWorkspace ws(workspace, feat_key_bytes(ncells), rows);
    hipLaunchKernelGGL(k_feat_cells, dim3((unsigned)((ncells + 3) / 4)), dim3(256), 0, st, score, w, h, cell, cw, ch, ncells, cellkey);
    const FeatCell f = {cellkey, w, cw, ch, cw * ch, xy, scores, ws.rows.rowoff};
    row_count(f, cw, rows, ws.rows.rowcount, st);
    row_scan(ws.rows.rowcount, rows, ws.rows.rowoff, ws.total, st);
    row_emit(f, cw, rows, ws.rows.rowoff, ~(size_t)0, nullptr, st);
    hipLaunchKernelGGL(k_feat_counts, dim3(div_up(frames, 256)), dim3(256), 0, st, ws.rows.rowoff, ws.total, ch, frames, counts);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_feature_describe(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, const int* xy, const int* counts,
                          int capacity, const int8_t* pattern, uint8_t* descriptors, int* bins, void* queue)
{
    const int rc = feat_image("camd_feature_describe", gray, w, h, pitch, stride, frames);
    if (rc != CAMD_OK) return rc;
    if (!xy || !counts || !pattern || !descriptors || !bins || capacity < 1 || (long long)frames * capacity >= (1LL << 31) ||
        (uintptr_t)xy % 4 != 0 || (uintptr_t)counts % 4 != 0 || (uintptr_t)pattern % 4 != 0 || (uintptr_t)descriptors % 8 != 0 ||
        (uintptr_t)bins % 4 != 0) {
        set_error("camd_feature_describe: bad arguments (xy, counts, pattern, descriptors, bins: device arrays, aligned to an element, "
                  "the pattern to 4 and the descriptors to 8 bytes; capacity > 0, frames * capacity < 2^31)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const unsigned long long slots = (unsigned long long)frames * capacity;
    hipLaunchKernelGGL(k_feat_describe, dim3((unsigned)((slots + 3) / 4)), dim3(256), 0, (hipStream_t)queue, gray, w, h, pitch, stride,
                       frames, xy, counts, capacity, pattern, descriptors, bins);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_feature_search(const uint8_t* desc1, const int* counts1, int frames1, int capacity1, const uint8_t* desc2, const int* counts2,
                        int frames2, int capacity2, const int* pairs, int npairs, int* best12, int* dist12, int* best21, int* dist21,
                        void* queue)
{
    if (!desc1 || !counts1 || !desc2 || !counts2 || !pairs || !best12 || !dist12 || !best21 || !dist21 || frames1 < 1 || frames2 < 1 ||
        capacity1 < 1 || capacity2 < 1 || npairs < 1 || npairs > 65535 || (long long)npairs * capacity1 >= (1LL << 30) ||
        (long long)npairs * capacity2 >= (1LL << 30) || (long long)frames1 * capacity1 >= (1LL << 31) ||
        (long long)frames2 * capacity2 >= (1LL << 31) || (uintptr_t)desc1 % 16 != 0 || (uintptr_t)desc2 % 16 != 0 ||
        ((uintptr_t)counts1 | (uintptr_t)counts2 | (uintptr_t)pairs | (uintptr_t)best12 | (uintptr_t)dist12 | (uintptr_t)best21 |
         (uintptr_t)dist21) % 4 != 0) {
        set_error("camd_feature_search: bad arguments (device arrays, the descriptors aligned to 16 bytes, the rest to an element; frames, "
                  "capacities > 0; 1 .. 65535 pairs, pairs * capacity < 2^30)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    FeatSets a = {{desc1, desc2}, {counts1, counts2}, {frames1, frames2}, {capacity1, capacity2}, pairs, {best12, best21}, {dist12, dist21}};
    const int cap = capacity1 > capacity2 ? capacity1 : capacity2;
    hipLaunchKernelGGL(k_feat_search, dim3(div_up(cap, 256), npairs, 2), dim3(256), 0, (hipStream_t)queue, a);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

size_t camd_feature_filter_workspace_bytes(int npairs)
{
    return npairs < 1 || npairs > 65535 ? 0 : FeatWorkspace::bytes(0, npairs);
}

int camd_feature_filter(const int* counts1, int frames1, int capacity1, int capacity2, const int* pairs, int npairs, const int* best12,
                        const int* dist12, const int* best21, int max_distance, int ratio_num, int ratio_den, int cross_check,
                        void* workspace, int* matches, int* distances, int* match_counts, void* queue)
{
    if (max_distance < 0 || max_distance > 256 || ratio_num < 1 || ratio_den < ratio_num || ratio_den > FEAT_MAX_RATIO) {
        set_error("camd_feature_filter: max_distance %d, ratio %d / %d; the filter takes max_distance 0 .. 256 and 1 <= num <= den <= %d",
                  max_distance, ratio_num, ratio_den, FEAT_MAX_RATIO);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (!counts1 || !pairs || !best12 || !dist12 || !best21 || !workspace || !matches || !distances || !match_counts || frames1 < 1 ||
        capacity1 < 1 || capacity2 < 1 || npairs < 1 || npairs > 65535 || (long long)npairs * capacity1 >= (1LL << 30) ||
        (long long)npairs * capacity2 >= (1LL << 30) || (uintptr_t)workspace % 8 != 0 ||
        ((uintptr_t)counts1 | (uintptr_t)pairs | (uintptr_t)best12 | (uintptr_t)dist12 | (uintptr_t)best21 | (uintptr_t)matches |
         (uintptr_t)distances | (uintptr_t)match_counts) % 4 != 0) {
        set_error("camd_feature_filter: bad arguments (device arrays, aligned to an element, the workspace to 8 bytes; frames, capacities "
                  "> 0; 1 .. 65535 pairs, pairs * capacity < 2^30)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    const FeatWorkspace ws(workspace, 0, npairs);
    const FeatMatch f = {counts1, pairs, best12, dist12, best21, frames1, capacity1, capacity2, max_distance, ratio_num, ratio_den,
                         cross_check != 0, matches, distances, ws.rows.rowoff};
    row_count(f, capacity1, npairs, ws.rows.rowcount, st);
    row_scan(ws.rows.rowcount, npairs, ws.rows.rowoff, ws.total, st);
    row_emit(f, capacity1, npairs, ws.rows.rowoff, ~(size_t)0, nullptr, st);
    hipLaunchKernelGGL(k_feat_counts, dim3(div_up(npairs, 256)), dim3(256), 0, st, ws.rows.rowoff, ws.total, 1, npairs, match_counts);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
