// chessboard.hip -- the inner corners of a chessboard found from the gray image alone, every frame of a recording at once.
//
// Stands where the reference calls cv2.findChessboardCorners (boards.py:160), but with a contract of its own
// (INTEGRATION.md section J): three stages of integer arithmetic, restated in NumPy by tests/chessboard_ref.py.
//   1  k_chess_response   the ChESS response (Bennett & Lasenby) times 5 of every pixel, int16, and its maximum per frame
//   2  camd_chess_peaks   the non-maximum-suppressed peaks of a frame, compacted in pixel order (compact.hpp)
//   3  k_chess_lattice    the peaks labelled as a lattice grown from the one nearest their centroid, put in board order
// Stage 1 is the hot path, 1 B read and 2 B written per pixel: a tile of 128 x 32 pixels and its 5 px halo go to LDS as
// dwords, and a thread computes four neighbouring pixels of a row from the up to five dwords of each of the 11 rows it
// needs (25 LDS dword reads for 84 samples), every sample picked out of a register by a constant shift.
// Stage 3 is one wavefront per frame with NO workgroup barrier, as in pnp.hip: candidates, queue and labels live in the
// wave's own slice of LDS, lane 0 writes it, a wavefront-scope fence orders that against the other lanes' reads, and what
// decides a branch is the same in every lane.  Every loop is bounded by a constant, the candidates or the board.
#include <climits>
#include <cmath>

#include "chess_wave.hpp"
#include "compact.hpp"

namespace camd {

constexpr int CHESS_BORDER = 5;                      // the ring's radius: nearer a border the response is 0
constexpr int CHESS_TW = 128, CHESS_TH = 32;         // a workgroup's tile: 32 threads x 4 pixels across, 8 x 4 rows down
constexpr int CHESS_LEFT = 8;                        // columns staged left of the tile: a thread's pixels stay dword-aligned
constexpr int CHESS_DWORDS = (CHESS_LEFT + CHESS_TW + 8) / 4;  // of a staged row: a wave half reads 32 consecutive ones
constexpr int CHESS_ROWS = CHESS_TH + 2 * CHESS_BORDER;
constexpr int CHESS_MAX_SIDE = 16384;                // of an image in stage 3: squared distances of pixels stay in int32
static_assert(CHESS_TW == 32 * 4 && CHESS_TH % 8 == 0 && CHESS_LEFT >= CHESS_BORDER && CHESS_LEFT % 4 == 0, "tile layout");

// ---- stage 1 ------------------------------------------------------------------------------------------------------
// IN4: image, pitch and stride are multiples of 4 bytes (the tile is staged as dwords); OUT8: the plane and w are
// multiples of 8 bytes / 4 pixels (a thread's four int16 leave as one 8-byte store)
template <bool IN4, bool OUT8>
__global__ __launch_bounds__(256) void k_chess_response(const uint8_t* __restrict__ gray, int w, int h, size_t pitch,
                                                       size_t stride, int frames, int16_t* __restrict__ out,
                                                       int* __restrict__ rmax)
{
    __shared__ uint32_t tile[CHESS_ROWS * CHESS_DWORDS];
    const int x0 = (int)blockIdx.x * CHESS_TW, y0 = (int)blockIdx.y * CHESS_TH;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int f = blockIdx.z; f < frames; f += gridDim.z) {
        const uint8_t* img = gray + (size_t)f * stride;
        for (int k = threadIdx.x; k < CHESS_ROWS * CHESS_DWORDS; k += 256) {
            const int row = k / CHESS_DWORDS, col = k - row * CHESS_DWORDS;
            const int y = y0 - CHESS_BORDER + row, x = x0 - CHESS_LEFT + 4 * col;
            uint32_t v = 0;  // (outside the image: such a sample only reaches pixels whose response is 0 anyway)
            if (y >= 0 && y < h && x + 4 > 0 && x < w) {
                const uint8_t* p = img + (size_t)y * pitch;
                if (IN4 && x >= 0 && x + 4 <= w) {
                    v = *(const uint32_t*)(p + x);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (x + q >= 0 && x + q < w) v |= (uint32_t)p[x + q] << (8 * q);
                }
            }
            tile[k] = v;
        }
        __syncthreads();
        int best = 0;
        const int x = x0 + 4 * tx;
#pragma unroll
        for (int k = 0; k < CHESS_TH / 8; k++) {
            const int ly = ty + 8 * k, y = y0 + ly;
            if (y >= h || x >= w) continue;
            // q[dy + 5][j]: the dword of row y + dy that holds columns x - 8 + 4 j .. x - 5 + 4 j (the unused are never loaded)
            uint32_t q[2 * CHESS_BORDER + 1][5];
#pragma unroll
            for (int dy = 0; dy < 2 * CHESS_BORDER + 1; dy++)
#pragma unroll
                for (int j = 0; j < 5; j++) q[dy][j] = tile[(ly + dy) * CHESS_DWORDS + tx + j];
            int r[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
#define G(dx, dy) ((int)((q[(dy) + 5][(i + (dx) + 8) >> 2] >> (((i + (dx) + 8) & 3) * 8)) & 255u))
                const int I0 = G(5, 0), I1 = G(5, 2), I2 = G(4, 4), I3 = G(2, 5), I4 = G(0, 5), I5 = G(-2, 5), I6 = G(-4, 4),
                          I7 = G(-5, 2), I8 = G(-5, 0), I9 = G(-5, -2), I10 = G(-4, -4), I11 = G(-2, -5), I12 = G(0, -5),
                          I13 = G(2, -5), I14 = G(4, -4), I15 = G(5, -2);
                const int local = G(0, 0) + G(1, 0) + G(-1, 0) + G(0, 1) + G(0, -1);
#undef G
                const int sr = abs(I0 + I8 - I4 - I12) + abs(I1 + I9 - I5 - I13) + abs(I2 + I10 - I6 - I14) + abs(I3 + I11 - I7 - I15);
                const int dr = abs(I0 - I8) + abs(I1 - I9) + abs(I2 - I10) + abs(I3 - I11) + abs(I4 - I12) + abs(I5 - I13) +
                               abs(I6 - I14) + abs(I7 - I15);
                const int ring = ((I0 + I1) + (I2 + I3)) + ((I4 + I5) + (I6 + I7)) + ((I8 + I9) + (I10 + I11)) + ((I12 + I13) + (I14 + I15));
                const bool inside = x + i >= CHESS_BORDER && x + i < w - CHESS_BORDER && y >= CHESS_BORDER && y < h - CHESS_BORDER;
                r[i] = inside ? 5 * sr - 5 * dr - abs(5 * ring - 16 * local) : 0;
                best = r[i] > best ? r[i] : best;
            }
            int16_t* o = out + ((size_t)f * h + y) * w + x;
            if (OUT8 && x + 4 <= w) {
                uint2 v;
                v.x = (uint32_t)(uint16_t)r[0] | (uint32_t)(uint16_t)r[1] << 16;
                v.y = (uint32_t)(uint16_t)r[2] | (uint32_t)(uint16_t)r[3] << 16;
                *(uint2*)o = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (x + i < w) o[i] = (int16_t)r[i];
            }
        }
        // an integer maximum: exact in whatever order the waves arrive (rmax starts at 0, a border pixel's response)
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int other = __shfl_xor(best, m, 64);
            best = other > best ? other : best;
        }
        if ((threadIdx.x & 63) == 0 && best > 0) atomicMax(rmax + f, best);
        __syncthreads();  // (the next frame's tile)
    }
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------
// the predicate and the sink of the shared compaction: row = frame * h + y
struct ChessPeak {
    const int16_t* r;
    const int* rmax;
    int w, h, relative, radius;
    int* peaks;
    const unsigned long long* rowoff;
    __device__ __forceinline__ bool on(int x, int row) const
    {
        const int f = row / h, y = row - f * h;
        const int16_t* plane = r + (size_t)f * h * w;
        const int v = plane[(size_t)y * w + x];
        if (v <= 0 || relative * v < rmax[f]) return false;
        const int ya = y - radius < 0 ? 0 : y - radius, yb = y + radius > h - 1 ? h - 1 : y + radius;
        const int xa = x - radius < 0 ? 0 : x - radius, xb = x + radius > w - 1 ? w - 1 : x + radius;
        for (int yy = ya; yy <= yb; yy++)
            for (int xx = xa; xx <= xb; xx++) {
                const int q = plane[(size_t)yy * w + xx];
                const bool lower = yy < y || (yy == y && xx < x);  // of equal responses the first in pixel order stays
                if (lower ? v <= q : (v < q)) return false;       // (p itself is not lower and not above itself)
            }
        return true;
    }
    __device__ __forceinline__ void emit(int x, int row, unsigned long long pos) const
    {
        const int f = row / h;
        const unsigned long long k = pos - rowoff[(size_t)f * h];
        if (k < (unsigned long long)CAMD_CHESS_CAPACITY) {
            int* o = peaks + ((size_t)f * CAMD_CHESS_CAPACITY + k) * 2;
            o[0] = x, o[1] = row - f * h;
        }
    }
};

__global__ __launch_bounds__(256) void k_chess_counts(const unsigned long long* __restrict__ rowoff,
                                                     const unsigned long long* __restrict__ total, int h, int frames,
                                                     int* __restrict__ counts)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    const unsigned long long end = f + 1 < frames ? rowoff[(size_t)(f + 1) * h] : *total;
    counts[f] = (int)(end - rowoff[(size_t)f * h]);
}

// the workspace of camd_chess_peaks: the total (padded to 64 bytes), then the compaction's rows
struct ChessWorkspace {
    unsigned long long* total;
    RowWorkspace rows;
    ChessWorkspace(void* ws, int nrows) : total((unsigned long long*)ws), rows((char*)ws + 64, nrows) {}
    static size_t bytes(int nrows) { return 64 + RowWorkspace::bytes(nrows); }
};

// ---- stage 3 ------------------------------------------------------------------------------------------------------
enum { CHESS_FOUND = 0, CHESS_FEW = 1, CHESS_OVERFLOW = 2, CHESS_INCOMPLETE = 4 };

struct ChessWave {  // one wave's slice of LDS
    int x[CAMD_CHESS_CAPACITY], y[CAMD_CHESS_CAPACITY];  // the candidates
    int qlabel[CAMD_CHESS_MAX_CORNERS + 4];               // the labelled ones in the order they were labelled: their cell
    uint16_t queue[CAMD_CHESS_MAX_CORNERS + 4];           // ... and their candidate index
    uint16_t grid[CAMD_CHESS_MAX_CORNERS];                // cell of the bounding box -> candidate
    uint8_t used[CAMD_CHESS_CAPACITY];
};
static_assert(4 * sizeof(ChessWave) <= 64 * 1024, "four waves' slices fit a workgroup's LDS");

// where in the queue the cell's candidate stands, or -1
__device__ __forceinline__ int find_cell(const ChessWave& W, int nl, int lane, int cell)
{
    for (int base = 0; base < nl; base += 64) {
        const int k = base + lane;
        const unsigned long long hit = __ballot(k < nl && W.qlabel[k] == cell);
        if (hit) return base + __ffsll((long long)hit) - 1;
    }
    return -1;
}

// the grid cell of board corner (c, r) under labeling t = swap << 2 | fi << 1 | fj
__device__ __forceinline__ int board_cell(int t, int c, int r, int ni, int nj)
{
    int i = (t & 4) ? r : c, j = (t & 4) ? c : r;
    if (t & 2) i = ni - 1 - i;
    if (t & 1) j = nj - 1 - j;
    return i * nj + j;
}

__global__ __launch_bounds__(256) void k_chess_lattice(const int* __restrict__ peaks, const int* __restrict__ counts, int w,
                                                      int frames, int across, int down, float* __restrict__ corners,
                                                      int* __restrict__ status_out)
{
    __shared__ ChessWave waves[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.x * 4 + wave;
    if (f >= frames) return;  // (the whole wave; there is no barrier to miss)
    ChessWave& W = waves[wave];
    const int n = across * down, count = counts[f];
    float* out = corners + (size_t)f * n * 2;
    int status = count > CAMD_CHESS_CAPACITY ? CHESS_OVERFLOW : count < n ? CHESS_FEW : CHESS_FOUND;
    int ni = 0, nj = 0, chosen = -1;
    if (uniform(status == CHESS_FOUND)) {
        status = CHESS_INCOMPLETE;  // until the board stands
        const int m = count;
        long long sx = 0, sy = 0;
        for (int k = lane; k < m; k += 64) {
            const int px = peaks[((size_t)f * CAMD_CHESS_CAPACITY + k) * 2], py = peaks[((size_t)f * CAMD_CHESS_CAPACITY + k) * 2 + 1];
            W.x[k] = px, W.y[k] = py, W.used[k] = 0;
            sx += px, sy += py;
        }
        wave_lds_fence();
        sx = wave_sum_all_i64(sx), sy = wave_sum_all_i64(sy);
        // 1: the seed, nearest the centroid
        const int s = (int)(nearest(m, lane, [&](int k) {
            const long long dx = (long long)m * W.x[k] - sx, dy = (long long)m * W.y[k] - sy;
            return dx * dx + dy * dy;
        }) & 1023);
        const int x_s = W.x[s], y_s = W.y[s];
        // 2: its nearest neighbour (m >= n >= 4: there is one)
        const int a = (int)(nearest(m, lane, [&](int k) {
            const long long dx = W.x[k] - x_s, dy = W.y[k] - y_s;
            return k == s ? -1ll : dx * dx + dy * dy;
        }) & 1023);
        const int ux = W.x[a] - x_s, uy = W.y[a] - y_s;
        const long long uu = (long long)ux * ux + (long long)uy * uy;
        // 3: the nearest at 30 degrees or more from the line of u
        const unsigned long long bkey = nearest(m, lane, [&](int k) {
            const long long dx = W.x[k] - x_s, dy = W.y[k] - y_s, cr = ux * dy - uy * dx, dd = dx * dx + dy * dy;
            return k != s && 4 * cr * cr >= uu * dd ? dd : -1ll;
        });
        if (uniform(bkey != CHESS_NONE)) {
            const int b = (int)(bkey & 1023);
            const int vx = W.x[b] - x_s, vy = W.y[b] - y_s;
            // 4: breadth first from the seed
            if (lane == 0) W.queue[0] = (uint16_t)s, W.qlabel[0] = pack_cell(0, 0), W.used[s] = 1;
            wave_lds_fence();
            int nl = 1, head = 0;
            while (uniform(head < nl && nl <= n)) {
                const int p = W.queue[head], cell = W.qlabel[head];
                head++;
                const int i = (cell >> 16) - 1024, j = (cell & 0xffff) - 1024, x_p = W.x[p], y_p = W.y[p];
                for (int dir = 0; dir < 4; dir++) {
                    if (uniform(nl > n)) break;
                    const int di = dir == 0 ? 1 : dir == 1 ? -1 : 0, dj = dir == 2 ? 1 : dir == 3 ? -1 : 0;
                    if (uniform(find_cell(W, nl, lane, pack_cell(i + di, j + dj)) >= 0)) continue;
                    int stx = (di + dj) * (di ? ux : vx), sty = (di + dj) * (di ? uy : vy);
                    const int behind = find_cell(W, nl, lane, pack_cell(i - di, j - dj));
                    if (uniform(behind >= 0)) {
                        const int c = W.queue[behind];
                        stx = x_p - W.x[c], sty = y_p - W.y[c];
                    } else {
                        for (int o = -1; o <= 1; o += 2) {  // the parallel pair beside p, the lower side first
                            const int oi = di ? 0 : o, oj = di ? o : 0;
                            const int from = find_cell(W, nl, lane, pack_cell(i + oi, j + oj));
                            const int to = uniform(from >= 0) ? find_cell(W, nl, lane, pack_cell(i + oi + di, j + oj + dj)) : -1;
                            if (uniform(to >= 0)) {
                                const int c0 = W.queue[from], c1 = W.queue[to];
                                stx = W.x[c1] - W.x[c0], sty = W.y[c1] - W.y[c0];
                                break;
                            }
                        }
                    }
                    const int qx = x_p + stx, qy = y_p + sty;
                    const unsigned long long key = nearest(m, lane, [&](int k) {
                        const long long dx = W.x[k] - qx, dy = W.y[k] - qy;
                        return W.used[k] ? -1ll : dx * dx + dy * dy;
                    });
                    if (uniform(key != CHESS_NONE && 4 * (long long)(key >> 10) <= (long long)stx * stx + (long long)sty * sty)) {
                        const int c = (int)(key & 1023);
                        if (lane == 0) W.queue[nl] = (uint16_t)c, W.qlabel[nl] = pack_cell(i + di, j + dj), W.used[c] = 1;
                        nl++;
                        wave_lds_fence();
                    }
                }
            }
            // 5: exactly the board: n cells, all different, in a box of n
            if (uniform(nl == n)) {
                int ia = INT_MAX, ib = INT_MIN, ja = INT_MAX, jb = INT_MIN;
                for (int k = lane; k < n; k += 64) {
                    const int ci = W.qlabel[k] >> 16, cj = W.qlabel[k] & 0xffff;
                    ia = ci < ia ? ci : ia, ib = ci > ib ? ci : ib, ja = cj < ja ? cj : ja, jb = cj > jb ? cj : jb;
                }
                ia = -wave_max_all(-ia), ib = wave_max_all(ib), ja = -wave_max_all(-ja), jb = wave_max_all(jb);
                ni = ib - ia + 1, nj = jb - ja + 1;
                if (uniform((ni == across && nj == down) || (ni == down && nj == across))) {
                    for (int k = lane; k < n; k += 64)
                        W.grid[((W.qlabel[k] >> 16) - ia) * nj + ((W.qlabel[k] & 0xffff) - ja)] = W.queue[k];
                    wave_lds_fence();
                    // 6: of the right-handed labelings of the board's shape, the one whose corner 0 comes first in pixel order
                    long long first = LLONG_MAX;
                    for (int t = 0; t < 8; t++) {
                        const bool fits = (t & 4) ? (ni == down && nj == across) : (ni == across && nj == down);
                        if (!fits) continue;
                        long long cx = 0, cy = 0, rx = 0, ry = 0;  // the steps along a row and down a column, summed
                        for (int r = 0; r < down; r++) {
                            const int e = W.grid[board_cell(t, across - 1, r, ni, nj)], b0 = W.grid[board_cell(t, 0, r, ni, nj)];
                            cx += W.x[e] - W.x[b0], cy += W.y[e] - W.y[b0];
                        }
                        for (int c = 0; c < across; c++) {
                            const int e = W.grid[board_cell(t, c, down - 1, ni, nj)], b0 = W.grid[board_cell(t, c, 0, ni, nj)];
                            rx += W.x[e] - W.x[b0], ry += W.y[e] - W.y[b0];
                        }
                        if (cx * ry - cy * rx <= 0) continue;
                        const int c0 = W.grid[board_cell(t, 0, 0, ni, nj)];
                        const long long key = (long long)W.y[c0] * w + W.x[c0];
                        if (key < first) first = key, chosen = t;
                    }
                    chosen = __builtin_amdgcn_readfirstlane(chosen);
                    if (chosen >= 0) status = CHESS_FOUND;
                }
            }
        }
    }
    // 7
    for (int k = lane; k < n; k += 64) {
        float px = NAN, py = NAN;
        if (status == CHESS_FOUND) {
            const int c = W.grid[board_cell(chosen, k % across, k / across, ni, nj)];
            px = (float)W.x[c], py = (float)W.y[c];
        }
        out[2 * k] = px, out[2 * k + 1] = py;
    }
    if (lane == 0) status_out[f] = status;
}

static bool chess_limits(const char* who, int across, int down, int relative, int nms_radius)
{
    if (across < 2 || down < 2 || (long long)across * down > CAMD_CHESS_MAX_CORNERS || relative < 1 || relative > 64 ||
        nms_radius < 1 || nms_radius > 8) {
        set_error("%s: a pattern of %d x %d corners, relative %d, nms_radius %d: the detector takes across, down >= 2 with at most "
                  "%d corners, relative 1 .. 64 and nms_radius 1 .. 8", who, across, down, relative, nms_radius,
                  CAMD_CHESS_MAX_CORNERS);
        return false;
    }
    return true;
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_chess_response(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, int16_t* response,
                        int* response_max, void* queue)
{
    if (!gray || !response || !response_max || w < 1 || h < 1 || frames < 1 || pitch < (size_t)w ||
        (frames > 1 && stride < (size_t)(h - 1) * pitch + (size_t)w) || (uintptr_t)response % 2 != 0 ||
        (uintptr_t)response_max % 4 != 0 || (long long)frames * h >= (1LL << 31)) {
        set_error("camd_chess_response: bad arguments (gray, response, response_max: device arrays, aligned to an element; w, h, "
                  "frames > 0 with frames * h < 2^31; pitch >= w, stride >= an image)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    CAMD_HIP(hipMemsetAsync(response_max, 0, (size_t)frames * sizeof(int), st));
    const bool in4 = ((uintptr_t)gray | pitch | stride) % 4 == 0, out8 = (uintptr_t)response % 8 == 0 && w % 4 == 0;
    const dim3 grid(div_up(w, CHESS_TW), div_up(h, CHESS_TH), frames < 65535 ? frames : 65535);
#define ARGS gray, w, h, pitch, stride, frames, response, response_max
    if (in4 && out8) hipLaunchKernelGGL((k_chess_response<true, true>), grid, dim3(256), 0, st, ARGS);
    else if (in4) hipLaunchKernelGGL((k_chess_response<true, false>), grid, dim3(256), 0, st, ARGS);
    else if (out8) hipLaunchKernelGGL((k_chess_response<false, true>), grid, dim3(256), 0, st, ARGS);
    else hipLaunchKernelGGL((k_chess_response<false, false>), grid, dim3(256), 0, st, ARGS);
#undef ARGS
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

size_t camd_chess_peaks_workspace_bytes(int h, int frames)
{
    if (h < 1 || frames < 1 || (long long)frames * h >= (1LL << 31)) return 0;
    return ChessWorkspace::bytes(frames * h);
}

int camd_chess_peaks(const int16_t* response, const int* response_max, int w, int h, int frames, int relative, int nms_radius,
                     void* workspace, int* peaks, int* counts, void* queue)
{
    if (!chess_limits("camd_chess_peaks", 2, 2, relative, nms_radius)) return CAMD_ERR_UNSUPPORTED;
    if (!response || !response_max || !workspace || !peaks || !counts || w < 1 || h < 1 || frames < 1 ||
        (long long)frames * h >= (1LL << 31) || (uintptr_t)response % 2 != 0 || (uintptr_t)response_max % 4 != 0 ||
        (uintptr_t)workspace % 8 != 0 || (uintptr_t)peaks % 4 != 0 || (uintptr_t)counts % 4 != 0) {
        set_error("camd_chess_peaks: bad arguments (response, response_max, workspace, peaks, counts: device arrays, aligned to an "
                  "element, the workspace to 8 bytes; w, h, frames > 0 with frames * h < 2^31)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    const int rows = frames * h;
    const ChessWorkspace ws(workspace, rows);
    const ChessPeak f = {response, response_max, w, h, relative, nms_radius, peaks, ws.rows.rowoff};
    row_count(f, w, rows, ws.rows.rowcount, st);
    row_scan(ws.rows.rowcount, rows, ws.rows.rowoff, ws.total, st);
    row_emit(f, w, rows, ws.rows.rowoff, ~(size_t)0, nullptr, st);  // (the capacity is per frame: ChessPeak::emit holds it)
    hipLaunchKernelGGL(k_chess_counts, dim3(div_up(frames, 256)), dim3(256), 0, st, ws.rows.rowoff, ws.total, h, frames, counts);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_chess_lattice(const int* peaks, const int* counts, int w, int h, int frames, int across, int down, float* corners,
                       int* status, void* queue)
{
    if (!chess_limits("camd_chess_lattice", across, down, 1, 1)) return CAMD_ERR_UNSUPPORTED;
    if (w > CHESS_MAX_SIDE || h > CHESS_MAX_SIDE) {
        set_error("camd_chess_lattice: an image of %d x %d; the lattice takes sides up to %d", w, h, CHESS_MAX_SIDE);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (!peaks || !counts || !corners || !status || w < 1 || h < 1 || frames < 1 || (uintptr_t)peaks % 4 != 0 ||
        (uintptr_t)counts % 4 != 0 || (uintptr_t)corners % 4 != 0 || (uintptr_t)status % 4 != 0) {
        set_error("camd_chess_lattice: bad arguments (peaks, counts, corners, status: device arrays, aligned to an element; w, h, "
                  "frames > 0)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_chess_lattice, dim3(div_up(frames, 4)), dim3(256), 0, (hipStream_t)queue, peaks, counts, w, frames, across,
                       down, corners, status);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
