// charuco.hip -- the inner corners of a ChArUco board, by id, in every frame of a recording at once; boards cut by the
// image or partly covered included.
//
// Stands where the reference calls cv2.aruco.detectMarkers / interpolateCornersCharuco (boards.py:359-368), with a
// contract of its own: stages 1 and 2 are chessboard.hip's (ChESS response, peaks) -- a
// ChArUco board's inner corners are X-junctions --, and this file turns a frame's peaks into numbered corners:
//   lattice   a seed cell: a peak, two of its near neighbours and the fourth corner they point to, in which a marker
//             of the board decodes; from it the peaks are labelled breadth first, step by step, wherever they are present
//   decode    every lattice cell with four labelled corners: (s + 2)^2 samples placed by a fixed-point bilinear blend of
//             the corners, thresholded between their extremes, a black ring, s*s bits matched in four turns
//   vote      each marker fixes the turn and offset between lattice and board; the one most markers agree on numbers
//             the corners
// Integers end to end, restated in NumPy by tests/charuco_ref.py.  One wavefront per frame, four frames per workgroup,
// NO workgroup barrier, as k_chess_lattice: the wave's state lives in its own slice of LDS, what decides a branch is the
// same in every lane, and every loop is bounded by a constant, CAMD_CHESS_CAPACITY or the board.
#include <climits>
#include <cmath>

#include "chess_wave.hpp"
#include "marker_decode.hpp"

namespace camd {

constexpr int CHARUCO_RANGE = 15;                       // lattice labels run -15 .. 15 about the seed
constexpr int CHARUCO_GRID = 2 * CHARUCO_RANGE + 3;     // ... and the grid one further, so a label's neighbours are in it
constexpr int CHARUCO_LABELS = 320;                     // corners one lattice holds
constexpr int CHARUCO_SEED_SCAN = 32, CHARUCO_SEED_TRIES = 4, CHARUCO_NEIGHBOURS = 16;
constexpr int CHARUCO_MIN_PEAKS = 5;
constexpr int CHARUCO_MAX_SIDE = 16384;
constexpr uint16_t CHARUCO_ABSENT = 0xffff;
enum { CHARUCO_FOUND = 0, CHARUCO_FEW = 1, CHARUCO_OVERFLOW = 2, CHARUCO_NO_LATTICE = 4, CHARUCO_NO_CONSENSUS = 8 };
static_assert(CAMD_CHARUCO_MAX_SQUARES - 1 <= CHARUCO_RANGE, "a board's corners fit the labels whichever corner is the seed");
static_assert(CAMD_CHARUCO_MAX_SQUARES * CAMD_CHARUCO_MAX_SQUARES <= 256, "the maps of a board's corners and squares");

struct CharucoWave {  // one wave's slice of LDS
    short x[CAMD_CHESS_CAPACITY], y[CAMD_CHESS_CAPACITY];  // the candidates (sides up to 16384)
    int qcell[CHARUCO_LABELS];                             // the labelled ones in the order they were labelled: their cell
    int vote[CHARUCO_LABELS];                              // of the cell whose least corner this one is: turn and offset, or -1
    uint16_t queue[CHARUCO_LABELS];                        // ... their candidate index
    short marker[CHARUCO_LABELS];                          // ... the marker decoded in that cell
    uint16_t grid[CHARUCO_GRID * CHARUCO_GRID];            // cell -> candidate
    uint16_t corner_of[256];                               // inner corner id -> candidate
    short marker_of[256];                                  // square -> marker id
    uint8_t flags[CAMD_CHESS_CAPACITY];                    // 1: labelled in the lattice at hand; 2: in one that failed
};
static_assert(4 * sizeof(CharucoWave) <= 64 * 1024, "four waves' slices fit a workgroup's LDS");

__device__ __forceinline__ int grid_at(int i, int j) { return (i + CHARUCO_RANGE + 1) * CHARUCO_GRID + (j + CHARUCO_RANGE + 1); }

// `nearest` among the keys from `lower` on: the candidates in order of (distance, index), one after the other
template <typename D>
__device__ __forceinline__ unsigned long long nearest_from(int m, int lane, unsigned long long lower, D d)
{
    unsigned long long best = CHESS_NONE;
    for (int k = lane; k < m; k += 64) {
        const long long v = d(k);
        const unsigned long long key = (unsigned long long)v << 10 | (unsigned)k;
        if (v >= 0 && key >= lower && key < best) best = key;
    }
    return wave_min_all(best);
}

struct CharucoBoard {
    const uint8_t* img;  // the frame
    int w, h;
    size_t pitch;
    int sx, sy, num, den, s, n_ids, first_id, max_errors;
    const unsigned long long* words;
};

// the square y * sx + x of the marker of that rank among the squares with x % 2 != y % 2 in row-major order, or -1
__device__ __forceinline__ int marker_square(int rank, int sx, int sy)
{
    if (rank < 0) return -1;
    const int pair = rank / sx, rem = rank - pair * sx, half = sx / 2;
    const int x = rem < half ? 2 * rem + 1 : 2 * (rem - half), y = rem < half ? 2 * pair : 2 * pair + 1;
    return y < sy ? y * sx + x : -1;
}

// The marker in the lattice cell with corners c00, c10 (one step along i), c01 (along j), c11, by the whole wave: id << 2 |
// turn, or -1; the same in every lane (marker_decode.hpp samples and matches).
__device__ int decode_cell(const CharucoBoard& B, const CharucoWave& W, int lane, int c00, int c10, int c01, int c11)
{
    const MarkerImage image = {B.img, B.w, B.h, B.pitch};
    const unsigned long long best = decode_marker(image, B.s, B.num, B.den, B.words, B.n_ids, B.max_errors, lane, W.x[c00], W.y[c00],
                                                  W.x[c10], W.y[c10], W.x[c01], W.y[c01], W.x[c11], W.y[c11]);
    return best == CHESS_NONE ? -1 : (int)(best & 0xffff);
}

// the board corner of lattice corner (i, j) under a turn and an offset; corner (cx, cy) is the top-left one of square (cx, cy)
__device__ __forceinline__ void board_corner(int turn, int ox, int oy, int i, int j, int& cx, int& cy)
{
    cx = ox + (turn == 0 ? i : turn == 1 ? j : turn == 2 ? -i : -j);
    cy = oy + (turn == 0 ? j : turn == 1 ? -i : turn == 2 ? -j : i);
}

__global__ __launch_bounds__(256) void k_charuco(const int* __restrict__ peaks, const int* __restrict__ counts,
                                                const uint8_t* __restrict__ gray, int w, int h, size_t pitch, size_t stride,
                                                int frames, int sx, int sy, int num, int den,
                                                const unsigned long long* __restrict__ words, int n_ids, int s, int first_id,
                                                int min_markers, int max_errors, float* __restrict__ corners,
                                                int* __restrict__ marker_ids, int* __restrict__ status_out)
{
    __shared__ CharucoWave waves[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.x * 4 + wave;
    if (f >= frames) return;  // (the whole wave; there is no barrier to miss)
    CharucoWave& W = waves[wave];
    const CharucoBoard B = {gray + (size_t)f * stride, w, h, pitch, sx, sy, num, den, s, n_ids, first_id, max_errors, words};
    const int n = (sx - 1) * (sy - 1), count = counts[f];
    int status = count > CAMD_CHESS_CAPACITY ? CHARUCO_OVERFLOW : count < CHARUCO_MIN_PEAKS ? CHARUCO_FEW : CHARUCO_NO_LATTICE;
    int nl = 0, chosen = -1;
    if (uniform(status == CHARUCO_NO_LATTICE)) {
        const int m = count;
        long long sumx = 0, sumy = 0;
        for (int k = lane; k < m; k += 64) {
            const int px = peaks[((size_t)f * CAMD_CHESS_CAPACITY + k) * 2], py = peaks[((size_t)f * CAMD_CHESS_CAPACITY + k) * 2 + 1];
            W.x[k] = (short)px, W.y[k] = (short)py, W.flags[k] = 0;
            sumx += px, sumy += py;
        }
        wave_lds_fence();
        sumx = wave_sum_all_i64(sumx), sumy = wave_sum_all_i64(sumy);
        unsigned long long seed_lower = 0;
        int grown = 0;
        for (int scan = 0; scan < CHARUCO_SEED_SCAN; scan++) {
            // 1: the next seed in order of distance from the centroid
            const unsigned long long skey = nearest_from(m, lane, seed_lower, [&](int k) {
                const long long dx = (long long)m * W.x[k] - sumx, dy = (long long)m * W.y[k] - sumy;
                return dx * dx + dy * dy;
            });
            if (uniform(skey == CHESS_NONE)) break;
            seed_lower = skey + 1;
            const int seed = (int)(skey & 1023);
            if (uniform((W.flags[seed] & 2) != 0)) continue;
            const int x_s = W.x[seed], y_s = W.y[seed];
            // 2: its steps u, v -- a cell of near neighbours in which a marker of the board decodes
            bool have = false;
            int ux = 0, uy = 0, vx = 0, vy = 0;
            unsigned long long a_lower = 0;
            for (int ia = 0; ia < CHARUCO_NEIGHBOURS && !have; ia++) {
                const unsigned long long akey = nearest_from(m, lane, a_lower, [&](int k) {
                    const long long dx = W.x[k] - x_s, dy = W.y[k] - y_s;
                    return k == seed ? -1ll : dx * dx + dy * dy;
                });
                if (uniform(akey == CHESS_NONE)) break;
                a_lower = akey + 1;
                const int a = (int)(akey & 1023);
                const int ax = W.x[a] - x_s, ay = W.y[a] - y_s;
                const long long uu = (long long)ax * ax + (long long)ay * ay;
                unsigned long long b_lower = 0;
                for (int ib = 0; ib < CHARUCO_NEIGHBOURS; ib++) {
                    const unsigned long long bkey = nearest_from(m, lane, b_lower, [&](int k) {
                        const long long dx = W.x[k] - x_s, dy = W.y[k] - y_s, cr = ax * dy - ay * dx, dd = dx * dx + dy * dy;
                        return k != seed && 4 * cr * cr >= uu * dd ? dd : -1ll;
                    });
                    if (uniform(bkey == CHESS_NONE)) break;
                    b_lower = bkey + 1;
                    const int b = (int)(bkey & 1023);
                    const int bx = W.x[b] - x_s, by = W.y[b] - y_s;
                    const long long vv = (long long)bx * bx + (long long)by * by;
                    const int qx = x_s + ax + bx, qy = y_s + ay + by;
                    const unsigned long long ckey = nearest(m, lane, [&](int k) {
                        const long long dx = W.x[k] - qx, dy = W.y[k] - qy;
                        return k == seed || k == a || k == b ? -1ll : dx * dx + dy * dy;
                    });
                    if (uniform(ckey == CHESS_NONE || 16 * (long long)(ckey >> 10) > (uu < vv ? uu : vv))) continue;
                    const bool flip = (long long)ax * by - (long long)ay * bx < 0;
                    const int got = decode_cell(B, W, lane, seed, flip ? b : a, flip ? a : b, (int)(ckey & 1023));
                    if (uniform(got >= 0 && marker_square((got >> 2) - first_id, sx, sy) >= 0)) {
                        have = true;
                        ux = flip ? bx : ax, uy = flip ? by : ay, vx = flip ? ax : bx, vy = flip ? ay : by;
                        break;
                    }
                }
            }
            if (uniform(!have)) continue;
            grown++;
            // 3: breadth first from the seed, cell (0, 0)
            for (int k = lane; k < CHARUCO_GRID * CHARUCO_GRID; k += 64) W.grid[k] = CHARUCO_ABSENT;
            wave_lds_fence();
            if (lane == 0) W.queue[0] = (uint16_t)seed, W.qcell[0] = pack_cell(0, 0), W.grid[grid_at(0, 0)] = (uint16_t)seed, W.flags[seed] |= 1;
            wave_lds_fence();
            nl = 1;
            int head = 0;
            while (uniform(head < nl && nl < CHARUCO_LABELS)) {
                const int p = W.queue[head], cell = W.qcell[head];
                head++;
                const int i = (cell >> 16) - 1024, j = (cell & 0xffff) - 1024, x_p = W.x[p], y_p = W.y[p];
                for (int dir = 0; dir < 4; dir++) {
                    if (uniform(nl >= CHARUCO_LABELS)) break;
                    const int di = dir == 0 ? 1 : dir == 1 ? -1 : 0, dj = dir == 2 ? 1 : dir == 3 ? -1 : 0;
                    const int ti = i + di, tj = j + dj;
                    if (uniform(abs(ti) > CHARUCO_RANGE || abs(tj) > CHARUCO_RANGE || W.grid[grid_at(ti, tj)] != CHARUCO_ABSENT)) continue;
                    int stx = (di + dj) * (di ? ux : vx), sty = (di + dj) * (di ? uy : vy);
                    const int behind = W.grid[grid_at(i - di, j - dj)];
                    if (uniform(behind != CHARUCO_ABSENT)) {
                        stx = x_p - W.x[behind], sty = y_p - W.y[behind];
                    } else {
                        for (int o = -1; o <= 1; o += 2) {  // the parallel pair beside p, the lower side first
                            const int oi = di ? 0 : o, oj = di ? o : 0;
                            const int c0 = W.grid[grid_at(i + oi, j + oj)], c1 = W.grid[grid_at(i + oi + di, j + oj + dj)];
                            if (uniform(c0 != CHARUCO_ABSENT && c1 != CHARUCO_ABSENT)) {
                                stx = W.x[c1] - W.x[c0], sty = W.y[c1] - W.y[c0];
                                break;
                            }
                        }
                    }
                    const int qx = x_p + stx, qy = y_p + sty;
                    const unsigned long long key = nearest(m, lane, [&](int k) {
                        const long long dx = W.x[k] - qx, dy = W.y[k] - qy;
                        return (W.flags[k] & 1) ? -1ll : dx * dx + dy * dy;
                    });
                    if (uniform(key != CHESS_NONE && 64 * (long long)(key >> 10) <= (long long)stx * stx + (long long)sty * sty)) {  // an eighth of the step
                        const int c = (int)(key & 1023);
                        if (lane == 0) {
                            W.queue[nl] = (uint16_t)c, W.qcell[nl] = pack_cell(ti, tj), W.grid[grid_at(ti, tj)] = (uint16_t)c;
                            W.flags[c] |= 1;
                        }
                        nl++;
                        wave_lds_fence();
                    }
                }
            }
            // 4: the marker of every cell whose four corners are labelled, and the turn and offset it stands for
            for (int k = 0; k < nl; k++) {
                const int cell = W.qcell[k], i = (cell >> 16) - 1024, j = (cell & 0xffff) - 1024;
                const int c10 = W.grid[grid_at(i + 1, j)], c01 = W.grid[grid_at(i, j + 1)], c11 = W.grid[grid_at(i + 1, j + 1)];
                int vote = -1, id = -1;
                if (uniform(c10 != CHARUCO_ABSENT && c01 != CHARUCO_ABSENT && c11 != CHARUCO_ABSENT)) {
                    const int got = decode_cell(B, W, lane, W.queue[k], c10, c01, c11);
                    const int square = got >= 0 ? marker_square((got >> 2) - first_id, sx, sy) : -1;
                    if (square >= 0) {
                        const int turn = got & 3, qy = square / sx, qx = square - qy * sx;
                        const int ox = turn == 0 ? qx - i : turn == 1 ? qx - j : turn == 2 ? qx + i + 1 : qx + j + 1;
                        const int oy = turn == 0 ? qy - j : turn == 1 ? qy + i + 1 : turn == 2 ? qy + j + 1 : qy - i;
                        vote = turn << 12 | (ox + 32) << 6 | (oy + 32);
                        id = got >> 2;
                    }
                }
                if (lane == 0) W.vote[k] = vote, W.marker[k] = (short)id;
            }
            wave_lds_fence();
            // 5: the vote most markers cast, the lowest of equals
            int best = 0;
            long long cast = 0;
            for (int k = lane; k < nl; k += 64) {
                const int mine = W.vote[k];
                if (mine < 0) continue;
                int agree = 0;
                for (int q = 0; q < nl; q++) agree += W.vote[q] == mine;
                const int key = agree << 14 | (0x3fff - mine);
                best = key > best ? key : best;
                cast++;
            }
            best = wave_max_all(best);
            cast = wave_sum_all_i64(cast);
            const int agree = best >> 14;
            if (uniform(cast > 0 && agree >= min_markers && cast - agree <= agree)) {
                chosen = 0x3fff - (best & 0x3fff);
                status = CHARUCO_FOUND;
                break;
            }
            status = CHARUCO_NO_CONSENSUS;
            for (int k = lane; k < m; k += 64)
                if (W.flags[k] & 1) W.flags[k] = 2;
            wave_lds_fence();
            if (uniform(grown == CHARUCO_SEED_TRIES)) break;
        }
    }
    // 6: the corners by id, the markers by square
    for (int k = lane; k < 256; k += 64) W.corner_of[k] = CHARUCO_ABSENT, W.marker_of[k] = -1;
    wave_lds_fence();
    if (uniform(status == CHARUCO_FOUND)) {
        const int turn = chosen >> 12, ox = ((chosen >> 6) & 63) - 32, oy = (chosen & 63) - 32;
        for (int k = lane; k < nl; k += 64) {
            const int cell = W.qcell[k], i = (cell >> 16) - 1024, j = (cell & 0xffff) - 1024;
            int cx, cy;
            board_corner(turn, ox, oy, i, j, cx, cy);
            if (cx >= 1 && cx <= sx - 1 && cy >= 1 && cy <= sy - 1) W.corner_of[(cy - 1) * (sx - 1) + cx - 1] = W.queue[k];
            if (W.vote[k] == chosen) W.marker_of[marker_square(W.marker[k] - first_id, sx, sy)] = W.marker[k];
        }
        wave_lds_fence();
    }
    float* out = corners + (size_t)f * n * 2;
    for (int k = lane; k < n; k += 64) {
        const int c = W.corner_of[k];
        out[2 * k] = c == CHARUCO_ABSENT ? NAN : (float)W.x[c], out[2 * k + 1] = c == CHARUCO_ABSENT ? NAN : (float)W.y[c];
    }
    for (int k = lane; k < sx * sy; k += 64) marker_ids[(size_t)f * sx * sy + k] = W.marker_of[k];
    if (lane == 0) status_out[f] = status;
}

// ---- every board of a set in one frame -----------------------------------------------------------------------------------
// The boards share squares, ratio and dictionary and differ in first_id; their id ranges are disjoint, so a decoded marker
// names its board.  One pass over one set of peaks: a seed cell qualifies by a marker of a board not yet found, a lattice's
// markers vote (board, turn, offset), the winner's board is found and written out at once -- its rows of the outputs are the
// only per-board state, so the slice of LDS is k_charuco's -- and its peaks are labelled no more.  With one board every
// step is k_charuco's (tests/multiboard_ref.py restates the rules; flags: 4 = labelled in an accepted lattice).

// the board of the set whose id range holds marker `id`, and the marker's square on it; -1 where none does
__device__ __forceinline__ int board_of(const camd_charuco_boards& set, int id, int sx, int sy, int& square)
{
    int board = -1;
    square = -1;
#pragma unroll
    for (int b = 0; b < CAMD_CHARUCO_MAX_BOARDS; b++) {
        const int sq = b < set.n ? marker_square(id - set.first_id[b], sx, sy) : -1;
        if (sq >= 0 && board < 0) board = b, square = sq;
    }
    return board;
}

__global__ __launch_bounds__(256) void k_charuco_multi(const int* __restrict__ peaks, const int* __restrict__ counts,
                                                      const uint8_t* __restrict__ gray, int w, int h, size_t pitch, size_t stride,
                                                      int frames, int sx, int sy, int num, int den,
                                                      const unsigned long long* __restrict__ words, int n_ids, int s,
                                                      camd_charuco_boards set, int min_markers, int max_errors,
                                                      float* __restrict__ corners, int* __restrict__ marker_ids,
                                                      int* __restrict__ status_out)
{
    __shared__ CharucoWave waves[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.x * 4 + wave;
    if (f >= frames) return;  // (the whole wave; there is no barrier to miss)
    CharucoWave& W = waves[wave];
    const CharucoBoard B = {gray + (size_t)f * stride, w, h, pitch, sx, sy, num, den, s, n_ids, 0, max_errors, words};
    const int n = (sx - 1) * (sy - 1), count = counts[f], nb = set.n;
    const int frame_status = count > CAMD_CHESS_CAPACITY ? CHARUCO_OVERFLOW : count < CHARUCO_MIN_PEAKS ? CHARUCO_FEW : CHARUCO_NO_LATTICE;
    const unsigned every = (1u << nb) - 1;
    unsigned found = 0, tried = 0;  // bit b: board b
    if (uniform(frame_status == CHARUCO_NO_LATTICE)) {
        const int m = count;
        long long sumx = 0, sumy = 0;
        for (int k = lane; k < m; k += 64) {
            const int px = peaks[((size_t)f * CAMD_CHESS_CAPACITY + k) * 2], py = peaks[((size_t)f * CAMD_CHESS_CAPACITY + k) * 2 + 1];
            W.x[k] = (short)px, W.y[k] = (short)py, W.flags[k] = 0;
            sumx += px, sumy += py;
        }
        wave_lds_fence();
        sumx = wave_sum_all_i64(sumx), sumy = wave_sum_all_i64(sumy);
        unsigned long long seed_lower = 0;
        int grown = 0;
        for (int scan = 0; scan < CHARUCO_SEED_SCAN * nb; scan++) {
            if (uniform(found == every)) break;
            // 1: the next seed in order of distance from the centroid; a peak some lattice has labelled seeds no more
            const unsigned long long skey = nearest_from(m, lane, seed_lower, [&](int k) {
                const long long dx = (long long)m * W.x[k] - sumx, dy = (long long)m * W.y[k] - sumy;
                return dx * dx + dy * dy;
            });
            if (uniform(skey == CHESS_NONE)) break;
            seed_lower = skey + 1;
            const int seed = (int)(skey & 1023);
            if (uniform((W.flags[seed] & 6) != 0)) continue;
            const int x_s = W.x[seed], y_s = W.y[seed];
            // 2: its steps u, v -- a cell of near neighbours in which a marker of a board not yet found decodes
            bool have = false;
            int ux = 0, uy = 0, vx = 0, vy = 0, seed_board = 0;
            unsigned long long a_lower = 0;
            for (int ia = 0; ia < CHARUCO_NEIGHBOURS && !have; ia++) {
                const unsigned long long akey = nearest_from(m, lane, a_lower, [&](int k) {
                    const long long dx = W.x[k] - x_s, dy = W.y[k] - y_s;
                    return k == seed ? -1ll : dx * dx + dy * dy;
                });
                if (uniform(akey == CHESS_NONE)) break;
                a_lower = akey + 1;
                const int a = (int)(akey & 1023);
                const int ax = W.x[a] - x_s, ay = W.y[a] - y_s;
                const long long uu = (long long)ax * ax + (long long)ay * ay;
                unsigned long long b_lower = 0;
                for (int ib = 0; ib < CHARUCO_NEIGHBOURS; ib++) {
                    const unsigned long long bkey = nearest_from(m, lane, b_lower, [&](int k) {
                        const long long dx = W.x[k] - x_s, dy = W.y[k] - y_s, cr = ax * dy - ay * dx, dd = dx * dx + dy * dy;
                        return k != seed && 4 * cr * cr >= uu * dd ? dd : -1ll;
                    });
                    if (uniform(bkey == CHESS_NONE)) break;
                    b_lower = bkey + 1;
                    const int b = (int)(bkey & 1023);
                    const int bx = W.x[b] - x_s, by = W.y[b] - y_s;
                    const long long vv = (long long)bx * bx + (long long)by * by;
                    const int qx = x_s + ax + bx, qy = y_s + ay + by;
                    const unsigned long long ckey = nearest(m, lane, [&](int k) {
                        const long long dx = W.x[k] - qx, dy = W.y[k] - qy;
                        return k == seed || k == a || k == b ? -1ll : dx * dx + dy * dy;
                    });
                    if (uniform(ckey == CHESS_NONE || 16 * (long long)(ckey >> 10) > (uu < vv ? uu : vv))) continue;
                    const bool flip = (long long)ax * by - (long long)ay * bx < 0;
                    const int got = decode_cell(B, W, lane, seed, flip ? b : a, flip ? a : b, (int)(ckey & 1023));
                    int square;
                    const int board = got >= 0 ? board_of(set, got >> 2, sx, sy, square) : -1;
                    if (uniform(board >= 0 && !(found >> board & 1))) {
                        have = true, seed_board = board;
                        ux = flip ? bx : ax, uy = flip ? by : ay, vx = flip ? ax : bx, vy = flip ? ay : by;
                        break;
                    }
                }
            }
            if (uniform(!have)) continue;
            grown++;
            // 3: breadth first from the seed, cell (0, 0), over the peaks no accepted lattice holds
            for (int k = lane; k < CHARUCO_GRID * CHARUCO_GRID; k += 64) W.grid[k] = CHARUCO_ABSENT;
            wave_lds_fence();
            if (lane == 0) W.queue[0] = (uint16_t)seed, W.qcell[0] = pack_cell(0, 0), W.grid[grid_at(0, 0)] = (uint16_t)seed, W.flags[seed] |= 1;
            wave_lds_fence();
            int nl = 1, head = 0;
            while (uniform(head < nl && nl < CHARUCO_LABELS)) {
                const int p = W.queue[head], cell = W.qcell[head];
                head++;
                const int i = (cell >> 16) - 1024, j = (cell & 0xffff) - 1024, x_p = W.x[p], y_p = W.y[p];
                for (int dir = 0; dir < 4; dir++) {
                    if (uniform(nl >= CHARUCO_LABELS)) break;
                    const int di = dir == 0 ? 1 : dir == 1 ? -1 : 0, dj = dir == 2 ? 1 : dir == 3 ? -1 : 0;
                    const int ti = i + di, tj = j + dj;
                    if (uniform(abs(ti) > CHARUCO_RANGE || abs(tj) > CHARUCO_RANGE || W.grid[grid_at(ti, tj)] != CHARUCO_ABSENT)) continue;
                    int stx = (di + dj) * (di ? ux : vx), sty = (di + dj) * (di ? uy : vy);
                    const int behind = W.grid[grid_at(i - di, j - dj)];
                    if (uniform(behind != CHARUCO_ABSENT)) {
                        stx = x_p - W.x[behind], sty = y_p - W.y[behind];
                    } else {
                        for (int o = -1; o <= 1; o += 2) {  // the parallel pair beside p, the lower side first
                            const int oi = di ? 0 : o, oj = di ? o : 0;
                            const int c0 = W.grid[grid_at(i + oi, j + oj)], c1 = W.grid[grid_at(i + oi + di, j + oj + dj)];
                            if (uniform(c0 != CHARUCO_ABSENT && c1 != CHARUCO_ABSENT)) {
                                stx = W.x[c1] - W.x[c0], sty = W.y[c1] - W.y[c0];
                                break;
                            }
                        }
                    }
                    const int qx = x_p + stx, qy = y_p + sty;
                    const unsigned long long key = nearest(m, lane, [&](int k) {
                        const long long dx = W.x[k] - qx, dy = W.y[k] - qy;
                        return (W.flags[k] & 5) ? -1ll : dx * dx + dy * dy;
                    });
                    if (uniform(key != CHESS_NONE && 64 * (long long)(key >> 10) <= (long long)stx * stx + (long long)sty * sty)) {  // an eighth of the step
                        const int c = (int)(key & 1023);
                        if (lane == 0) {
                            W.queue[nl] = (uint16_t)c, W.qcell[nl] = pack_cell(ti, tj), W.grid[grid_at(ti, tj)] = (uint16_t)c;
                            W.flags[c] |= 1;
                        }
                        nl++;
                        wave_lds_fence();
                    }
                }
            }
            // 4: the marker of every cell whose four corners are labelled; one of a board not yet found casts its board,
            //    turn and offset
            for (int k = 0; k < nl; k++) {
                const int cell = W.qcell[k], i = (cell >> 16) - 1024, j = (cell & 0xffff) - 1024;
                const int c10 = W.grid[grid_at(i + 1, j)], c01 = W.grid[grid_at(i, j + 1)], c11 = W.grid[grid_at(i + 1, j + 1)];
                int vote = -1, id = -1;
                if (uniform(c10 != CHARUCO_ABSENT && c01 != CHARUCO_ABSENT && c11 != CHARUCO_ABSENT)) {
                    const int got = decode_cell(B, W, lane, W.queue[k], c10, c01, c11);
                    int square;
                    const int board = got >= 0 ? board_of(set, got >> 2, sx, sy, square) : -1;
                    if (board >= 0 && !(found >> board & 1)) {
                        const int turn = got & 3, qy = square / sx, qx = square - qy * sx;
                        const int ox = turn == 0 ? qx - i : turn == 1 ? qx - j : turn == 2 ? qx + i + 1 : qx + j + 1;
                        const int oy = turn == 0 ? qy - j : turn == 1 ? qy + i + 1 : turn == 2 ? qy + j + 1 : qy - i;
                        vote = board << 14 | turn << 12 | (ox + 32) << 6 | (oy + 32);
                        id = got >> 2;
                    }
                }
                if (lane == 0) W.vote[k] = vote, W.marker[k] = (short)id;
            }
            wave_lds_fence();
            // 5: the vote most markers cast, the lowest of equals
            int best = 0;
            long long cast = 0;
            for (int k = lane; k < nl; k += 64) {
                const int mine = W.vote[k];
                if (mine < 0) continue;
                int agree = 0;
                for (int q = 0; q < nl; q++) agree += W.vote[q] == mine;
                const int key = agree << 17 | (0x1ffff - mine);
                best = key > best ? key : best;
                cast++;
            }
            best = wave_max_all(best);
            cast = wave_sum_all_i64(cast);
            const int agree = best >> 17;
            if (uniform(cast > 0 && agree >= min_markers && cast - agree <= agree)) {
                // 6: the winner's board is found: its corners by id and its markers by square, written to its own rows
                const int chosen = 0x1ffff - (best & 0x1ffff);
                const int board = chosen >> 14, turn = (chosen >> 12) & 3, ox = ((chosen >> 6) & 63) - 32, oy = (chosen & 63) - 32;
                const int first_id = set.first_id[board];
                found |= 1u << board;
                for (int k = lane; k < 256; k += 64) W.corner_of[k] = CHARUCO_ABSENT, W.marker_of[k] = -1;
                wave_lds_fence();
                for (int k = lane; k < nl; k += 64) {
                    const int cell = W.qcell[k], i = (cell >> 16) - 1024, j = (cell & 0xffff) - 1024;
                    int cx, cy;
                    board_corner(turn, ox, oy, i, j, cx, cy);
                    if (cx >= 1 && cx <= sx - 1 && cy >= 1 && cy <= sy - 1) W.corner_of[(cy - 1) * (sx - 1) + cx - 1] = W.queue[k];
                    if (W.vote[k] == chosen) W.marker_of[marker_square(W.marker[k] - first_id, sx, sy)] = W.marker[k];
                }
                wave_lds_fence();
                const size_t row = (size_t)f * nb + board;
                float* out = corners + row * n * 2;
                for (int k = lane; k < n; k += 64) {
                    const int c = W.corner_of[k];
                    out[2 * k] = c == CHARUCO_ABSENT ? NAN : (float)W.x[c], out[2 * k + 1] = c == CHARUCO_ABSENT ? NAN : (float)W.y[c];
                }
                for (int k = lane; k < sx * sy; k += 64) marker_ids[row * sx * sy + k] = W.marker_of[k];
                if (lane == 0) status_out[row] = CHARUCO_FOUND;
                for (int k = lane; k < m; k += 64)
                    if (W.flags[k] & 1) W.flags[k] = 4;
                wave_lds_fence();
                continue;
            }
            tried |= 1u << seed_board;
            for (int k = lane; k < m; k += 64)
                if (W.flags[k] & 1) W.flags[k] = 2;
            wave_lds_fence();
            if (uniform(grown == CHARUCO_SEED_TRIES * nb)) break;
        }
    }
    // 7: the boards that were not found
    for (int board = 0; board < nb; board++) {
        if (uniform((found >> board & 1) != 0)) continue;
        const size_t row = (size_t)f * nb + board;
        for (int k = lane; k < 2 * n; k += 64) corners[row * n * 2 + k] = NAN;
        for (int k = lane; k < sx * sy; k += 64) marker_ids[row * sx * sy + k] = -1;
        if (lane == 0)
            status_out[row] = frame_status != CHARUCO_NO_LATTICE ? frame_status : (tried >> board & 1) ? CHARUCO_NO_CONSENSUS : CHARUCO_NO_LATTICE;
    }
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_charuco_detect(const int* peaks, const int* counts, const uint8_t* gray, int w, int h, size_t pitch, size_t stride,
                        int frames, int squares_x, int squares_y, int marker_num, int marker_den,
                        const unsigned long long* dictionary_words, int n_ids, int s, int first_id, int min_markers,
                        int max_bit_errors, float* corners, int* marker_ids, int* status, void* queue)
{
    if (squares_x < CAMD_CHARUCO_MIN_SQUARES || squares_x > CAMD_CHARUCO_MAX_SQUARES || squares_y < CAMD_CHARUCO_MIN_SQUARES ||
        squares_y > CAMD_CHARUCO_MAX_SQUARES || s < 4 || s > 7 || n_ids < 1 || n_ids > CAMD_CHARUCO_MAX_IDS || marker_num < 1 ||
        marker_num >= marker_den || marker_den > CAMD_CHARUCO_MAX_RATIO_DEN || first_id < 0 ||
        first_id + squares_x * squares_y / 2 > n_ids || min_markers < 1 || max_bit_errors < 0 || max_bit_errors > s * s) {
        set_error("camd_charuco_detect: a board of %d x %d squares, markers of %d x %d bits and %d / %d of a square, ids %d .. of "
                  "%d, min_markers %d, max_bit_errors %d: the detector takes %d .. %d squares each way, 4 .. 7 bits, a ratio 0 < "
                  "num < den <= %d, up to %d ids that hold the board's from first_id on, min_markers >= 1, max_bit_errors 0 .. s*s",
                  squares_x, squares_y, s, s, marker_num, marker_den, first_id, n_ids, min_markers, max_bit_errors,
                  CAMD_CHARUCO_MIN_SQUARES, CAMD_CHARUCO_MAX_SQUARES, CAMD_CHARUCO_MAX_RATIO_DEN, CAMD_CHARUCO_MAX_IDS);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (w > CHARUCO_MAX_SIDE || h > CHARUCO_MAX_SIDE) {
        set_error("camd_charuco_detect: an image of %d x %d; the detector takes sides up to %d", w, h, CHARUCO_MAX_SIDE);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (!peaks || !counts || !gray || !dictionary_words || !corners || !marker_ids || !status || w < 3 || h < 3 || frames < 1 ||
        pitch < (size_t)w || (frames > 1 && stride < (size_t)(h - 1) * pitch + (size_t)w) || (uintptr_t)peaks % 4 != 0 ||
        (uintptr_t)counts % 4 != 0 || (uintptr_t)dictionary_words % 8 != 0 || (uintptr_t)corners % 4 != 0 ||
        (uintptr_t)marker_ids % 4 != 0 || (uintptr_t)status % 4 != 0) {
        set_error("camd_charuco_detect: bad arguments (peaks, counts, gray, dictionary_words, corners, marker_ids, status: device "
                  "arrays, aligned to an element; w, h >= 3, frames > 0; pitch >= w, stride >= an image)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_charuco, dim3(div_up(frames, 4)), dim3(256), 0, (hipStream_t)queue, peaks, counts, gray, w, h, pitch, stride,
                       frames, squares_x, squares_y, marker_num, marker_den, dictionary_words, n_ids, s, first_id, min_markers,
                       max_bit_errors, corners, marker_ids, status);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_charuco_detect_multi(const int* peaks, const int* counts, const uint8_t* gray, int w, int h, size_t pitch, size_t stride,
                              int frames, int squares_x, int squares_y, int marker_num, int marker_den,
                              const unsigned long long* dictionary_words, int n_ids, int s, const camd_charuco_boards* boards,
                              int min_markers, int max_bit_errors, float* corners, int* marker_ids, int* status, void* queue)
{
    if (!boards) {
        set_error("camd_charuco_detect_multi: bad arguments (boards: the set, on the host)");
        return CAMD_ERR_BAD_ARG;
    }
    const camd_charuco_boards set = *boards;
    const int markers = squares_x * squares_y / 2;
    bool set_ok = set.n >= 1 && set.n <= CAMD_CHARUCO_MAX_BOARDS;
    for (int a = 0; set_ok && a < set.n; a++) {
        set_ok = set.first_id[a] >= 0 && (long long)set.first_id[a] + markers <= n_ids;
        for (int b = 0; set_ok && b < a; b++)
            set_ok = (long long)set.first_id[a] + markers <= set.first_id[b] || (long long)set.first_id[b] + markers <= set.first_id[a];
    }
    if (squares_x < CAMD_CHARUCO_MIN_SQUARES || squares_x > CAMD_CHARUCO_MAX_SQUARES || squares_y < CAMD_CHARUCO_MIN_SQUARES ||
        squares_y > CAMD_CHARUCO_MAX_SQUARES || s < 4 || s > 7 || n_ids < 1 || n_ids > CAMD_CHARUCO_MAX_IDS || marker_num < 1 ||
        marker_num >= marker_den || marker_den > CAMD_CHARUCO_MAX_RATIO_DEN || !set_ok || min_markers < 1 || max_bit_errors < 0 ||
        max_bit_errors > s * s) {
        set_error("camd_charuco_detect_multi: %d boards of %d x %d squares, markers of %d x %d bits and %d / %d of a square, %d ids, "
                  "min_markers %d, max_bit_errors %d: the detector takes 1 .. %d boards of %d .. %d squares each way, 4 .. 7 bits, a "
                  "ratio 0 < num < den <= %d, up to %d ids that hold every board's from its first_id on in ranges apart from each "
                  "other, min_markers >= 1, max_bit_errors 0 .. s*s",
                  set.n, squares_x, squares_y, s, s, marker_num, marker_den, n_ids, min_markers, max_bit_errors,
                  CAMD_CHARUCO_MAX_BOARDS, CAMD_CHARUCO_MIN_SQUARES, CAMD_CHARUCO_MAX_SQUARES, CAMD_CHARUCO_MAX_RATIO_DEN,
                  CAMD_CHARUCO_MAX_IDS);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (w > CHARUCO_MAX_SIDE || h > CHARUCO_MAX_SIDE) {
        set_error("camd_charuco_detect_multi: an image of %d x %d; the detector takes sides up to %d", w, h, CHARUCO_MAX_SIDE);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (!peaks || !counts || !gray || !dictionary_words || !corners || !marker_ids || !status || w < 3 || h < 3 || frames < 1 ||
        pitch < (size_t)w || (frames > 1 && stride < (size_t)(h - 1) * pitch + (size_t)w) || (uintptr_t)peaks % 4 != 0 ||
        (uintptr_t)counts % 4 != 0 || (uintptr_t)dictionary_words % 8 != 0 || (uintptr_t)corners % 4 != 0 ||
        (uintptr_t)marker_ids % 4 != 0 || (uintptr_t)status % 4 != 0) {
        set_error("camd_charuco_detect_multi: bad arguments (peaks, counts, gray, dictionary_words, corners, marker_ids, status: "
                  "device arrays, aligned to an element; w, h >= 3, frames > 0; pitch >= w, stride >= an image)");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_charuco_multi, dim3(div_up(frames, 4)), dim3(256), 0, (hipStream_t)queue, peaks, counts, gray, w, h, pitch,
                       stride, frames, squares_x, squares_y, marker_num, marker_den, dictionary_words, n_ids, s, set, min_markers,
                       max_bit_errors, corners, marker_ids, status);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
