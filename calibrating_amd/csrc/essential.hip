// essential.hip -- the device side of epipolar_geometry.find_essential_matrix: a RANSAC 8-point estimator of the
// essential matrix of matched pixels, with a contract of this package's own (cv2.findEssentialMat is NOT restated:
// DESIGN.md section 2).  Three stages, each an entry of the C ABI:
//   camd_essential_hypotheses   hypothesis h draws 8 distinct matches from splitmix64 keyed by (seed, h), forms the 9 x 9
//                               normal matrix of their 8 x 9 system and takes its null vector (null_vector<9>, pnp_common.hpp)
//   camd_essential_score        the inlier count of every hypothesis over every match, and the winner
//   camd_essential_moments      for ONE matrix: the inlier mask and the 45 + 1 sums  sum a^T a, sum 1  over the inliers
// and the same three stages for MANY pairs of views in one launch each (camd_essential_batch_*, the device side of
// find_essential_matrices): the pairs' rows follow one another in two arrays, a device table names each pair's rows, its two
// inv(K) and its threshold, and host-made block tables give every workgroup ONE pair.  A pair's numbers are, bit for bit,
// the single call's: the bodies of the hypothesis, winner and moments kernels are device functions both entries call.
// What every stage computes of a match is written once, below (ess_rays, ess_row, ess_inlier): products and sums are
// individually rounded (-ffp-contract=off) in the order the source gives, so tests/essential_ref.py restates them bit for
// bit.  Integer atomics only (adds commute); the moments are reduced by the fixed-order block tree of compact.hpp.
#include "common.hpp"
#include "compact.hpp"
#include "pnp_common.hpp"

#include <cmath>

namespace camd {

constexpr int ESS_MAX_HYPOTHESES = 1 << 20;
constexpr int ESS_MAX_REDRAWS = 1024;  // of one index; beyond it (never, in practice: (7/8)^1024) the smallest free index
constexpr double ESS_NULL_PIVOT = 1e-10;  // a Cholesky pivot of M + mu I below this fraction of tr M counts as a null direction
constexpr int ESS_SCORE_ROWS = 4;  // matches a lane of the score kernel owns
constexpr int ESS_SUMS = 46;  // the packed lower triangle of sum a^T a, then the number of inliers

struct EssRows {
    const void *uv1, *uv2;  // [n][stride] of one float type; u, v are the first two of a row
    size_t n;
    int stride1, stride2;
    double k1[9], k2[9];  // inv(K1), inv(K2), row-major
};

// the rays (u, v, 1) @ inv(K).T of match i: a[r] = (k[3r] * u + k[3r + 1] * v) + k[3r + 2]
template <typename T>
__device__ __forceinline__ void ess_rays(const EssRows& m, size_t i, double* a, double* b)
{
    const T* p = (const T*)m.uv1 + i * (size_t)m.stride1;
    const T* q = (const T*)m.uv2 + i * (size_t)m.stride2;
    const double u1 = (double)p[0], v1 = (double)p[1], u2 = (double)q[0], v2 = (double)q[1];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        a[r] = (m.k1[3 * r] * u1 + m.k1[3 * r + 1] * v1) + m.k1[3 * r + 2];
        b[r] = (m.k2[3 * r] * u2 + m.k2[3 * r + 1] * v2) + m.k2[3 * r + 2];
    }
}

// the row of the 8-point system in the reference's layout [x1 x2, x2 y1, z1 x2, x1 y2, y1 y2, z1 y2, x1 z2, y1 z2, z1 z2]:
// row . e = b^T E a with E = e as 3 x 3, row-major
__device__ __forceinline__ void ess_row(const double* a, const double* b, double* r)
{
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int k = 0; k < 3; k++) r[3 * j + k] = a[k] * b[j];
}

// Is the squared Sampson error of the match below thr2?  With p = E a and q = E^T b (its first two entries):
//   p[r] = (e[3r] a0 + e[3r + 1] a1) + e[3r + 2] a2         q[c] = (e[c] b0 + e[3 + c] b1) + e[6 + c] b2
//   num = (b0 p0 + b1 p1) + b2 p2                           den = ((p0 p0 + p1 p1) + q0 q0) + q1 q1
// and the answer is num * num < thr2 * den: the quotient num^2 / den is not formed.  A zero or non-finite E (a marked
// hypothesis) and a match with den = 0 are no inliers: 0 < 0 and every comparison with NaN are false.
__device__ __forceinline__ bool ess_inlier(const double* e, const double* a, const double* b, double thr2)
{
    const double p0 = (e[0] * a[0] + e[1] * a[1]) + e[2] * a[2];
    const double p1 = (e[3] * a[0] + e[4] * a[1]) + e[5] * a[2];
    const double p2 = (e[6] * a[0] + e[7] * a[1]) + e[8] * a[2];
    const double q0 = (e[0] * b[0] + e[3] * b[1]) + e[6] * b[2];
    const double q1 = (e[1] * b[0] + e[4] * b[1]) + e[7] * b[2];
    const double num = (b[0] * p0 + b[1] * p1) + b[2] * p2;
    const double den = ((p0 * p0 + p1 * p1) + q0 * q0) + q1 * q1;
    return num * num < thr2 * den;
}

// one step of splitmix64 (boards._splitmix64)
__device__ __forceinline__ unsigned long long ess_splitmix(unsigned long long& state)
{
    state += 0x9E3779B97F4A7C15ull;
    unsigned long long z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- stage 1: one LANE per hypothesis (the 45 + 9 doubles of null_vector<9> live in its registers), a wave
// per workgroup, no barrier.  `key` = the 64 bits splitmix64 gives from the state `seed`; hypothesis h runs the stream
// whose state starts at splitmix64's output from the state key ^ h: nothing is shared between hypotheses.
template <typename T>
__device__ __forceinline__ void ess_hypothesis(const EssRows& m, unsigned long long key, int h, int* __restrict__ samples,
                                               double* __restrict__ Es)
{
    unsigned long long state = key ^ (unsigned long long)h;
    state = ess_splitmix(state);
    // index k: floor(z n / 2^64) of the next 64 bits z, drawn again from the same stream while it repeats an earlier index
    uint32_t idx[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        auto drawn = [&](uint32_t c) {
            bool dup = false;
#pragma unroll
            for (int j = 0; j < 8; j++) dup = dup || (j < k && idx[j] == c);
            return dup;
        };
        uint32_t c = 0;
        bool dup = true;
        for (int tries = 0; dup && tries < ESS_MAX_REDRAWS; tries++) {
            c = (uint32_t)__umul64hi(ess_splitmix(state), (unsigned long long)m.n);
            dup = drawn(c);
        }
        if (dup)
            for (c = 0; drawn(c); c++) {}  // (k < 8 <= n indices are taken: one of 0 .. k is free)
        idx[k] = c;
    }
    double M[45];
#pragma unroll
    for (int q = 0; q < 45; q++) M[q] = 0.;
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        uint32_t i = idx[0];
#pragma unroll
        for (int j = 1; j < 8; j++) i = j == k ? idx[j] : i;
        samples[k] = (int)i;
        double a[3], b[3], r[9];
        ess_rays<T>(m, (size_t)i, a, b);
        ess_row(a, b, r);
#pragma unroll
        for (int p = 0; p < 9; p++)
#pragma unroll
            for (int q = 0; q <= p; q++) M[p * (p + 1) / 2 + q] += r[p] * r[q];
    }
    double trace = 0.;
#pragma unroll
    for (int q = 0; q < 9; q++) trace += M[q * (q + 1) / 2 + q];
    double v[9];
    bool ok = null_vector<9>(M, v);  // leaves the Cholesky factor of M + 1e-13 tr(M) I in M
    // 8 matches in general position leave ONE null direction.  Each further one (matches that coincide, ...) shows as one
    // more pivot at the level of the shift: such a sample does not determine E and is marked
    int null_pivots = 0;
#pragma unroll
    for (int q = 0; q < 9; q++) null_pivots += M[q * (q + 1) / 2 + q] * M[q * (q + 1) / 2 + q] < ESS_NULL_PIVOT * trace ? 1 : 0;
    ok = ok && null_pivots <= 1;
    // the sign: the entry of the largest magnitude (the first of equals) is positive
    double big = v[0];
#pragma unroll
    for (int q = 1; q < 9; q++) big = fabs(v[q]) > fabs(big) ? v[q] : big;
    const bool flip = big < 0.;
#pragma unroll
    for (int q = 0; q < 9; q++) Es[q] = ok ? (flip ? -v[q] : v[q]) : 0.;  // marked: all zero, scores 0
}

template <typename T>
__global__ __launch_bounds__(64) void k_ess_hypotheses(EssRows m, unsigned long long key, int H, int* __restrict__ samples,
                                                       double* __restrict__ Es)
{
    const int h = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (h < H) ess_hypothesis<T>(m, key, h, samples + (size_t)h * 8, Es + (size_t)h * 9);
}

// ---- stage 2: a lane owns ESS_SCORE_ROWS matches (rows base + 256 r + thread of its workgroup's 1024), their rays in
// registers, and walks the hypotheses [blockIdx.y chunk, +chunk): E is wave-uniform (scalar loads), the count a ballot and
// popcount, one integer atomicAdd per (wave, hypothesis with a non-zero count).  Waves start at different hypotheses of the
// chunk, so they do not queue on one counter.
template <typename T>
__global__ __launch_bounds__(256) void k_ess_score(EssRows m, const double* __restrict__ Es, int H, int chunk, double thr2,
                                                   int* __restrict__ counts)
{
    double a[ESS_SCORE_ROWS][3], b[ESS_SCORE_ROWS][3];
#pragma unroll
    for (int r = 0; r < ESS_SCORE_ROWS; r++) {
        const size_t i = (size_t)blockIdx.x * (256 * ESS_SCORE_ROWS) + 256 * r + threadIdx.x;
#pragma unroll
        for (int q = 0; q < 3; q++) a[r][q] = b[r][q] = 0.;  // a row beyond n: zero rays, den = 0, never an inlier
        if (i < m.n) ess_rays<T>(m, i, a[r], b[r]);
    }
    const int h0 = (int)blockIdx.y * chunk, span = (H - h0 < chunk ? H - h0 : chunk);
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const int first = (int)((wave * 7u) % (unsigned)span);
    for (int j = 0; j < span; j++) {
        const int h = h0 + (first + j < span ? first + j : first + j - span);
        const double* __restrict__ E = Es + (size_t)h * 9;
        double e[9];
#pragma unroll
        for (int q = 0; q < 9; q++) e[q] = E[q];
        int c = 0;
#pragma unroll
        for (int r = 0; r < ESS_SCORE_ROWS; r++) c += __popcll(__ballot(ess_inlier(e, a[r], b[r], thr2)));
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(counts + h, c);
    }
}

// the largest count, ties to the lowest index: winner[0 .. 8] = its E, winner[9] = its index, winner[10] = its count
__device__ __forceinline__ void ess_winner(const int* __restrict__ counts, const double* __restrict__ Es, int H,
                                           double* __restrict__ winner, unsigned long long* sh)
{
    unsigned long long best = 0;  // (every key of a hypothesis is above 0: its low word is 2^32 - 1 - h)
    for (int h = threadIdx.x; h < H; h += 256) {
        const unsigned long long key = ((unsigned long long)(uint32_t)counts[h] << 32) | (0xffffffffu - (uint32_t)h);
        best = key > best ? key : best;
    }
    sh[threadIdx.x] = best;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = sh[threadIdx.x + o] > sh[threadIdx.x] ? sh[threadIdx.x + o] : sh[threadIdx.x];
        __syncthreads();
    }
    const uint32_t h = 0xffffffffu - (uint32_t)sh[0];
    if (threadIdx.x < 9) winner[threadIdx.x] = Es[(size_t)h * 9 + threadIdx.x];
    if (threadIdx.x == 9) winner[9] = (double)h;
    if (threadIdx.x == 10) winner[10] = (double)(uint32_t)(sh[0] >> 32);
}

__global__ __launch_bounds__(256) void k_ess_winner(const int* __restrict__ counts, const double* __restrict__ Es, int H,
                                                    double* __restrict__ winner)
{
    __shared__ unsigned long long sh[256];
    ess_winner(counts, Es, H, winner, sh);
}

// ---- stage 3: mask[i] and, over the inliers, s[p (p + 1) / 2 + q] += row[p] * row[q] (q <= p), s[45] += 1.  The shape of
// k_ep_pose_partials: thread t of workgroup g takes rows g 256 + t, + 256 G, ... in that order; block_tree; k_ep_final.
// Workgroup g of the G that share the rows of `m`; dst: the workgroup's ESS_SUMS partials; sh: __shared__ double[256].
template <typename T>
__device__ __forceinline__ void ess_moments(const EssRows& m, int g, int G, const double* __restrict__ E, double thr2,
                                            uint8_t* __restrict__ mask, double* __restrict__ dst, double* sh)
{
    double s[ESS_SUMS], e[9];
#pragma unroll
    for (int q = 0; q < ESS_SUMS; q++) s[q] = 0.;
#pragma unroll
    for (int q = 0; q < 9; q++) e[q] = E[q];
    for (size_t i = (size_t)g * 256 + threadIdx.x; i < m.n; i += (size_t)G * 256) {
        double a[3], b[3], r[9];
        ess_rays<T>(m, i, a, b);
        const bool on = ess_inlier(e, a, b, thr2);
        mask[i] = on ? 1 : 0;
        if (!on) continue;
        ess_row(a, b, r);
#pragma unroll
        for (int p = 0; p < 9; p++)
#pragma unroll
            for (int q = 0; q <= p; q++) s[p * (p + 1) / 2 + q] += r[p] * r[q];
        s[45] += 1.;
    }
    block_tree<ESS_SUMS>(s, sh, dst);
}

template <typename T>
__global__ __launch_bounds__(256) void k_ess_moments(EssRows m, const double* __restrict__ E, double thr2, uint8_t* __restrict__ mask,
                                                     double* __restrict__ partials)
{
    __shared__ double sh[256];
    ess_moments<T>(m, (int)blockIdx.x, (int)gridDim.x, E, thr2, mask, partials + (size_t)blockIdx.x * ESS_SUMS, sh);
}

// ---- the batch: many pairs, one launch a stage ----------------------------------------------------------------------------
// pair p's record, ESS_PAIR_DOUBLES doubles of the device table: [0], [1] = its first row and its number of rows (int64 bit
// patterns), [2 .. 10] = inv(K) of the view uv_a shows, [11 .. 19] = of the view uv_b shows, [20] = its threshold2
constexpr int ESS_PAIR_DOUBLES = 21;

struct EssBatch {
    const void *uv_a, *uv_b;  // [m][stride] of one float type: the pairs' rows one after the other
    const double* table;      // [pairs][ESS_PAIR_DOUBLES], on the device
    size_t m;
    int stride_a, stride_b, pairs;
};

// the rows of pair p as the single call's kernels take them; false (and no rows) when the record leaves the arrays
template <typename T>
__device__ __forceinline__ bool ess_pair_rows(const EssBatch& B, int p, EssRows* m, double* thr2, size_t* first_row = nullptr)
{
    m->n = 0;
    if ((unsigned)p >= (unsigned)B.pairs) return false;
    const double* rec = B.table + (size_t)p * ESS_PAIR_DOUBLES;
    const unsigned long long first = (unsigned long long)__double_as_longlong(rec[0]), n = (unsigned long long)__double_as_longlong(rec[1]);
    if (first > B.m || n > B.m - first) return false;
    m->uv1 = (const T*)B.uv_a + first * (size_t)B.stride_a;
    m->uv2 = (const T*)B.uv_b + first * (size_t)B.stride_b;
    m->n = n, m->stride1 = B.stride_a, m->stride2 = B.stride_b;
#pragma unroll
    for (int q = 0; q < 9; q++) m->k1[q] = rec[2 + q], m->k2[q] = rec[11 + q];
    *thr2 = rec[20];
    if (first_row) *first_row = (size_t)first;
    return true;
}

// one lane per (pair, hypothesis): workgroup b of the grid is the b % hblocks-th 64 hypotheses of pair b / hblocks.  A pair of
// fewer than 8 rows draws nothing: its samples are -1 and its matrices zero.
template <typename T>
__global__ __launch_bounds__(64) void k_ess_hypotheses_batch(EssBatch B, unsigned long long key, int H, int hblocks,
                                                             int* __restrict__ samples, double* __restrict__ Es)
{
    const int p = (int)(blockIdx.x / (unsigned)hblocks), h = (int)(blockIdx.x % (unsigned)hblocks) * 64 + (int)threadIdx.x;
    if (h >= H || p >= B.pairs) return;
    int* sm = samples + ((size_t)p * H + h) * 8;
    double* E = Es + ((size_t)p * H + h) * 9;
    EssRows m;
    double thr2;
    if (!ess_pair_rows<T>(B, p, &m, &thr2) || m.n < 8) {
        for (int k = 0; k < 8; k++) sm[k] = -1;
        for (int q = 0; q < 9; q++) E[q] = 0.;
        return;
    }
    ess_hypothesis<T>(m, key, h, sm, E);
}

// blocks[b] = (pair, g, G, -): workgroup b owns rows 1024 g .. 1024 g + 1023 of ONE pair (the score), or is workgroup g of the
// G that sum the pair's moments.  LDS_SUM: the four waves add their counts of a hypothesis in LDS, 256 hypotheses at a time,
// and the workgroup issues ONE global atomicAdd per hypothesis with a non-zero count; otherwise one per wave, as k_ess_score.
template <typename T, bool LDS_SUM>
__global__ __launch_bounds__(256) void k_ess_score_batch(EssBatch B, const int4* __restrict__ blocks, const double* __restrict__ Es, int H,
                                                         int chunk, int* __restrict__ counts)
{
    __shared__ int tile[256];
    const int4 blk = blocks[blockIdx.x];
    EssRows m;
    double thr2;
    if (!ess_pair_rows<T>(B, blk.x, &m, &thr2) || blk.y < 0) return;  // (uniform: before any barrier)
    double a[ESS_SCORE_ROWS][3], b[ESS_SCORE_ROWS][3];
#pragma unroll
    for (int r = 0; r < ESS_SCORE_ROWS; r++) {
        const size_t i = (size_t)blk.y * (256 * ESS_SCORE_ROWS) + 256 * r + threadIdx.x;
#pragma unroll
        for (int q = 0; q < 3; q++) a[r][q] = b[r][q] = 0.;
        if (i < m.n) ess_rays<T>(m, i, a[r], b[r]);
    }
    Es += (size_t)blk.x * H * 9;
    counts += (size_t)blk.x * H;
    const int h0 = (int)blockIdx.y * chunk, span = (H - h0 < chunk ? H - h0 : chunk);
    const unsigned wave_here = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (LDS_SUM) {
        for (int t0 = 0; t0 < span; t0 += 256) {
            const int tn = span - t0 < 256 ? span - t0 : 256;
            tile[threadIdx.x] = 0;
            __syncthreads();
            const int first = (int)((wave_here * 64u) % (unsigned)tn);
            for (int j = 0; j < tn; j++) {
                const int k = first + j < tn ? first + j : first + j - tn;
                const double* __restrict__ E = Es + (size_t)(h0 + t0 + k) * 9;
                double e[9];
#pragma unroll
                for (int q = 0; q < 9; q++) e[q] = E[q];
                int c = 0;
#pragma unroll
                for (int r = 0; r < ESS_SCORE_ROWS; r++) c += __popcll(__ballot(ess_inlier(e, a[r], b[r], thr2)));
                if ((threadIdx.x & 63) == 0 && c) atomicAdd(tile + k, c);
            }
            __syncthreads();
            if ((int)threadIdx.x < tn && tile[threadIdx.x]) atomicAdd(counts + h0 + t0 + threadIdx.x, tile[threadIdx.x]);
            __syncthreads();
        }
    } else {
        const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
        const int first = (int)((wave * 7u) % (unsigned)span);
        for (int j = 0; j < span; j++) {
            const int h = h0 + (first + j < span ? first + j : first + j - span);
            const double* __restrict__ E = Es + (size_t)h * 9;
            double e[9];
#pragma unroll
            for (int q = 0; q < 9; q++) e[q] = E[q];
            int c = 0;
#pragma unroll
            for (int r = 0; r < ESS_SCORE_ROWS; r++) c += __popcll(__ballot(ess_inlier(e, a[r], b[r], thr2)));
            if ((threadIdx.x & 63) == 0 && c) atomicAdd(counts + h, c);
        }
    }
}

// one workgroup per pair: winner[p] = the 11 doubles of k_ess_winner over the pair's counts
__global__ __launch_bounds__(256) void k_ess_winner_batch(const int* __restrict__ counts, const double* __restrict__ Es, int H,
                                                          double* __restrict__ winner)
{
    __shared__ unsigned long long sh[256];
    const size_t p = blockIdx.x;
    ess_winner(counts + p * H, Es + p * H * 9, H, winner + p * 11, sh);
}

// workgroup b = workgroup blocks[b].y of the blocks[b].z of its pair; its partials are the b-th of partials; the pair's matrix
// is E[pair * E_stride ..]; mask is the one [m] array
template <typename T>
__global__ __launch_bounds__(256) void k_ess_moments_batch(EssBatch B, const int4* __restrict__ blocks, const double* __restrict__ E,
                                                           int E_stride, uint8_t* __restrict__ mask, double* __restrict__ partials)
{
    __shared__ double sh[256];
    const int4 blk = blocks[blockIdx.x];
    EssRows m;
    double thr2;
    size_t first;
    if (!ess_pair_rows<T>(B, blk.x, &m, &thr2, &first) || blk.y < 0 || blk.z < 1 || blk.y >= blk.z) return;
    ess_moments<T>(m, blk.y, blk.z, E + (size_t)blk.x * E_stride, thr2, mask + first, partials + (size_t)blockIdx.x * ESS_SUMS, sh);
}

// finals[f] = (pair, its first workgroup of the moments launch, their number G, -): sums[pair] = k_ep_final over its partials
__global__ __launch_bounds__(256) void k_ess_final_batch(const int4* __restrict__ finals, int pairs, int blocks,
                                                         const double* __restrict__ partials, double* __restrict__ sums)
{
    __shared__ double sh[256];
    const int4 f = finals[blockIdx.x];
    if ((unsigned)f.x >= (unsigned)pairs || f.y < 0 || f.z < 1 || f.z > SUM_MAX_BLOCKS || f.y > blocks - f.z) return;
    ep_final<ESS_SUMS>(partials + (size_t)f.y * ESS_SUMS, f.z, sums + (size_t)f.x * ESS_SUMS, sh);
}

static int make_rows(EssRows* m, const char* who, const void* uv1, const void* uv2, int uv_type, size_t n, int uv1_stride,
                     int uv2_stride, const double* K1inv, const double* K2inv)
{
    const size_t elem = uv_type == CAMD_VALUE_F64 ? 8 : 4;
    if (!uv1 || !uv2 || !K1inv || !K2inv || !float_type_ok(uv_type) || n < 8 || (unsigned long long)n > 0x7fffffffull ||
        uv1_stride < 2 || uv2_stride < 2 || (uintptr_t)uv1 % elem || (uintptr_t)uv2 % elem) {
        set_error("%s: bad arguments (uv1, uv2: [n][stride >= 2] of CAMD_VALUE_F64 or _F32, aligned to an element; 8 <= n < 2^31, "
                  "got %zu; K1inv, K2inv: 9 host doubles)", who, n);
        return CAMD_ERR_BAD_ARG;
    }
    m->uv1 = uv1, m->uv2 = uv2, m->n = n, m->stride1 = uv1_stride, m->stride2 = uv2_stride;
    for (int q = 0; q < 9; q++) {
        m->k1[q] = K1inv[q], m->k2[q] = K2inv[q];
        if (!std::isfinite(K1inv[q]) || !std::isfinite(K2inv[q])) {
            set_error("%s: K1inv, K2inv must be finite", who);
            return CAMD_ERR_BAD_ARG;
        }
    }
    return CAMD_OK;
}

static bool hypotheses_ok(int H) { return H >= 1 && H <= ESS_MAX_HYPOTHESES; }

}  // namespace camd

using namespace camd;

extern "C" {

int camd_essential_hypotheses(const void* uv1, const void* uv2, int uv_type, size_t n, int uv1_stride, int uv2_stride,
                              const double K1inv[9], const double K2inv[9], unsigned long long seed, int hypotheses, int* samples,
                              double* Es, void* queue)
{
    EssRows m;
    const int rc = make_rows(&m, "camd_essential_hypotheses", uv1, uv2, uv_type, n, uv1_stride, uv2_stride, K1inv, K2inv);
    if (rc != CAMD_OK) return rc;
    if (!hypotheses_ok(hypotheses) || !samples || !doubles_ok(Es)) {
        set_error("camd_essential_hypotheses: 1 .. 2^20 hypotheses, samples and Es (aligned) are required, got %d", hypotheses);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    unsigned long long state = seed, key;
    state += 0x9E3779B97F4A7C15ull;
    key = state;
    key = (key ^ (key >> 30)) * 0xBF58476D1CE4E5B9ull;
    key = (key ^ (key >> 27)) * 0x94D049BB133111EBull;
    key ^= key >> 31;
    with_float(uv_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_ess_hypotheses<T>), dim3(div_up(hypotheses, 64)), dim3(64), 0, (hipStream_t)queue, m, key, hypotheses,
                           samples, Es);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_essential_score(const void* uv1, const void* uv2, int uv_type, size_t n, int uv1_stride, int uv2_stride,
                         const double K1inv[9], const double K2inv[9], const double* Es, int hypotheses, double threshold2,
                         int* counts, double* winner, void* queue)
{
    EssRows m;
    const int rc = make_rows(&m, "camd_essential_score", uv1, uv2, uv_type, n, uv1_stride, uv2_stride, K1inv, K2inv);
    if (rc != CAMD_OK) return rc;
    if (!hypotheses_ok(hypotheses) || !doubles_ok(Es) || !counts || !doubles_ok(winner) || !(threshold2 > 0.) ||
        !std::isfinite(threshold2)) {
        set_error("camd_essential_score: 1 .. 2^20 hypotheses, a positive finite threshold2, Es, counts and winner are required");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    // the matches give the grid's x, 1024 a workgroup; while that leaves the chip idle the hypotheses are split over y
    const int gx = div_up((long long)n, 256 * ESS_SCORE_ROWS);
    int gy = div_up(2048, gx);
    const int most = div_up(hypotheses, 16) < 65535 ? div_up(hypotheses, 16) : 65535;
    gy = gy < 1 ? 1 : gy > most ? most : gy;
    const int chunk = div_up(hypotheses, gy);
    gy = div_up(hypotheses, chunk);
    fill((uint32_t*)counts, (size_t)hypotheses, 0u, nullptr, st);
    with_float(uv_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_ess_score<T>), dim3(gx, gy), dim3(256), 0, st, m, Es, hypotheses, chunk, threshold2, counts);
    });
    hipLaunchKernelGGL(k_ess_winner, dim3(1), dim3(256), 0, st, counts, Es, hypotheses, winner);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_essential_moments_blocks(size_t n) { return sum_blocks(n); }

int camd_essential_moments(const void* uv1, const void* uv2, int uv_type, size_t n, int uv1_stride, int uv2_stride,
                           const double K1inv[9], const double K2inv[9], const double* E, double threshold2, uint8_t* mask,
                           double* partials_ws, double* sums, void* queue)
{
    EssRows m;
    const int rc = make_rows(&m, "camd_essential_moments", uv1, uv2, uv_type, n, uv1_stride, uv2_stride, K1inv, K2inv);
    if (rc != CAMD_OK) return rc;
    if (!doubles_ok(E) || !mask || !doubles_ok(partials_ws) || !doubles_ok(sums) || !(threshold2 > 0.) || !std::isfinite(threshold2)) {
        set_error("camd_essential_moments: a positive finite threshold2, E, mask, partials_ws and sums are required");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    const int g = sum_blocks(n);
    with_float(uv_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_ess_moments<T>), dim3(g), dim3(256), 0, st, m, E, threshold2, mask, partials_ws);
    });
    hipLaunchKernelGGL((k_ep_final<ESS_SUMS>), dim3(1), dim3(256), 0, st, partials_ws, g, sums);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

static int make_batch(EssBatch* B, const char* who, const void* uv_a, const void* uv_b, int uv_type, size_t m, int stride_a,
                      int stride_b, const double* pair_table, int pairs)
{
    const size_t elem = uv_type == CAMD_VALUE_F64 ? 8 : 4;
    if (!uv_a || !uv_b || !float_type_ok(uv_type) || m < 1 || (unsigned long long)m > 0x7fffffffull || stride_a < 2 || stride_b < 2 ||
        (uintptr_t)uv_a % elem || (uintptr_t)uv_b % elem || !doubles_ok(pair_table) || pairs < 1) {
        set_error("%s: bad arguments (uv_a, uv_b: [m][stride >= 2] of CAMD_VALUE_F64 or _F32, aligned to an element; 1 <= m < 2^31, "
                  "got %zu; pair_table: [pairs >= 1][21] device doubles, got %d pairs)", who, m, pairs);
        return CAMD_ERR_BAD_ARG;
    }
    B->uv_a = uv_a, B->uv_b = uv_b, B->table = pair_table, B->m = m, B->stride_a = stride_a, B->stride_b = stride_b, B->pairs = pairs;
    return CAMD_OK;
}

int camd_essential_batch_hypotheses(const void* uv_a, const void* uv_b, int uv_type, size_t m, int uv_a_stride, int uv_b_stride,
                                    const double* pair_table, int pairs, unsigned long long seed, int hypotheses, int* samples,
                                    double* Es, void* queue)
{
    EssBatch B;
    const int rc = make_batch(&B, "camd_essential_batch_hypotheses", uv_a, uv_b, uv_type, m, uv_a_stride, uv_b_stride, pair_table, pairs);
    if (rc != CAMD_OK) return rc;
    if (!hypotheses_ok(hypotheses) || !samples || !doubles_ok(Es)) {
        set_error("camd_essential_batch_hypotheses: 1 .. 2^20 hypotheses, samples and Es (aligned) are required, got %d", hypotheses);
        return CAMD_ERR_BAD_ARG;
    }
    const int hblocks = div_up(hypotheses, 64);
    if ((long long)hblocks * pairs > 0x7fffffffll) {
        set_error("camd_essential_batch_hypotheses: %d pairs of %d hypotheses exceed the grid", pairs, hypotheses);
        return CAMD_ERR_UNSUPPORTED;
    }
    CAMD_NEED_DEVICE();
    unsigned long long state = seed, key;
    state += 0x9E3779B97F4A7C15ull;
    key = state;
    key = (key ^ (key >> 30)) * 0xBF58476D1CE4E5B9ull;
    key = (key ^ (key >> 27)) * 0x94D049BB133111EBull;
    key ^= key >> 31;
    with_float(uv_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_ess_hypotheses_batch<T>), dim3((unsigned)(hblocks * pairs)), dim3(64), 0, (hipStream_t)queue, B, key,
                           hypotheses, hblocks, samples, Es);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_essential_batch_score(const void* uv_a, const void* uv_b, int uv_type, size_t m, int uv_a_stride, int uv_b_stride,
                               const double* pair_table, int pairs, const int* block_table, int blocks, const double* Es,
                               int hypotheses, int lds_sum, int* counts, double* winner, void* queue)
{
    EssBatch B;
    const int rc = make_batch(&B, "camd_essential_batch_score", uv_a, uv_b, uv_type, m, uv_a_stride, uv_b_stride, pair_table, pairs);
    if (rc != CAMD_OK) return rc;
    if (!hypotheses_ok(hypotheses) || !doubles_ok(Es) || !counts || !doubles_ok(winner) || !block_table || (uintptr_t)block_table % 16 ||
        blocks < 1 || (unsigned long long)pairs * (unsigned long long)hypotheses > 0x7fffffffull) {
        set_error("camd_essential_batch_score: 1 .. 2^20 hypotheses (pairs * hypotheses < 2^31), block_table ([blocks >= 1][4] int32, "
                  "16-aligned), Es, counts and winner are required");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    // as camd_essential_score: the rows give the grid's x; while that leaves the chip idle the hypotheses are split over y
    int gy = div_up(2048, blocks);
    const int most = div_up(hypotheses, 16) < 65535 ? div_up(hypotheses, 16) : 65535;
    gy = gy < 1 ? 1 : gy > most ? most : gy;
    const int chunk = div_up(hypotheses, gy);
    gy = div_up(hypotheses, chunk);
    fill((uint32_t*)counts, (size_t)pairs * hypotheses, 0u, nullptr, st);
    with_float(uv_type, [&](auto v) {
        using T = decltype(v);
        if (lds_sum)
            hipLaunchKernelGGL((k_ess_score_batch<T, true>), dim3(blocks, gy), dim3(256), 0, st, B, (const int4*)block_table, Es,
                               hypotheses, chunk, counts);
        else
            hipLaunchKernelGGL((k_ess_score_batch<T, false>), dim3(blocks, gy), dim3(256), 0, st, B, (const int4*)block_table, Es,
                               hypotheses, chunk, counts);
    });
    hipLaunchKernelGGL(k_ess_winner_batch, dim3(pairs), dim3(256), 0, st, counts, Es, hypotheses, winner);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_essential_batch_moments(const void* uv_a, const void* uv_b, int uv_type, size_t m, int uv_a_stride, int uv_b_stride,
                                 const double* pair_table, int pairs, const int* block_table, int blocks, const int* final_table,
                                 int finals, const double* E, int E_stride, uint8_t* mask, double* partials_ws, double* sums,
                                 void* queue)
{
    EssBatch B;
    const int rc = make_batch(&B, "camd_essential_batch_moments", uv_a, uv_b, uv_type, m, uv_a_stride, uv_b_stride, pair_table, pairs);
    if (rc != CAMD_OK) return rc;
    if (!doubles_ok(E) || E_stride < 9 || !mask || !doubles_ok(partials_ws) || !doubles_ok(sums) || !block_table || !final_table ||
        (uintptr_t)block_table % 16 || (uintptr_t)final_table % 16 || blocks < 1 || finals < 1 || finals > pairs) {
        set_error("camd_essential_batch_moments: E ([pairs][E_stride >= 9]), mask, partials_ws, sums, block_table ([blocks >= 1][4]) and "
                  "final_table ([1 .. pairs][4], both int32 and 16-aligned) are required");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    with_float(uv_type, [&](auto v) {
        using T = decltype(v);
        hipLaunchKernelGGL((k_ess_moments_batch<T>), dim3(blocks), dim3(256), 0, st, B, (const int4*)block_table, E, E_stride, mask,
                           partials_ws);
    });
    hipLaunchKernelGGL(k_ess_final_batch, dim3(finals), dim3(256), 0, st, (const int4*)final_table, pairs, blocks, partials_ws, sums);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
