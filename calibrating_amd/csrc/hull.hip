// hull.hip -- sparse (u, v, z) samples filled by their least-squares plane INSIDE their convex hull only, batched over
// frames: the operation behind the reference's interpolate_uvzs(..., constrained_type="convex_hull") (utils.py:356-415),
// which Cam.get_calibration_board_depth (camera.py:234-251) and MatchingByBoard (stereo_matching.py:73-110) rest on.
//
// The mask has a contract of its OWN (UNPINNED against cv2.convexHull / cv2.drawContours,
// DESIGN.md section 2, U33): pixel (x, y) is inside iff the integer point lies in the closed convex hull of the valid
// samples' rounded pixels.  Everything that decides the mask is an integer: int64 cross products for the hull, int64
// floor / ceil divisions for the row spans.  No floating point enters it.
//
// Stage A (k_hull_fit): one wavefront per frame and NO workgroup barrier, as pnp.hip and subpix.hip.  The frame's rounded
// pixels live in the wave's LDS; the hull is gift-wrapped, each step a lane-strided scan plus an xor butterfly under a
// total order, so the vertex set does not depend on which lane saw which row; the nine plane sums are added lane-strided
// in rising row order and meet in the butterfly of pnp_common.hpp (no float atomics); every lane solves the 3 x 3 system
// by the centred moments.  A frame's record depends on nothing but its own rows: alone or anywhere in a batch, the
// same bits.  Stage B (k_hull_fill): one wavefront per image row, the row's closed span from the hull's edges, every
// pixel written exactly once, 16 bytes per lane where the row's address allows.
#include "hull_common.hpp"
#include "pnp_common.hpp"

namespace camd {

constexpr double HULL_COLLINEAR_TOL = 1e-9;    // sparse.COLLINEAR_TOL
constexpr int HULL_DROPPED = INT_MIN;          // px of a row that takes no part

struct HullFitArgs {
    const double* uv;
    const void* z;  // null: every z counts as 1 (the mask alone)
    const long long* start;
    int* vertices;
    int* hull_counts;
    double* abc;
    int* status;
    unsigned long long rows;
    unsigned per_frame;
    int uv_stride, z_type, frames, w, h, keep_last, capacity;
};

struct HullPoint {
    int x, y;  // x == HULL_DROPPED: none
};

// is r the better next vertex than q, seen from the hull vertex p?  The sign of the cross product, then the larger
// squared distance among collinear candidates: a total order on the points other than p (they lie within a half turn).
__device__ __forceinline__ bool hull_better(const HullPoint& p, const HullPoint& q, const HullPoint& r)
{
    if (r.x == HULL_DROPPED) return false;
    if (q.x == HULL_DROPPED) return true;
    const long long qx = (long long)q.x - p.x, qy = (long long)q.y - p.y, rx = (long long)r.x - p.x, ry = (long long)r.y - p.y;
    const long long c = qx * ry - qy * rx;
    if (c != 0) return c < 0;
    return rx * rx + ry * ry > qx * qx + qy * qy;
}

__device__ __forceinline__ HullPoint hull_shuffle(const HullPoint& a, int m)
{
    HullPoint o;
    o.x = __shfl_xor(a.x, m, 64), o.y = __shfl_xor(a.y, m, 64);
    return o;
}

template <typename Z>
__global__ __launch_bounds__(64) void k_hull_fit(HullFitArgs a)
{
    extern __shared__ int hull_lds[];  // capacity x, then capacity y
    int* px = hull_lds;
    int* py = hull_lds + a.capacity;
    const int lane = threadIdx.x, f = blockIdx.x;
    if (f >= a.frames) return;
    int* verts = a.vertices + (size_t)f * a.capacity * 2;

    // the frame's rows; a range that is not inside the rows or longer than the capacity is read nowhere
    long long s, e;
    if (a.start) s = a.start[f], e = a.start[f + 1];
    else s = (long long)f * a.per_frame, e = s + a.per_frame;
    int n = 0;
    if (s >= 0 && e >= s && (unsigned long long)e <= a.rows && e - s <= (long long)a.capacity) n = (int)(e - s);
    const double* uv = a.uv + (size_t)s * a.uv_stride;
    const Z* z = a.z ? (const Z*)a.z + (size_t)s : nullptr;

    // 1. validate and round
    int status = 0;
    for (int i = lane; i < n; i += 64) {
        const double u = uv[(size_t)i * a.uv_stride], v = uv[(size_t)i * a.uv_stride + 1], zz = z ? (double)z[i] : 1.;
        int x = HULL_DROPPED, y = 0;
        if (isfinite(u) && isfinite(v) && isfinite(zz) && zz != 0.) {
            const double ru = rint(u), rv = rint(v);
            if (fabs(ru) <= HULL_MAX_COORD && fabs(rv) <= HULL_MAX_COORD) {
                x = (int)ru, y = (int)rv;
                if (a.keep_last && !(x >= 0 && x < a.w && y >= 0 && y < a.h)) x = HULL_DROPPED;  // the scatter drops it
            } else {
                status |= HULL_OUT_OF_RANGE;
            }
        }
        px[i] = x, py[i] = y;
    }
    status = wave_or(status);
    wave_lds_fence();

    // 2. of several rows on one pixel the last one stays (the scatter's rule).  A lane owns at most 64 rows: one bit each
    if (a.keep_last) {
        unsigned long long drop = 0;
        int k = 0;
        for (int i = lane; i < n; i += 64, k++) {
            const int x = px[i], y = py[i];
            if (x == HULL_DROPPED) continue;
            for (int j = i + 1; j < n; j++)
                if (px[j] == x && py[j] == y) {
                    drop |= 1ull << k;
                    break;
                }
        }
        wave_lds_fence();  // every lane has read before any lane writes
        k = 0;
        for (int i = lane; i < n; i += 64, k++)
            if (drop >> k & 1) px[i] = HULL_DROPPED;
        wave_lds_fence();
    }

    // 3. the nine sums of sparse._fit_plane over the rows that take part, from the unrounded float64 samples
    double sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    HullPoint first = {HULL_DROPPED, 0};
    for (int i = lane; i < n; i += 64) {
        if (px[i] == HULL_DROPPED) continue;
        const double u = uv[(size_t)i * a.uv_stride], v = uv[(size_t)i * a.uv_stride + 1], zz = z ? (double)z[i] : 1.;
        sum[0] += u * u; sum[1] += u * v; sum[2] += u;
        sum[3] += v * v; sum[4] += v;     sum[5] += 1.0;
        sum[6] += u * zz; sum[7] += v * zz; sum[8] += zz;
        if (first.x == HULL_DROPPED || px[i] < first.x || (px[i] == first.x && py[i] < first.y)) first = {px[i], py[i]};
    }
    wave_sum_all<9>(sum);
    const double cnt = sum[5];

    // 4. the plane: the normal equations through the centred second moments, as sparse._fit_plane solves them
    double A = NAN, B = NAN, C = NAN;
    int count = 0;
    if (uniform(cnt == 0.)) {
        status |= HULL_NO_SAMPLE;
    } else {
        const double su = sum[2], sv = sum[4], sz = sum[8];
        const double mu = su / cnt, mv = sv / cnt, mz = sz / cnt;
        const double cuu = sum[0] - su * mu, cvv = sum[3] - sv * mv, cuv = sum[1] - su * mv;
        const double cuz = sum[6] - su * mz, cvz = sum[7] - sv * mz;
        const double det = cuu * cvv - cuv * cuv;
        if (cnt < 3. || !(det > HULL_COLLINEAR_TOL * cuu * cvv)) {
            status |= HULL_DEGENERATE;
        } else {
            A = (cuz * cvv - cvz * cuv) / det;
            B = (cvz * cuu - cuz * cuv) / det;
            C = mz - A * mu - B * mv;
        }

        // 5. the hull.  Start: the lowest (x, y), a vertex for certain; then wrap until the start comes round again.
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const HullPoint o = hull_shuffle(first, m);
            if (o.x != HULL_DROPPED && (first.x == HULL_DROPPED || o.x < first.x || (o.x == first.x && o.y < first.y))) first = o;
        }
        HullPoint p = first;
        const int most = n < a.capacity ? n : a.capacity;  // a hull has no more vertices than the frame has rows
        while (count < most) {
            if (lane == 0) verts[count * 2] = p.x, verts[count * 2 + 1] = p.y;
            count++;
            HullPoint best = {HULL_DROPPED, 0};
            for (int i = lane; i < n; i += 64) {
                const HullPoint r = {px[i], py[i]};
                if (r.x == HULL_DROPPED || (r.x == p.x && r.y == p.y)) continue;
                if (hull_better(p, best, r)) best = r;
            }
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const HullPoint o = hull_shuffle(best, m);
                if (hull_better(p, best, o)) best = o;
            }
            if (uniform(best.x == HULL_DROPPED || (best.x == first.x && best.y == first.y))) break;
            p = best;
        }
    }
    if (lane == 0) {
        a.hull_counts[f] = count;
        a.status[f] = status;
        a.abc[(size_t)f * 3] = A, a.abc[(size_t)f * 3 + 1] = B, a.abc[(size_t)f * 3 + 2] = C;
    }
}

// ---- stage B ---------------------------------------------------------------------------------------------------------
// (the closed span of a row inside the hull, hull_span, lives in hull_common.hpp: lidar.hip fills by it too)
struct HullPlane {  // the value: exactly k_sp_plane_eval's expression (sparse.hip); 1 / that with `reciprocal`
    double a, b, c;
    int reciprocal, zero;  // zero: the whole frame is 0, whatever `reciprocal` says
    typedef float Px;
    __device__ __forceinline__ float operator()(int x, int y, bool inside) const
    {
        if (zero) return 0.0f;
        float v = 0.0f;
        if (inside) v = (float)__fma_rn(1.0, c, __fma_rn((double)y, b, __dmul_rn((double)x, a)));
        return reciprocal ? __fdiv_rn(1.0f, v) : v;
    }
};

struct HullMask {
    typedef uint8_t Px;
    __device__ __forceinline__ uint8_t operator()(int, int, bool inside) const { return inside ? 1 : 0; }
};

constexpr int HULL_ROWS_PER_WAVE = 2;
constexpr int HULL_ROWS_PER_GROUP = 4 * HULL_ROWS_PER_WAVE;

// One wavefront per row, HULL_ROWS_PER_WAVE rows after one another; the group's waves share nothing.  A row is written
// as a scalar head up to the first 16-byte boundary, a body of whole 16-byte vectors, one per lane and round, and a
// scalar tail.  `aligned`: the image's base is 16-byte aligned (else everything is head).
template <typename V>
__global__ __launch_bounds__(256) void k_hull_fill(const int* __restrict__ vertices, const int* __restrict__ hull_counts,
                                                   const double* __restrict__ abc, int capacity, int frames, int w, int h,
                                                   int tiles, int reciprocal, const uint8_t* __restrict__ zero_frames,
                                                   int aligned, typename V::Px* __restrict__ out)
{
    typedef typename V::Px Px;
    constexpr int N = 16 / (int)sizeof(Px);
    struct alignas(16) Vec { Px v[N]; };
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    if (f >= frames) return;
    const int* verts = vertices + (size_t)f * capacity * 2;
    int count = hull_counts[f];
    count = count < 0 ? 0 : (count > capacity ? capacity : count);
    V value;
    if constexpr (sizeof(Px) == 4) {
        value.a = abc[(size_t)f * 3], value.b = abc[(size_t)f * 3 + 1], value.c = abc[(size_t)f * 3 + 2];
        value.reciprocal = reciprocal, value.zero = zero_frames && zero_frames[f] ? 1 : 0;
    }
    for (int r = 0; r < HULL_ROWS_PER_WAVE; r++) {
        const int y = tile * HULL_ROWS_PER_GROUP + wave * HULL_ROWS_PER_WAVE + r;
        if (y >= h) return;  // (the whole wave)
        int xl, xr;
        hull_span(verts, count, y, w, lane, &xl, &xr);
        const size_t base = ((size_t)f * h + y) * (size_t)w;
        Px* row = out + base;
        int head = aligned ? (int)((N - (base % N)) % N) : w;
        if (head > w) head = w;
        const int body = (w - head) / N;
        for (int x = lane; x < head; x += 64) row[x] = value(x, y, x >= xl && x <= xr);
        for (int q = lane; q < body; q += 64) {
            const int x0 = head + q * N;
            Vec vec;
#pragma unroll
            for (int j = 0; j < N; j++) vec.v[j] = value(x0 + j, y, x0 + j >= xl && x0 + j <= xr);
            *(Vec*)(row + x0) = vec;
        }
        for (int x = head + body * N + lane; x < w; x += 64) row[x] = value(x, y, x >= xl && x <= xr);
    }
}

static int hull_record_ok(const int* vertices, const int* hull_counts, int capacity, int frames, int w, int h, const void* out,
                          const char* who)
{
    if (frames < 1 || w <= 0 || h <= 0 || capacity < 1 || capacity > HULL_MAX_POINTS || !vertices || !hull_counts || !out ||
        (uintptr_t)vertices % 4 != 0 || (uintptr_t)hull_counts % 4 != 0) {
        set_error("%s: bad arguments (frames, w, h >= 1; vertex_capacity 1 .. %d; vertices, hull_counts, out: device arrays)",
                  who, HULL_MAX_POINTS);
        return CAMD_ERR_BAD_ARG;
    }
    if ((long long)frames * div_up(h, HULL_ROWS_PER_GROUP) > INT_MAX) {
        set_error("%s: %d frames of %d rows are beyond the grid", who, frames, h);
        return CAMD_ERR_UNSUPPORTED;
    }
    return CAMD_OK;
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_hull_fit(const double* uv, int uv_stride, const void* z, int z_type, size_t rows, const long long* start, int frames,
                  int w, int h, int keep_last_per_pixel, int vertex_capacity, int* vertices, int* hull_counts, double* abc,
                  int* status, void* queue)
{
    if (frames < 1 || uv_stride < 2 || vertex_capacity < 1 || vertex_capacity > HULL_MAX_POINTS || !vertices || !hull_counts ||
        !doubles_ok(abc) || !status || (rows && !doubles_ok(uv)) || (z && !float_type_ok(z_type)) ||
        (start && (uintptr_t)start % 8 != 0) || (!start && rows % (size_t)frames != 0) || rows >= ((size_t)1 << 40) ||
        (keep_last_per_pixel && (w <= 0 || h <= 0))) {
        set_error("camd_hull_fit: bad arguments (frames >= 1; uv_stride >= 2; vertex_capacity 1 .. %d; z_type CAMD_VALUE_F64 or "
                  "_F32; without start the rows are a multiple of the frames; keep_last_per_pixel needs w, h >= 1)",
                  HULL_MAX_POINTS);
        return CAMD_ERR_BAD_ARG;
    }
    if (!start && rows / (size_t)frames > (size_t)vertex_capacity) {
        set_error("camd_hull_fit: %zu rows per frame, the vertex capacity is %d", rows / (size_t)frames, vertex_capacity);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    HullFitArgs a = {};
    a.uv = uv, a.z = z, a.start = start, a.vertices = vertices, a.hull_counts = hull_counts, a.abc = abc, a.status = status;
    a.rows = rows, a.per_frame = (unsigned)(rows / (size_t)frames), a.uv_stride = uv_stride, a.z_type = z_type;
    a.frames = frames, a.w = w, a.h = h, a.keep_last = keep_last_per_pixel ? 1 : 0, a.capacity = vertex_capacity;
    const size_t lds = (size_t)vertex_capacity * 2 * sizeof(int);
    with_float(z ? z_type : CAMD_VALUE_F64, [&](auto v) {
        using Z = decltype(v);
        hipLaunchKernelGGL((k_hull_fit<Z>), dim3(frames), dim3(64), lds, (hipStream_t)queue, a);
    });
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_hull_fill(const int* vertices, const int* hull_counts, const double* abc, int vertex_capacity, int frames, int w, int h,
                   int reciprocal, const uint8_t* zero_frames, float* out, void* queue)
{
    int rc = hull_record_ok(vertices, hull_counts, vertex_capacity, frames, w, h, out, "camd_hull_fill");
    if (rc != CAMD_OK) return rc;
    if (!doubles_ok(abc) || (uintptr_t)out % 4 != 0) {
        set_error("camd_hull_fill: abc must be an aligned device array of doubles, out of floats");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    const int tiles = div_up(h, HULL_ROWS_PER_GROUP);
    hipLaunchKernelGGL((k_hull_fill<HullPlane>), dim3((unsigned)(frames * tiles)), dim3(256), 0, (hipStream_t)queue, vertices,
                       hull_counts, abc, vertex_capacity, frames, w, h, tiles, reciprocal ? 1 : 0, zero_frames,
                       (uintptr_t)out % 16 == 0 ? 1 : 0, out);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_hull_mask(const int* vertices, const int* hull_counts, int vertex_capacity, int frames, int w, int h, uint8_t* out,
                   void* queue)
{
    int rc = hull_record_ok(vertices, hull_counts, vertex_capacity, frames, w, h, out, "camd_hull_mask");
    if (rc != CAMD_OK) return rc;
    CAMD_NEED_DEVICE();
    const int tiles = div_up(h, HULL_ROWS_PER_GROUP);
    hipLaunchKernelGGL((k_hull_fill<HullMask>), dim3((unsigned)(frames * tiles)), dim3(256), 0, (hipStream_t)queue, vertices,
                       hull_counts, (const double*)nullptr, vertex_capacity, frames, w, h, tiles, 0, (const uint8_t*)nullptr,
                       (uintptr_t)out % 16 == 0 ? 1 : 0, out);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
