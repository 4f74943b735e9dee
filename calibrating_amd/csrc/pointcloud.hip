// pointcloud.hip -- the depth post-ops that follow get_depth in the reference's demos:
//   utils.depth_to_point_cloud   (utils.py:213-246)   depth (+ optional INTER_NEAREST upsampling) -> N x 3 points
//   utils.apply_T_to_point_cloud (utils.py:152-161)
//   utils.point_cloud_to_depth   (utils.py:249-318)   projection + "far first, near last" overwrite = z-buffer
//   Cam.project_cam2_depth       (camera.py:298-309)  the three above composed; here ONE fused scatter kernel
//   utils.point_cloud_to_arr2d   (utils.py:254-317)   the same z-buffer carrying a payload (values of the winning point)
//   utils.get_reproject_remap    (utils.py:332-344)   ... whose payload is the (u, v) of the source grid cell
// float64 throughout like the reference's NumPy.  Every matrix product is the chain dot3 / dot4 below: left to right,
// a plain first product, then fused multiply-adds.  oracle/pointcloud_ref.c states the same arithmetic as serial loops,
// and the tests hold every entry point of this file to it bit for bit, on every point and every pixel -- ties, image
// edges, half-way projections and NaN / inf included; that oracle in turn reproduces the reference's recorded runs.
#include "common.hpp"
#include "compact.hpp"

namespace camd {

struct PcGrid {
    int w, h;        // source depth
    int gw, gh;      // sampling grid (= w, h when rate == 1)
    double ifx, ify; // cv2.resize(INTER_NEAREST): sx = min(floor(x * ifx), w - 1)
    double rate;
};

__device__ __forceinline__ double pc_sample(const double* __restrict__ depth, const PcGrid& g, int x, int y)
{
    int sx = x, sy = y;
    if (g.gw != g.w || g.gh != g.h) {
        sx = min((int)floor(x * g.ifx), g.w - 1);
        sy = min((int)floor(y * g.ify), g.h - 1);
    }
    return depth[(size_t)sy * g.w + sx];
}

// Matrix products the way NumPy's matmul rounds them: the reference's (K^-1 @ P.T).T, (T @ P4.T).T and P @ K.T are BLAS
// dgemm calls whose x86-64 kernels accumulate the k terms in order with fused multiply-adds, starting from the plain
// first product.  Measured against the reference's own run (tests/golden/reference_plumbing.npz) and against NumPy on
// every shape involved: this chain reproduces the bits, individually rounded products and sums differ in 1 of 4 values.
__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
    return __fma_rn(a2, b2, __fma_rn(a1, b1, __dmul_rn(a0, b0)));
}
__device__ __forceinline__ double dot4(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3)
{
    return __fma_rn(a3, b3, __fma_rn(a2, b2, __fma_rn(a1, b1, __dmul_rn(a0, b0))));
}

// the z-buffers hold order_key(zs) (compact.hpp)
static constexpr unsigned long long ZKEY_EMPTY = 0xffffffffffffffffull;

// depth_to_point_cloud as a compaction (compact.hpp): the grid cells with a non-zero depth, in row-major order
struct PcRows {
    const double* depth;
    PcGrid g;
    double Ki[9];
    double* points;
    double* uv;  // NULL: the points alone
    __device__ __forceinline__ bool on(int x, int y) const { return pc_sample(depth, g, x, y) != 0.0; }
    __device__ __forceinline__ void emit(int x, int y, unsigned long long pos) const
    {
        const double z = pc_sample(depth, g, x, y);
        // utils.py:225-246: us, vs are grid indices (/ interpolation_rate when upsampled)
        const double u = g.rate == 1.0 ? (double)x : (double)x / g.rate;
        const double v = g.rate == 1.0 ? (double)y : (double)y / g.rate;
        const double p0 = u * z, p1 = v * z, p2 = 1.0 * z;
        points[pos * 3 + 0] = dot3(Ki[0], Ki[1], Ki[2], p0, p1, p2);
        points[pos * 3 + 1] = dot3(Ki[3], Ki[4], Ki[5], p0, p1, p2);
        points[pos * 3 + 2] = dot3(Ki[6], Ki[7], Ki[8], p0, p1, p2);
        if (uv) { uv[pos * 2] = u; uv[pos * 2 + 1] = v; }
    }
};

struct Mat34 { double m[12]; };
struct Mat33 { double m[9]; };

// project one camera-space point with K (utils.py:286-288, 311-316): the target pixel and the z-buffer key of the point.
// Every pass of every z-buffer calls this one function, so that a pass which recomputes a point sees the bits the
// pass before it saw.  false: the point lands outside the image (or its projection is NaN / inf) and is dropped.
__device__ __forceinline__ bool project_pixel(double X, double Y, double Z, const Mat33& K, int w, int h, size_t* pix,
                                              unsigned long long* key)
{
    const double xs = dot3(X, Y, Z, K.m[0], K.m[1], K.m[2]);
    const double ys = dot3(X, Y, Z, K.m[3], K.m[4], K.m[5]);
    const double zs = dot3(X, Y, Z, K.m[6], K.m[7], K.m[8]);
    const double u = xs / zs, v = ys / zs;
    const double ru = rint(u), rv = rint(v);  // np.round: half to even
    if (!(ru >= 0.0 && ru < (double)w && rv >= 0.0 && rv < (double)h)) return false;  // also drops NaN / inf
    *pix = (size_t)(int)rv * w + (int)ru;
    *key = order_key(zs);
    return true;
}

// ... and keep the nearest per pixel
__device__ __forceinline__ void zbuffer_point(double X, double Y, double Z, const Mat33& K, int w, int h,
                                              unsigned long long* __restrict__ keys)
{
    size_t pix;
    unsigned long long key;
    if (project_pixel(X, Y, Z, K, w, h, &pix, &key)) atomicMin(keys + pix, key);
}

__global__ __launch_bounds__(256) void k_pc_scatter(const double* __restrict__ points, size_t n, int stride, Mat33 K, int w,
                                                    int h, unsigned long long* __restrict__ keys)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    zbuffer_point(points[i * stride], points[i * stride + 1], points[i * stride + 2], K, w, h, keys);
}

__global__ __launch_bounds__(256) void k_pc_resolve(const unsigned long long* __restrict__ keys, size_t n, double bg,
                                                    double* __restrict__ depth)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) depth[i] = keys[i] == ZKEY_EMPTY ? bg : order_value(keys[i]);
}

__global__ __launch_bounds__(256) void k_apply_T(const double* __restrict__ src, size_t n, Mat34 T, double* __restrict__ dst)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = src[i * 3], y = src[i * 3 + 1], z = src[i * 3 + 2];
    dst[i * 3 + 0] = dot4(T.m[0], T.m[1], T.m[2], T.m[3], x, y, z, 1.0);
    dst[i * 3 + 1] = dot4(T.m[4], T.m[5], T.m[6], T.m[7], x, y, z, 1.0);
    dst[i * 3 + 2] = dot4(T.m[8], T.m[9], T.m[10], T.m[11], x, y, z, 1.0);
}

// one cell of camera 2's sampling grid -> point (K2^-1) -> T -> K1 projection: target pixel and key (false: z == 0 or
// outside).  Shared by the depth-only scatter and by both atomics passes of the payload z-buffer below.
__device__ __forceinline__ bool grid_cell_pixel(const double* __restrict__ depth2, const PcGrid& g, int x, int y,
                                                const Mat33& K2inv, const Mat34& T, const Mat33& K1, int w1, int h1,
                                                size_t* pix, unsigned long long* key)
{
    const double z = pc_sample(depth2, g, x, y);
    if (z == 0.0) return false;
    const double u = g.rate == 1.0 ? (double)x : (double)x / g.rate;
    const double v = g.rate == 1.0 ? (double)y : (double)y / g.rate;
    const double p0 = u * z, p1 = v * z, p2 = 1.0 * z;
    const double X = dot3(K2inv.m[0], K2inv.m[1], K2inv.m[2], p0, p1, p2);
    const double Y = dot3(K2inv.m[3], K2inv.m[4], K2inv.m[5], p0, p1, p2);
    const double Z = dot3(K2inv.m[6], K2inv.m[7], K2inv.m[8], p0, p1, p2);
    const double X1 = dot4(T.m[0], T.m[1], T.m[2], T.m[3], X, Y, Z, 1.0);
    const double Y1 = dot4(T.m[4], T.m[5], T.m[6], T.m[7], X, Y, Z, 1.0);
    const double Z1 = dot4(T.m[8], T.m[9], T.m[10], T.m[11], X, Y, Z, 1.0);
    return project_pixel(X1, Y1, Z1, K1, w1, h1, pix, key);
}

// Cam.project_cam2_depth fused: depth2 grid cell -> point (K2^-1) -> T -> K1 projection -> z-buffer
__global__ __launch_bounds__(256) void k_project_depth(const double* __restrict__ depth2, PcGrid g, Mat33 K2inv, Mat34 T,
                                                       Mat33 K1, int w1, int h1, unsigned long long* __restrict__ keys)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.gw) return;
    size_t pix;
    unsigned long long key;
    if (grid_cell_pixel(depth2, g, x, y, K2inv, T, K1, w1, h1, &pix, &key)) atomicMin(keys + pix, key);
}

// ---- the z-buffer that remembers its winner (point_cloud_to_arr2d with values, get_reproject_remap) -----------------
// The reference sorts the points far to near and lets the later write win (utils.py:280-288, 312-316); what arrives in
// a pixel is the PAYLOAD of the nearest point.  Three passes over caller-provided buffers:
//   1  keys[pix]  = min over the sources of order_key(zs)                  (atomicMin, u64; ZKEY_EMPTY = nobody)
//   2  owner[pix] = 1 + max index of the sources whose key equals keys[pix] (atomicMax, u32; 0 = nobody)
//   3  one thread per target pixel gathers the owner's payload, or the background value
// Two atomics passes because a 64-bit atomicMin cannot carry a 64-bit depth AND an index, and depth bits may not be
// dropped: the winner is decided on all 64 of them.  Both are commutative, so the result does not depend on the order
// in which the hardware serves them.  Points with bit-equal z on one pixel: the larger index wins -- what a STABLE
// far-to-near sort followed by last-write-wins gives; np.argsort's default (introsort) leaves that case to its
// internals.  index = row-major cell of the sampling grid (fused form) or row of the point array (generic form).
__global__ __launch_bounds__(256) void k_zb_clear(unsigned long long* __restrict__ keys, uint32_t* __restrict__ owner,
                                                  size_t n)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { keys[i] = ZKEY_EMPTY; owner[i] = 0u; }
}

template <bool OWNER>
__global__ __launch_bounds__(256) void k_reproject_pass(const double* __restrict__ depth2, size_t depth_stride, PcGrid g,
                                                        Mat33 K2inv, Mat34 T, Mat33 K1, int w1, int h1,
                                                        unsigned long long* __restrict__ keys,
                                                        uint32_t* __restrict__ owner)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.gw) return;
    const size_t b = blockIdx.z, npix = (size_t)w1 * h1;
    size_t pix;
    unsigned long long key;
    if (!grid_cell_pixel(depth2 + b * depth_stride, g, x, y, K2inv, T, K1, w1, h1, &pix, &key)) return;
    if (!OWNER) atomicMin(keys + b * npix + pix, key);
    else if (keys[b * npix + pix] == key) atomicMax(owner + b * npix + pix, (uint32_t)((size_t)y * g.gw + x) + 1u);
}

// pass 3 of get_reproject_remap: owner -> (x, y) of the grid cell -> np.float32(x / rate), np.float32(y / rate)
// (utils.py:234-240, 339); -1 where nothing landed (bg_value=-1, :342)
__global__ __launch_bounds__(256) void k_reproject_emit(const uint32_t* __restrict__ owner, int gw, double rate, size_t npix,
                                                        float bg, float* __restrict__ mapx, float* __restrict__ mapy,
                                                        size_t map_stride)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= npix) return;
    const uint32_t o = owner[b * npix + i];
    float fx = bg, fy = bg;
    if (o) {
        const uint32_t x = (o - 1u) % (uint32_t)gw, y = (o - 1u) / (uint32_t)gw;
        fx = (float)(rate == 1.0 ? (double)x : (double)x / rate);
        fy = (float)(rate == 1.0 ? (double)y : (double)y / rate);
    }
    mapx[b * map_stride + i] = fx;
    mapy[b * map_stride + i] = fy;
}

__global__ __launch_bounds__(256) void k_pc_owner(const double* __restrict__ points, size_t n, int stride, Mat33 K, int w,
                                                  int h, const unsigned long long* __restrict__ keys,
                                                  uint32_t* __restrict__ owner)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    size_t pix;
    unsigned long long key;
    if (!project_pixel(points[i * stride], points[i * stride + 1], points[i * stride + 2], K, w, h, &pix, &key)) return;
    if (keys[pix] == key) atomicMax(owner + pix, (uint32_t)i + 1u);
}

static int make_grid(PcGrid* g, int w, int h, double rate, const char* who)
{
    if (w <= 0 || h <= 0 || !(rate > 0.0)) { set_error("%s: bad size / interpolation rate", who); return CAMD_ERR_BAD_ARG; }
    g->w = w; g->h = h; g->rate = rate;
    if (rate == 1.0) {
        g->gw = w; g->gh = h; g->ifx = g->ify = 1.0;
    } else {
        // utils.py:231: y_, x_ = int(round(y * rate)), int(round(x * rate))  (Python round: half to even)
        g->gw = (int)nearbyint(w * rate);
        g->gh = (int)nearbyint(h * rate);
        if (g->gw <= 0 || g->gh <= 0) { set_error("%s: empty sampling grid", who); return CAMD_ERR_BAD_ARG; }
        g->ifx = 1.0 / ((double)g->gw / w);   // cv2.resize: inv_scale = dsize / ssize, ifx = 1 / inv_scale
        g->ify = 1.0 / ((double)g->gh / h);
    }
    return CAMD_OK;
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_point_cloud_grid(int w, int h, double rate, int* grid_w, int* grid_h)
{
    PcGrid g;
    int rc = make_grid(&g, w, h, rate, "camd_point_cloud_grid");
    if (rc != CAMD_OK) return rc;
    if (grid_w) *grid_w = g.gw;
    if (grid_h) *grid_h = g.gh;
    return CAMD_OK;
}

size_t camd_point_cloud_workspace_bytes(int w, int h, double rate)
{
    PcGrid g;
    if (make_grid(&g, w, h, rate, "camd_point_cloud_workspace_bytes") != CAMD_OK) return 0;
    return RowWorkspace::bytes(g.gh);
}

int camd_depth_to_point_cloud(const double* depth, int w, int h, const double Kinv[9], double rate, double* points,
                              double* uv, size_t capacity, unsigned long long* count, void* workspace, void* stream)
{
    PcGrid g;
    int rc = make_grid(&g, w, h, rate, "camd_depth_to_point_cloud");
    if (rc != CAMD_OK) return rc;
    if (!depth || !Kinv || !points || !count || !workspace) { set_error("camd_depth_to_point_cloud: NULL argument"); return CAMD_ERR_BAD_ARG; }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const RowWorkspace ws(workspace, g.gh);
    PcRows f;
    f.depth = depth; f.g = g; f.points = points; f.uv = uv;
    for (int i = 0; i < 9; i++) f.Ki[i] = Kinv[i];
    row_count(f, g.gw, g.gh, ws.rowcount, st);
    row_scan(ws.rowcount, g.gh, ws.rowoff, count, st);
    row_emit(f, g.gw, g.gh, ws.rowoff, capacity, nullptr, st);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_apply_T_to_point_cloud(const double* points, size_t n, const double T[16], double* out, void* stream)
{
    if (!T || (n && (!points || !out))) { set_error("camd_apply_T_to_point_cloud: NULL argument"); return CAMD_ERR_BAD_ARG; }
    if (n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    Mat34 M;
    for (int i = 0; i < 12; i++) M.m[i] = T[i];
    hipLaunchKernelGGL(k_apply_T, dim3(div_up((long long)n, 256)), dim3(256), 0, (hipStream_t)stream, points, n, M, out);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_point_cloud_to_depth(const double* points, size_t n, int point_stride, const double K[9], int w, int h,
                              double bg_value, double* depth, unsigned long long* keys_ws, void* stream)
{
    if (!K || !depth || !keys_ws || w <= 0 || h <= 0 || point_stride < 3 || (n && !points)) {
        set_error("camd_point_cloud_to_depth: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)w * h;
    Mat33 Km;
    for (int i = 0; i < 9; i++) Km.m[i] = K[i];
    fill(keys_ws, npix, ZKEY_EMPTY, nullptr, st);
    if (n) hipLaunchKernelGGL(k_pc_scatter, dim3(div_up((long long)n, 256)), dim3(256), 0, st, points, n, point_stride, Km, w, h, keys_ws);
    hipLaunchKernelGGL(k_pc_resolve, dim3(div_up((long long)npix, 256)), dim3(256), 0, st, keys_ws, npix, bg_value, depth);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_project_depth(const double* depth2, int w2, int h2, const double K2inv[9], const double T_2in1[16],
                       const double K1[9], double rate, int w1, int h1, double* depth1, unsigned long long* keys_ws,
                       void* stream)
{
    PcGrid g;
    int rc = make_grid(&g, w2, h2, rate, "camd_project_depth");
    if (rc != CAMD_OK) return rc;
    if (!depth2 || !K2inv || !T_2in1 || !K1 || !depth1 || !keys_ws || w1 <= 0 || h1 <= 0) {
        set_error("camd_project_depth: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)w1 * h1;
    Mat33 Ki, Km;
    Mat34 M;
    for (int i = 0; i < 9; i++) { Ki.m[i] = K2inv[i]; Km.m[i] = K1[i]; }
    for (int i = 0; i < 12; i++) M.m[i] = T_2in1[i];
    fill(keys_ws, npix, ZKEY_EMPTY, nullptr, st);
    hipLaunchKernelGGL(k_project_depth, dim3(div_up(g.gw, 256), g.gh), dim3(256), 0, st, depth2, g, Ki, M, Km, w1, h1, keys_ws);
    hipLaunchKernelGGL(k_pc_resolve, dim3(div_up((long long)npix, 256)), dim3(256), 0, st, keys_ws, npix, 0.0, depth1);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_reproject_remap(const double* depth2, int w2, int h2, size_t depth_stride, const double K2inv[9],
                         const double T_2in1[16], const double K1[9], double rate, int w1, int h1, float* mapx,
                         float* mapy, size_t map_stride, unsigned long long* keys_ws, uint32_t* owner_ws, int batch,
                         void* stream)
{
    PcGrid g;
    int rc = make_grid(&g, w2, h2, rate, "camd_reproject_remap");
    if (rc != CAMD_OK) return rc;
    if (!depth2 || !K2inv || !T_2in1 || !K1 || !mapx || !mapy || !keys_ws || !owner_ws || w1 <= 0 || h1 <= 0 ||
        batch <= 0 || batch > 65535 || g.gh > 65535 || (size_t)w1 * h1 > ((size_t)1 << 38) / (size_t)(batch > 0 ? batch : 1) ||
        (batch > 1 && (depth_stride < (size_t)w2 * h2 || map_stride < (size_t)w1 * h1))) {
        set_error("camd_reproject_remap: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    if ((unsigned long long)g.gw * (unsigned long long)g.gh >= 0xffffffffull) {
        set_error("camd_reproject_remap: a sampling grid of %d x %d cells does not fit the 32-bit owner index", g.gw, g.gh);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)w1 * h1;
    Mat33 Ki, Km;
    Mat34 M;
    for (int i = 0; i < 9; i++) { Ki.m[i] = K2inv[i]; Km.m[i] = K1[i]; }
    for (int i = 0; i < 12; i++) M.m[i] = T_2in1[i];
    const dim3 src_grid(div_up(g.gw, 256), g.gh, batch), dst_grid(div_up((long long)npix, 256), batch);
    hipLaunchKernelGGL(k_zb_clear, dim3(div_up((long long)(npix * batch), 256)), dim3(256), 0, st, keys_ws, owner_ws,
                       npix * batch);
    hipLaunchKernelGGL((k_reproject_pass<false>), src_grid, dim3(256), 0, st, depth2, depth_stride, g, Ki, M, Km, w1, h1,
                       keys_ws, owner_ws);
    hipLaunchKernelGGL((k_reproject_pass<true>), src_grid, dim3(256), 0, st, depth2, depth_stride, g, Ki, M, Km, w1, h1,
                       keys_ws, owner_ws);
    hipLaunchKernelGGL(k_reproject_emit, dst_grid, dim3(256), 0, st, owner_ws, g.gw, g.rate, npix, -1.0f, mapx, mapy,
                       map_stride);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_point_cloud_to_arr2d(const double* points, size_t n, int point_stride, const double K[9], int w, int h,
                              const void* values, int channels, int value_type, double bg_value, void* out,
                              unsigned long long* keys_ws, uint32_t* owner_ws, void* stream)
{
    if (!K || !out || !keys_ws || !owner_ws || w <= 0 || h <= 0 || point_stride < 3 || channels < 1 ||
        (n && (!points || !values))) {
        set_error("camd_point_cloud_to_arr2d: bad arguments");
        return CAMD_ERR_BAD_ARG;
    }
    if (!float_u8_type_ok(value_type)) {
        set_error("camd_point_cloud_to_arr2d: value_type %d is none of float64 / float32 / uint8", value_type);
        return CAMD_ERR_BAD_ARG;
    }
    if (value_type == CAMD_VALUE_U8 && !(bg_value >= 0.0 && bg_value <= 255.0 && bg_value == (double)(uint8_t)bg_value)) {
        set_error("camd_point_cloud_to_arr2d: bg_value %g is not a uint8", bg_value);
        return CAMD_ERR_BAD_ARG;
    }
    if ((unsigned long long)n >= 0xffffffffull) {
        set_error("camd_point_cloud_to_arr2d: %zu points do not fit the 32-bit owner index", n);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)w * h;
    Mat33 Km;
    for (int i = 0; i < 9; i++) Km.m[i] = K[i];
    const dim3 src_grid(div_up((long long)n, 256)), dst_grid(div_up((long long)npix, 256));
    hipLaunchKernelGGL(k_zb_clear, dst_grid, dim3(256), 0, st, keys_ws, owner_ws, npix);
    if (n) {
        hipLaunchKernelGGL(k_pc_scatter, src_grid, dim3(256), 0, st, points, n, point_stride, Km, w, h, keys_ws);
        hipLaunchKernelGGL(k_pc_owner, src_grid, dim3(256), 0, st, points, n, point_stride, Km, w, h, keys_ws, owner_ws);
    }
    owner_gather(value_type, owner_ws, npix, values, channels, bg_value, 0, out, st);  // utils.py:308, 314-316
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
