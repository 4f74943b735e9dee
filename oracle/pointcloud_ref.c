/*
 * pointcloud_ref.c -- exact CPU restatement of the point-cloud and z-buffer family (csrc/pointcloud.hip).
 *
 * TEST INFRASTRUCTURE ONLY (see oracle.h).  Plain serial loops in index order: no order-preserving keys, no atomics,
 * no passes.  The arithmetic is the one include/calibrating_amd.h and pointcloud.hip state as their contract, which is
 * how NumPy's matmul (a BLAS dgemm with FMA kernels) rounds the reference's (K^-1 @ P.T).T, (T @ P4.T).T and P @ K.T:
 * every dot product is a left-to-right chain that starts with the plain first product and continues with fused
 * multiply-adds.  -ffp-contract=off (Makefile) keeps the compiler from fusing anything else.
 *
 *   sampling grid  gw = nearbyint(w * rate), gh likewise; ifx = 1 / ((double)gw / w); sx = min(floor(x * ifx), w - 1)
 *                  u = rate == 1 ? x : x / rate
 *   point          K^-1 row . (u*z, v*z, 1.0*z)
 *   pose           T row . (X, Y, Z, 1)
 *   projection     xs, ys, zs = point . K rows (zs too: the real third row); u = xs / zs, v = ys / zs; rint
 *                  kept iff 0 <= ru < w && 0 <= rv < h (drops NaN and inf)
 *   z-buffer       sources in index order, a source is taken when zs < best || zs == best: the later index wins a
 *                  bit-equal tie, a negative zs beats a positive one
 */
#include <math.h>

#include "oracle.h"

static double pc_dot3(const double* a, double b0, double b1, double b2)
{
    return __builtin_fma(a[2], b2, __builtin_fma(a[1], b1, a[0] * b0));
}

static double pc_dot4(const double* a, double b0, double b1, double b2, double b3)
{
    return __builtin_fma(a[3], b3, __builtin_fma(a[2], b2, __builtin_fma(a[1], b1, a[0] * b0)));
}

typedef struct pc_grid {
    int w, h, gw, gh;
    double ifx, ify, rate;
} pc_grid;

static int pc_make_grid(pc_grid* g, int w, int h, double rate)
{
    if (w <= 0 || h <= 0 || !(rate > 0.0)) return -1;
    g->w = w; g->h = h; g->rate = rate;
    if (rate == 1.0) {
        g->gw = w; g->gh = h; g->ifx = g->ify = 1.0;
        return 0;
    }
    const double fw = nearbyint(w * rate), fh = nearbyint(h * rate);
    if (!(fw >= 1.0 && fw <= 2147483647.0 && fh >= 1.0 && fh <= 2147483647.0)) return -1;
    g->gw = (int)fw; g->gh = (int)fh;
    g->ifx = 1.0 / ((double)g->gw / w);
    g->ify = 1.0 / ((double)g->gh / h);
    return 0;
}

static double pc_sample(const double* depth, const pc_grid* g, int x, int y)
{
    int sx = x, sy = y;
    if (g->gw != g->w || g->gh != g->h) {
        const double fx = floor(x * g->ifx), fy = floor(y * g->ify);
        sx = fx < (double)(g->w - 1) ? (int)fx : g->w - 1;
        sy = fy < (double)(g->h - 1) ? (int)fy : g->h - 1;
    }
    return depth[(size_t)sy * g->w + sx];
}

/* grid cell -> the operands (u*z, v*z, 1.0*z) of the K^-1 product, and (u, v) */
static void pc_cell(const pc_grid* g, int x, int y, double z, double p[3], double uv[2])
{
    uv[0] = g->rate == 1.0 ? (double)x : (double)x / g->rate;
    uv[1] = g->rate == 1.0 ? (double)y : (double)y / g->rate;
    p[0] = uv[0] * z; p[1] = uv[1] * z; p[2] = 1.0 * z;
}

/* 1: the point lands on pixel *pix with depth *zs; 0: dropped */
static int pc_project(double X, double Y, double Z, const double K[9], int w, int h, size_t* pix, double* zs)
{
    const double xs = pc_dot3(K, X, Y, Z), ys = pc_dot3(K + 3, X, Y, Z);
    *zs = pc_dot3(K + 6, X, Y, Z);
    const double ru = rint(xs / *zs), rv = rint(ys / *zs);
    if (!(ru >= 0.0 && ru < (double)w && rv >= 0.0 && rv < (double)h)) return 0;
    *pix = (size_t)(int)rv * w + (size_t)(int)ru;
    return 1;
}

static void pc_clear(int64_t* owner, double* zs, size_t npix)
{
    for (size_t i = 0; i < npix; i++) { owner[i] = -1; zs[i] = 0.0; }
}

static void pc_take(int64_t* owner, double* best, size_t pix, int64_t src, double zs)
{
    if (owner[pix] < 0 || zs < best[pix] || zs == best[pix]) { owner[pix] = src; best[pix] = zs; }
}

long long oracle_depth_to_point_cloud(const double* depth, int w, int h, const double Kinv[9], double rate,
                                      double* points, double* uv)
{
    pc_grid g;
    if (pc_make_grid(&g, w, h, rate)) return -1;
    long long n = 0;
    for (int y = 0; y < g.gh; y++)
        for (int x = 0; x < g.gw; x++) {
            const double z = pc_sample(depth, &g, x, y);
            if (z == 0.0) continue;
            double p[3], c[2];
            pc_cell(&g, x, y, z, p, c);
            if (points)
                for (int r = 0; r < 3; r++) points[n * 3 + r] = pc_dot3(Kinv + 3 * r, p[0], p[1], p[2]);
            if (uv) { uv[n * 2] = c[0]; uv[n * 2 + 1] = c[1]; }
            n++;
        }
    return n;
}

void oracle_apply_T(const double* points, size_t n, const double T[16], double* out)
{
    for (size_t i = 0; i < n; i++)
        for (int r = 0; r < 3; r++)
            out[i * 3 + r] = pc_dot4(T + 4 * r, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], 1.0);
}

int oracle_zbuffer_points(const double* points, size_t n, int stride, const double K[9], int w, int h,
                          int64_t* owner, double* zs)
{
    if (w <= 0 || h <= 0 || stride < 3) return -1;
    pc_clear(owner, zs, (size_t)w * h);
    for (size_t i = 0; i < n; i++) {
        size_t pix;
        double z;
        const double* p = points + i * (size_t)stride;
        if (pc_project(p[0], p[1], p[2], K, w, h, &pix, &z)) pc_take(owner, zs, pix, (int64_t)i, z);
    }
    return 0;
}

int oracle_zbuffer_grid(const double* depth2, int w2, int h2, const double K2inv[9], const double T[16],
                        const double K1[9], double rate, int w1, int h1, int64_t* owner, double* zs)
{
    pc_grid g;
    if (pc_make_grid(&g, w2, h2, rate) || w1 <= 0 || h1 <= 0) return -1;
    pc_clear(owner, zs, (size_t)w1 * h1);
    for (int y = 0; y < g.gh; y++)
        for (int x = 0; x < g.gw; x++) {
            const double z = pc_sample(depth2, &g, x, y);
            if (z == 0.0) continue;
            double p[3], c[2], P[3], Q[3], zq;
            size_t pix;
            pc_cell(&g, x, y, z, p, c);
            for (int r = 0; r < 3; r++) P[r] = pc_dot3(K2inv + 3 * r, p[0], p[1], p[2]);
            for (int r = 0; r < 3; r++) Q[r] = pc_dot4(T + 4 * r, P[0], P[1], P[2], 1.0);
            if (pc_project(Q[0], Q[1], Q[2], K1, w1, h1, &pix, &zq))
                pc_take(owner, zs, pix, (int64_t)y * g.gw + x, zq);
        }
    return 0;
}

int oracle_point_cloud_grid(int w, int h, double rate, int* gw, int* gh)
{
    pc_grid g;
    if (pc_make_grid(&g, w, h, rate)) return -1;
    *gw = g.gw; *gh = g.gh;
    return 0;
}
