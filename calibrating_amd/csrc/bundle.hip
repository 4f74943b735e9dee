// bundle.hip -- the poses of N views (3 <= N <= 16) and one world point per match refined together from the matched
// pinhole pixels of pairs of views: the joint refinement after ReconstructionExtrinsics' propagation.  The reference has
// none (its reconstruction_epipolar_geometry.py:31-314 ends at the propagation); the contract is this project's own
// (INTEGRATION.md section F).
//
// The problem.  Every match of pair (a, b), a < b, is one world point X with exactly two observations.  Unknowns: X (3) per
// used match and the world-to-camera pose (R, t) of every view, pnp.hip's local perturbation R <- exp([w]x) R, t <- t + d.
// Seven numbers are held: the pose of `fixed` and one coordinate (`axis`) of the world centre of `anchor`.  For the
// anchor the step is taken in (w, e), e a shift of its centre c = -R^T t: to first order d = -R e - t x w, so with
// M = [I 0; -[t]x -R] the reduced system is M^T (S + lambda diag U) M in the anchor's rows and columns, row 3 + axis of
// them dropped; its candidate is R' = exp([w]x) R, c' = c + e, t' = -R' c', which keeps the coordinate exactly.
//
// The normal matrix is an arrow the other way round from stereo_calibrate.hip's: the MANY blocks are the points' 3 x 3
// V = Ga^T Ga + Gb^T Gb, the SHARED block is all the views.  A point gives, with V* = V + lambda diag V = L L^T,
// Z_v = L^-1 (J_v^T G_v)^T (3 x 6) and y = L^-1 (Ga^T ra + Gb^T rb):
//   S_aa += Ja^T Ja - Za^T Za    S_bb += Jb^T Jb - Zb^T Zb    S_ba += -Zb^T Za    g_v += J_v^T r_v - Z_v^T y
// and its own step follows from the views' steps: dX = -L^-T (y + Za da + Zb db).  Nothing per point is stored but X and
// its candidate; the terms are formed again where they are needed (point_terms, the one code path of stages 2 and 4).
//
// Kernels.  k_bundle_start: one lane per match, the midpoint of the two rays and the status; the used matches are
// compacted per pair by compact.hpp's count / scan / emit over segments of BUNDLE_SEGMENT rows that never straddle two
// pairs.  k_bundle_linearise: one lane per used point, a workgroup per chunk of 256 points of ONE pair (a host-made
// table), three passes over the chunk -- (S_aa, g_a, diag U_a, cost), (S_bb, g_b, diag U_b), S_ba: 35 / 33 / 36
// accumulators beside the point's terms -- each summed by the butterfly and then (w0 + w1) + (w2 + w3): one partial per
// workgroup.  k_bundle_pair_sum: one wavefront per pair, lane l takes partials l, l + 64, ... in rising order, then the
// butterfly.  k_bundle_solve: one workgroup places the pairs' blocks in rising order into the lower triangle in LDS
// (6 N (6 N + 1) / 2 doubles, 37 KB at N = 16), damps, transforms the anchor, factors the 6 N - 7 kept rows in place
// (right-looking Cholesky: every element takes its subtractions in rising column order whatever the thread) and solves.
// k_bundle_evaluate / k_bundle_update: the candidates and the accept / damp / stop bookkeeping of the joint solvers
// (joint_common.hpp's lm_update, shared with calibrate.hip and stereo_calibrate.hip; their arrow template is not used
// here: the many blocks are 3 x 3 and the shared one is factored in LDS).  No atomics: the same input gives the same bits
// on every run.
#include "compact.hpp"
#include "joint_common.hpp"

namespace camd {

constexpr int BUNDLE_MAX_EVALUATIONS = 100;  // every case of tests/bundle_cases.py ends below half of it
constexpr int BUNDLE_CHUNK = CAMD_BUNDLE_CHUNK, BUNDLE_SEGMENT = CAMD_BUNDLE_SEGMENT, BUNDLE_MAX_VIEWS = CAMD_BUNDLE_MAX_VIEWS;
constexpr int BUNDLE_PARTIAL = CAMD_BUNDLE_PARTIAL_DOUBLES, BUNDLE_EVAL = CAMD_BUNDLE_EVAL_DOUBLES;
// |d_a x d_b| of the unit rays below which a match has no start point (status 2): a triangulation angle under 0.03 rad
// (1.7 degrees).  Below it the depth of a point is decided by the noise of the pixels and of the start poses, and such
// points run off to infinity or to z = 0 during the iteration (tests/bundle_cases.py "sixteen" has such pairs).
constexpr double BUNDLE_MIN_SINE = 0.03;
// a partial of a pair's part of the reduced system
enum { BP_AA = 0, BP_BB = 21, BP_BA = 42, BP_GA = 78, BP_GB = 84, BP_DA = 90, BP_DB = 96, BP_COST = 102, BP_BAD = 103 };
// a partial of the candidate: its cost, |dX|^2, |X|^2, points whose candidate is behind a view or whose block did not factor
enum { BE_COST = 0, BE_STEP = 1, BE_NORM = 2, BE_BAD = 3 };
enum {
    BS_ACCEPT = CAMD_BUNDLE_ACCEPT, BS_LAMBDA = CAMD_BUNDLE_LAMBDA, BS_COST = CAMD_BUNDLE_COST,
    BS_EVALS = CAMD_BUNDLE_EVALUATIONS, BS_STATUS = CAMD_BUNDLE_STATUS,
    BS_CONVERGED = CAMD_BUNDLE_CONVERGED, BS_SOLVED = CAMD_BUNDLE_SOLVED, BS_PIVOT = CAMD_BUNDLE_PIVOT,
    BS_FIXED = CAMD_BUNDLE_FIXED, BS_ANCHOR = CAMD_BUNDLE_ANCHOR, BS_AXIS = CAMD_BUNDLE_AXIS, BS_COST0 = CAMD_BUNDLE_COST0,
    BS_POSES = CAMD_BUNDLE_POSES, BS_CAND = CAMD_BUNDLE_CANDIDATE, BS_STEP = CAMD_BUNDLE_STEP, BS_K = CAMD_BUNDLE_K,
    BS_LABEL = CAMD_BUNDLE_LABEL
};

struct BundleArgs {
    const void *uv_a, *uv_b;  // the matches as given: [matches][2] of uv_type
    int uv_type, views, pairs, segments, chunks;
    long long matches, used;
    double threshold2;            // the squared threshold, < 0: none
    const int* pair_views;        // pairs x 2
    const long long* pair_start;  // pairs + 1: the rows of pair p
    const long long* seg_first;   // segments: the first row of a segment; seg_n: its rows (<= BUNDLE_SEGMENT)
    const int* seg_n;
    const int* chunk_table;       // chunks x 4: pair, first used point, points (<= BUNDLE_CHUNK), 0
    const long long* pair_chunk;  // pairs + 1: the chunks of pair p
    int* status;                  // matches
    double* points;               // matches x 3
    unsigned long long* rowoff;   // segments + 1
    uint32_t* rowcount;           // segments
    void *cuv_a, *cuv_b;          // used x 2 of uv_type
    double *X, *Xc;               // used x 3: the points and their candidates
    long long* src;               // used: the row a used point came from
    double *partials, *pairblk, *epartials, *epairblk, *state, *pair_error, *rows_a, *rows_b;
};

struct View {
    double R[9], t[3], fx, fy, cx, cy;
};
__device__ __forceinline__ void load_view(const double* state, int where, int v, View& q)
{
    load_pose(state + where + 12 * v, q.R, q.t);
    const double* k = state + BS_K + 4 * v;
    q.fx = k[0], q.fy = k[1], q.cx = k[2], q.cy = k[3];
}

// one observation of X in view q: the camera point's z, the residual (projected - observed), and with TERMS its 2 x 6
// Jacobian J in the view's (w, d) and 2 x 3 Jacobian G in X
template <bool TERMS>
__device__ __forceinline__ double observe(const View& q, const double X[3], const double uv[2], double r[2], double J[2][6],
                                          double G[2][3])
{
    const double* R = q.R;
    const double P[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2], R[3] * X[0] + R[4] * X[1] + R[5] * X[2],
                         R[6] * X[0] + R[7] * X[1] + R[8] * X[2]};
    const double z = P[2] + q.t[2];
    const double iz = z != 0. ? __ddiv_rn(1., z) : 1.;
    const double x = (P[0] + q.t[0]) * iz, y = (P[1] + q.t[1]) * iz;
    r[0] = x * q.fx + q.cx - uv[0], r[1] = y * q.fy + q.cy - uv[1];
    if (TERMS) {
        const double g[2][3] = {{q.fx * iz, 0., -(q.fx * x) * iz}, {0., q.fy * iz, -(q.fy * y) * iz}};
#pragma unroll
        for (int e = 0; e < 2; e++) {
            J[e][0] = P[1] * g[e][2] - P[2] * g[e][1];
            J[e][1] = P[2] * g[e][0] - P[0] * g[e][2];
            J[e][2] = P[0] * g[e][1] - P[1] * g[e][0];
            J[e][3] = g[e][0], J[e][4] = g[e][1], J[e][5] = g[e][2];
#pragma unroll
            for (int j = 0; j < 3; j++) G[e][j] = g[e][0] * R[j] + g[e][1] * R[3 + j] + g[e][2] * R[6 + j];
        }
    }
    return z;
}

// everything stages 2 and 4 need of one point at the current estimate and lambda
struct PointTerms {
    double ra[2], rb[2], Ja[2][6], Jb[2][6];
    double L[6], il[3];        // V + lambda diag V = L L^T (packed lower triangle), 1 / its diagonal
    double Za[3][6], Zb[3][6]; // L^-1 (J^T G)^T
    double y[3];               // L^-1 (Ga^T ra + Gb^T rb)
    bool ok;
};
__device__ __forceinline__ void point_terms(const View& qa, const View& qb, const double X[3], const double ua[2], const double ub[2],
                                            double lambda, PointTerms& o)
{
    double Ga[2][3], Gb[2][3];
    observe<true>(qa, X, ua, o.ra, o.Ja, Ga);
    observe<true>(qb, X, ub, o.rb, o.Jb, Gb);
    double V[6], gp[3], pivot;
#pragma unroll
    for (int p = 0; p < 3; p++) {
#pragma unroll
        for (int q = 0; q <= p; q++)
            V[p * (p + 1) / 2 + q] = (Ga[0][p] * Ga[0][q] + Ga[1][p] * Ga[1][q]) + (Gb[0][p] * Gb[0][q] + Gb[1][p] * Gb[1][q]);
        gp[p] = (Ga[0][p] * o.ra[0] + Ga[1][p] * o.ra[1]) + (Gb[0][p] * o.rb[0] + Gb[1][p] * o.rb[1]);
    }
    damped<3>(V, lambda, o.L);
    o.ok = cholesky<3>(o.L, pivot);
    const double* L = o.L;
    o.il[0] = __ddiv_rn(1., L[0]), o.il[1] = __ddiv_rn(1., L[2]), o.il[2] = __ddiv_rn(1., L[5]);
    auto forward = [&](double w0, double w1, double w2, double& z0, double& z1, double& z2) {
        z0 = w0 * o.il[0];
        z1 = (w1 - L[1] * z0) * o.il[1];
        z2 = (w2 - L[3] * z0 - L[4] * z1) * o.il[2];
    };
#pragma unroll
    for (int i = 0; i < 6; i++) {
        forward(o.Ja[0][i] * Ga[0][0] + o.Ja[1][i] * Ga[1][0], o.Ja[0][i] * Ga[0][1] + o.Ja[1][i] * Ga[1][1],
                o.Ja[0][i] * Ga[0][2] + o.Ja[1][i] * Ga[1][2], o.Za[0][i], o.Za[1][i], o.Za[2][i]);
        forward(o.Jb[0][i] * Gb[0][0] + o.Jb[1][i] * Gb[1][0], o.Jb[0][i] * Gb[0][1] + o.Jb[1][i] * Gb[1][1],
                o.Jb[0][i] * Gb[0][2] + o.Jb[1][i] * Gb[1][2], o.Zb[0][i], o.Zb[1][i], o.Zb[2][i]);
    }
    forward(gp[0], gp[1], gp[2], o.y[0], o.y[1], o.y[2]);
}

// the chunk of this workgroup: its pair's views and this lane's used point (on: it has one).  A table entry outside the
// arrays gives an empty chunk.
struct Chunk {
    int pair, a, b;
    long long at;
    bool on;
};
__device__ __forceinline__ Chunk chunk_of(const BundleArgs& g, int c)
{
    const int* e = g.chunk_table + 4 * (size_t)c;
    Chunk k = {e[0], 0, 0, (long long)e[1] + threadIdx.x, false};
    if (k.pair < 0 || k.pair >= g.pairs || e[1] < 0 || e[2] < 0 || e[2] > BUNDLE_CHUNK || (long long)e[1] + e[2] > g.used) return k;
    k.a = g.pair_views[2 * k.pair], k.b = g.pair_views[2 * k.pair + 1];
    if (k.a < 0 || k.b < 0 || k.a >= g.views || k.b >= g.views) return k;
    k.on = (int)threadIdx.x < e[2];
    return k;
}
__device__ __forceinline__ void load_used(const BundleArgs& g, long long at, const double* Xs, double X[3], double ua[2], double ub[2])
{
    X[0] = Xs[3 * at], X[1] = Xs[3 * at + 1], X[2] = Xs[3 * at + 2];
    ua[0] = load_value(g.cuv_a, g.uv_type, 2 * (size_t)at), ua[1] = load_value(g.cuv_a, g.uv_type, 2 * (size_t)at + 1);
    ub[0] = load_value(g.cuv_b, g.uv_type, 2 * (size_t)at), ub[1] = load_value(g.cuv_b, g.uv_type, 2 * (size_t)at + 1);
}

// Q sums of the workgroup's 256 lanes: the butterfly in each wave, then (w0 + w1) + (w2 + w3); thread q < Q returns sum q.
// sh: __shared__ double[4 * Q], free again after the barrier that ends the call
template <int Q>
__device__ __forceinline__ double block_sums(double* s, double* sh)
{
    wave_sum_all<Q>(s);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < Q; q++) sh[(threadIdx.x >> 6) * Q + q] = s[q];
    }
    __syncthreads();
    const int q = (int)threadIdx.x < Q ? threadIdx.x : 0;
    const double v = (sh[q] + sh[Q + q]) + (sh[2 * Q + q] + sh[3 * Q + q]);
    __syncthreads();
    return v;
}

// ---- stage 1: the start point and the status of every match ----------------------------------------------------------
__global__ __launch_bounds__(256) void k_bundle_start(BundleArgs g)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int p = blockIdx.y;
    const long long row = g.pair_start[p] + i;
    if (i < 0 || row >= g.pair_start[p + 1] || row < 0 || row >= g.matches) return;
    const int a = g.pair_views[2 * p], b = g.pair_views[2 * p + 1];
    double X[3] = {NAN, NAN, NAN};
    int status = 1;
    if (a >= 0 && b >= 0 && a < g.views && b < g.views) {
        View qa, qb;
        load_view(g.state, BS_POSES, a, qa);
        load_view(g.state, BS_POSES, b, qb);
        const double ua[2] = {load_value(g.uv_a, g.uv_type, 2 * (size_t)row), load_value(g.uv_a, g.uv_type, 2 * (size_t)row + 1)};
        const double ub[2] = {load_value(g.uv_b, g.uv_type, 2 * (size_t)row), load_value(g.uv_b, g.uv_type, 2 * (size_t)row + 1)};
        if (isfinite(ua[0]) && isfinite(ua[1]) && isfinite(ub[0]) && isfinite(ub[1])) {
            // the unit rays in the world and the views' centres c = -R^T t
            double d[2][3], c[2][3];
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const View& q = s ? qb : qa;
                const double* uv = s ? ub : ua;
                const double x = (uv[0] - q.cx) * __ddiv_rn(1., q.fx), y = (uv[1] - q.cy) * __ddiv_rn(1., q.fy);
                double n2 = 0.;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    d[s][j] = q.R[j] * x + q.R[3 + j] * y + q.R[6 + j];
                    c[s][j] = -(q.R[j] * q.t[0] + q.R[3 + j] * q.t[1] + q.R[6 + j] * q.t[2]);
                    n2 += d[s][j] * d[s][j];
                }
                const double in = __ddiv_rn(1., sqrt(n2));
#pragma unroll
                for (int j = 0; j < 3; j++) d[s][j] *= in;
            }
            const double cr[3] = {d[0][1] * d[1][2] - d[0][2] * d[1][1], d[0][2] * d[1][0] - d[0][0] * d[1][2],
                                  d[0][0] * d[1][1] - d[0][1] * d[1][0]};
            const double s2 = cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2];
            const double w[3] = {c[0][0] - c[1][0], c[0][1] - c[1][1], c[0][2] - c[1][2]};
            const double bb = d[0][0] * d[1][0] + d[0][1] * d[1][1] + d[0][2] * d[1][2];
            const double dd = d[0][0] * w[0] + d[0][1] * w[1] + d[0][2] * w[2];
            const double ee = d[1][0] * w[0] + d[1][1] * w[1] + d[1][2] * w[2];
            status = 2;
            if (s2 >= BUNDLE_MIN_SINE * BUNDLE_MIN_SINE) {
                const double is = __ddiv_rn(1., s2), sa = (bb * ee - dd) * is, sb = (ee - bb * dd) * is;
                double Y[3], ra[2], rb[2];
#pragma unroll
                for (int j = 0; j < 3; j++) Y[j] = 0.5 * ((c[0][j] + sa * d[0][j]) + (c[1][j] + sb * d[1][j]));
                const double za = observe<false>(qa, Y, ua, ra, nullptr, nullptr), zb = observe<false>(qb, Y, ub, rb, nullptr, nullptr);
                if (za > 0. && zb > 0. && isfinite(Y[0]) && isfinite(Y[1]) && isfinite(Y[2])) {
                    const double ea = ra[0] * ra[0] + ra[1] * ra[1], eb = rb[0] * rb[0] + rb[1] * rb[1];
                    status = (g.threshold2 >= 0. && (ea > g.threshold2 || eb > g.threshold2)) ? 3 : 0;
                    if (status == 0) X[0] = Y[0], X[1] = Y[1], X[2] = Y[2];
                }
            }
        }
    }
    g.status[row] = status;
    g.points[3 * row] = X[0], g.points[3 * row + 1] = X[1], g.points[3 * row + 2] = X[2];
}

// the compaction's predicate: element x of segment y is used
struct BundleUsed {
    BundleArgs g;
    __device__ __forceinline__ bool on(int x, int y) const
    {
        const long long row = g.seg_first[y] + x;
        return x < g.seg_n[y] && row >= 0 && row < g.matches && g.status[row] == 0;
    }
    __device__ __forceinline__ void emit(int x, int y, unsigned long long pos) const
    {
        const size_t row = (size_t)(g.seg_first[y] + x);
        with_float(g.uv_type, [&](auto v) {
            using T = decltype(v);
            ((T*)g.cuv_a)[2 * pos] = ((const T*)g.uv_a)[2 * row], ((T*)g.cuv_a)[2 * pos + 1] = ((const T*)g.uv_a)[2 * row + 1];
            ((T*)g.cuv_b)[2 * pos] = ((const T*)g.uv_b)[2 * row], ((T*)g.cuv_b)[2 * pos + 1] = ((const T*)g.uv_b)[2 * row + 1];
            return 0;
        });
        g.X[3 * pos] = g.points[3 * row], g.X[3 * pos + 1] = g.points[3 * row + 1], g.X[3 * pos + 2] = g.points[3 * row + 2];
        g.src[pos] = (long long)row;
    }
};

// ---- stage 2: a chunk's part of its pair's reduced system at the current estimate and lambda (FINAL: undamped) ----------
// Where the last step was taken ([ACCEPT] != 0) the point's candidate becomes the point first; k_bundle_update has
// already moved the views.
template <bool FINAL>
__global__ __launch_bounds__(256) void k_bundle_linearise(BundleArgs g)
{
    __shared__ double sh[4 * 36];
    const Chunk k = chunk_of(g, blockIdx.x);
    const double lambda = FINAL ? 0. : g.state[BS_LAMBDA];
    View qa, qb;
    load_view(g.state, BS_POSES, k.a, qa);
    load_view(g.state, BS_POSES, k.b, qb);
    double X[3] = {0., 0., 1.}, ua[2] = {0., 0.}, ub[2] = {0., 0.};
    if (k.on) {
        const bool moved = g.state[BS_ACCEPT] != 0.;
        load_used(g, k.at, moved ? g.Xc : g.X, X, ua, ub);
        if (moved) g.X[3 * k.at] = X[0], g.X[3 * k.at + 1] = X[1], g.X[3 * k.at + 2] = X[2];
    }
    double* out = g.partials + (size_t)blockIdx.x * BUNDLE_PARTIAL;
    auto sel = [&](double v) { return k.on ? v : 0.; };  // (a lane without a point adds exact zeros)
    {  // pass 1: S_aa, g_a, diag U_a, the cost, the points whose block did not factor
        double s[35] = {};
        PointTerms o;
        point_terms(qa, qb, X, ua, ub, lambda, o);
#pragma unroll
        for (int p = 0; p < 6; p++) {
#pragma unroll
            for (int q = 0; q <= p; q++)
                s[p * (p + 1) / 2 + q] = sel(((o.Ja[0][p] * o.Ja[0][q] + o.Ja[1][p] * o.Ja[1][q]) -
                                               (o.Za[0][p] * o.Za[0][q] + o.Za[1][p] * o.Za[1][q] + o.Za[2][p] * o.Za[2][q])));
            s[21 + p] = sel(((o.Ja[0][p] * o.ra[0] + o.Ja[1][p] * o.ra[1]) - (o.Za[0][p] * o.y[0] + o.Za[1][p] * o.y[1] + o.Za[2][p] * o.y[2])));
            s[27 + p] = sel((o.Ja[0][p] * o.Ja[0][p] + o.Ja[1][p] * o.Ja[1][p]));
        }
        s[33] = sel(((o.ra[0] * o.ra[0] + o.ra[1] * o.ra[1]) + (o.rb[0] * o.rb[0] + o.rb[1] * o.rb[1])));
        s[34] = k.on && !o.ok ? 1. : 0.;
        const double v = block_sums<35>(s, sh);
        const int t = threadIdx.x;
        if (t < 21) out[BP_AA + t] = v;
        else if (t < 27) out[BP_GA + t - 21] = v;
        else if (t < 33) out[BP_DA + t - 27] = v;
        else if (t == 33) out[BP_COST] = v;
        else if (t == 34) out[BP_BAD] = v;
    }
    {  // pass 2: S_bb, g_b, diag U_b
        double s[33] = {};
        PointTerms o;
        point_terms(qa, qb, X, ua, ub, lambda, o);
#pragma unroll
        for (int p = 0; p < 6; p++) {
#pragma unroll
            for (int q = 0; q <= p; q++)
                s[p * (p + 1) / 2 + q] = sel(((o.Jb[0][p] * o.Jb[0][q] + o.Jb[1][p] * o.Jb[1][q]) -
                                               (o.Zb[0][p] * o.Zb[0][q] + o.Zb[1][p] * o.Zb[1][q] + o.Zb[2][p] * o.Zb[2][q])));
            s[21 + p] = sel(((o.Jb[0][p] * o.rb[0] + o.Jb[1][p] * o.rb[1]) - (o.Zb[0][p] * o.y[0] + o.Zb[1][p] * o.y[1] + o.Zb[2][p] * o.y[2])));
            s[27 + p] = sel((o.Jb[0][p] * o.Jb[0][p] + o.Jb[1][p] * o.Jb[1][p]));
        }
        const double v = block_sums<33>(s, sh);
        const int t = threadIdx.x;
        if (t < 21) out[BP_BB + t] = v;
        else if (t < 27) out[BP_GB + t - 21] = v;
        else if (t < 33) out[BP_DB + t - 27] = v;
    }
    {  // pass 3: S_ba (row: view b, column: view a)
        double s[36] = {};
        PointTerms o;
        point_terms(qa, qb, X, ua, ub, lambda, o);
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = 0; q < 6; q++) s[p * 6 + q] = sel(-(o.Zb[0][p] * o.Za[0][q] + o.Zb[1][p] * o.Za[1][q] + o.Zb[2][p] * o.Za[2][q]));
        const double v = block_sums<36>(s, sh);
        if (threadIdx.x < 36) out[BP_BA + threadIdx.x] = v;
    }
}

// the second level: one wavefront per pair adds its chunks' partials, lane l those of chunks l, l + 64, ... in rising order,
// then the butterfly.  Q doubles per partial, summed eight at a time.
template <int Q>
__global__ __launch_bounds__(64) void k_bundle_pair_sum(BundleArgs g, const double* __restrict__ partials, double* __restrict__ blocks)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    long long c0 = g.pair_chunk[p], c1 = g.pair_chunk[p + 1];
    if (c0 < 0 || c1 > g.chunks || c1 < c0) c0 = c1 = 0;
#pragma unroll 1
    for (int base = 0; base < Q; base += 8) {
        double s[8] = {};
        for (long long c = c0 + lane; c < c1; c += 64) {
            const double* o = partials + (size_t)c * Q + base;
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (base + q < Q) s[q] += o[q];
        }
        wave_sum_all<8>(s);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (base + q < Q) blocks[(size_t)p * Q + base + q] = s[q];
        }
    }
}

// ---- stage 3: the reduced system of all views, in LDS ------------------------------------------------------------------
constexpr int BUNDLE_DIM = 6 * BUNDLE_MAX_VIEWS;
__device__ __forceinline__ int tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// the anchor's x = M y: (w, d) from (w, e), M = [I 0; -[t]x -R]
__device__ __forceinline__ void anchor_matrix(const double* R, const double* t, double M[6][6])
{
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) M[i][j] = i == j && i < 3 ? 1. : 0.;
    M[3][1] = t[2], M[3][2] = -t[1], M[4][0] = -t[2], M[4][2] = t[0], M[5][0] = t[1], M[5][1] = -t[0];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[3 + i][3 + j] = -R[3 * i + j];
}

template <bool FINAL>
__global__ __launch_bounds__(256) void k_bundle_solve(BundleArgs g)
{
    __shared__ double A[BUNDLE_DIM * (BUNDLE_DIM + 1) / 2];
    __shared__ double rhs[BUNDLE_DIM], dU[BUNDLE_DIM], B[6][BUNDLE_DIM], C[6][BUNDLE_DIM], Mx[6][6], scalars[4];
    __shared__ int idx[BUNDLE_DIM];
    __shared__ int flags[2];
    const int t = threadIdx.x, n6 = 6 * g.views;
    const int fixed = (int)g.state[BS_FIXED], anchor = (int)g.state[BS_ANCHOR], axis = (int)g.state[BS_AXIS];
    const bool gauge = fixed >= 0 && fixed < g.views && anchor >= 0 && anchor < g.views && anchor != fixed && axis >= 0 && axis < 3;
    for (int e = t; e < n6 * (n6 + 1) / 2; e += 256) A[e] = 0.;
    for (int e = t; e < n6; e += 256) rhs[e] = 0., dU[e] = 0.;
    if (t < 4) scalars[t] = 0.;  // the cost, the points that did not factor, 1 / the current pivot's root, the smallest pivot
    if (t == 0) flags[0] = gauge ? 1 : 0;
    __syncthreads();
    // the pairs' blocks in rising pair order; a pair touches every place at most once
    for (int p = 0; p < g.pairs; p++) {
        const int a = g.pair_views[2 * p], b = g.pair_views[2 * p + 1];
        if (a < 0 || b <= a || b >= g.views) continue;
        const double* o = g.pairblk + (size_t)p * BUNDLE_PARTIAL;
        if (t < 21 || (t >= 21 && t < 42)) {
            const int v = t < 21 ? a : b, e = t < 21 ? t : t - 21;
            int i = 0;
            while ((i + 1) * (i + 2) / 2 <= e) i++;
            const int j = e - i * (i + 1) / 2;
            A[tri(6 * v + i, 6 * v + j)] += o[t];
        } else if (t < 78) {
            const int e = t - 42;
            A[tri(6 * b + e / 6, 6 * a + e % 6)] += o[t];
        } else if (t < 84) rhs[6 * a + t - 78] += o[t];
        else if (t < 90) rhs[6 * b + t - 84] += o[t];
        else if (t < 96) dU[6 * a + t - 90] += o[t];
        else if (t < 102) dU[6 * b + t - 96] += o[t];
        else if (t == 102) scalars[0] += o[t];
        else if (t == 103) scalars[1] += o[t];
        __syncthreads();
    }
    if (!FINAL) {
        const double lambda = g.state[BS_LAMBDA];
        for (int e = t; e < n6; e += 256) A[tri(e, e)] += lambda * dU[e];
    }
    if (t < 36 && gauge) {
        double R[9], tt[3], M[6][6];
        load_pose(g.state + BS_POSES + 12 * anchor, R, tt);
        anchor_matrix(R, tt, M);
        Mx[t / 6][t % 6] = M[t / 6][t % 6];
    }
    __syncthreads();
    if (gauge) {
        // the anchor's rows and columns: M^T A M, M^T rhs
        const int a0 = 6 * anchor;
        for (int e = t; e < 6 * n6; e += 256) B[e / n6][e % n6] = A[tri(a0 + e / n6, e % n6)];
        __syncthreads();
        for (int e = t; e < 6 * n6; e += 256) {
            const int k = e / n6, j = e % n6;
            double s = 0.;
            for (int m = 0; m < 6; m++) s += Mx[m][k] * B[m][j];
            C[k][j] = s;
        }
        __syncthreads();
        for (int e = t; e < 6 * n6; e += 256) {
            const int k = e / n6, j = e % n6;
            if (j < a0 || j >= a0 + 6) A[tri(a0 + k, j)] = C[k][j];
        }
        if (t < 36 && t % 6 <= t / 6) {
            const int k = t / 6, l = t % 6;
            double s = 0.;
            for (int m = 0; m < 6; m++) s += C[k][a0 + m] * Mx[m][l];
            A[tri(a0 + k, a0 + l)] = s;
        }
        double r6 = 0.;
        if (t < 6)
            for (int m = 0; m < 6; m++) r6 += Mx[m][t] * rhs[a0 + m];
        __syncthreads();
        if (t < 6) rhs[a0 + t] = r6;
    }
    // the kept rows
    if (t == 0) {
        int n = 0;
        for (int e = 0; e < n6; e++)
            if (gauge && e / 6 != fixed && e != 6 * anchor + 3 + axis) idx[n++] = e;
        flags[1] = n;
        scalars[3] = INFINITY;
    }
    __syncthreads();
    const int n = flags[1];
    if (FINAL) {  // scaled to a unit diagonal
        for (int e = t; e < n; e += 256) dU[e] = __ddiv_rn(1., sqrt(A[tri(idx[e], idx[e])]));
        __syncthreads();
        for (int i = t; i < n; i += 256)
            for (int j = 0; j <= i; j++) A[tri(idx[i], idx[j])] *= dU[i] * dU[j];
        __syncthreads();
    }
    // Cholesky in place, right-looking: element (i, k) takes its subtractions for j = 0, 1, ... in that order
    for (int j = 0; j < n; j++) {
        if (t == 0) {
            const double d = A[tri(idx[j], idx[j])];
            if (!(d > 0. && isfinite(d))) flags[0] = 0;
            scalars[3] = d < scalars[3] ? d : scalars[3];
            const double r = sqrt(d);
            A[tri(idx[j], idx[j])] = r;
            scalars[2] = __ddiv_rn(1., r);
        }
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += 256) A[tri(idx[i], idx[j])] *= scalars[2];
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += 256) {
            const double lij = A[tri(idx[i], idx[j])];
            for (int k = j + 1; k <= i; k++) A[tri(idx[i], idx[k])] -= lij * A[tri(idx[k], idx[j])];
        }
        __syncthreads();
    }
    if (FINAL) {
        if (t == 0) {
            const double cost = scalars[0], pivot = n > 0 ? scalars[3] : NAN;
            const bool good = flags[0] != 0 && n > 0 && scalars[1] == 0. && pivot >= SINGULAR_PIVOT && isfinite(cost) &&
                              g.state[BS_CONVERGED] != 0.;
            g.state[BS_STATUS] = good ? 0. : 3.;
            g.state[BS_PIVOT] = pivot;
            g.state[BS_COST] = cost;
            g.state[BS_ACCEPT] = 0.;  // (the points have taken their candidates in k_bundle_linearise)
        }
        for (int p = t; p < g.pairs; p += 256) {
            const long long c0 = g.pair_chunk[p], c1 = g.pair_chunk[p + 1];
            long long m = 0;
            if (c0 >= 0 && c1 <= g.chunks)
                for (long long c = c0; c < c1; c++) m += g.chunk_table[4 * c + 2];
            g.pair_error[p] = m > 0 ? sqrt(__ddiv_rn(g.pairblk[(size_t)p * BUNDLE_PARTIAL + BP_COST], 2. * (double)m)) : NAN;
        }
        return;
    }
    // L L^T x = -rhs: column by column; x[i] takes its subtractions in rising j (forward) and falling j (backward)
    for (int e = t; e < n; e += 256) dU[e] = -rhs[idx[e]];
    __syncthreads();
    for (int j = 0; j < n; j++) {
        if (t == 0) dU[j] = __ddiv_rn(dU[j], A[tri(idx[j], idx[j])]);
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += 256) dU[i] -= A[tri(idx[i], idx[j])] * dU[j];
        __syncthreads();
    }
    for (int j = n - 1; j >= 0; j--) {
        if (t == 0) dU[j] = __ddiv_rn(dU[j], A[tri(idx[j], idx[j])]);
        __syncthreads();
        for (int i = t; i < j; i += 256) dU[i] -= A[tri(idx[j], idx[i])] * dU[j];
        __syncthreads();
    }
    // back to every view's (w, d): zero where held, M y for the anchor
    for (int e = t; e < n6; e += 256) rhs[e] = 0.;
    if (t == 0) {
        bool ok = flags[0] != 0 && n > 0 && scalars[1] == 0.;
        for (int e = 0; e < n; e++) ok = ok && isfinite(dU[e]);
        flags[0] = ok ? 1 : 0;
    }
    __syncthreads();
    const bool ok = flags[0] != 0;
    for (int e = t; e < n; e += 256) rhs[idx[e]] = ok ? dU[e] : 0.;
    __syncthreads();
    if (t < g.views) {
        double R[9], tt[3], R2[9], t2[3], y[6], x[6];
        load_pose(g.state + BS_POSES + 12 * t, R, tt);
        for (int q = 0; q < 6; q++) y[q] = rhs[6 * t + q], x[q] = y[q];
        rotate_left(y, R, R2);
        if (gauge && t == anchor) {
            double c2[3];
            for (int j = 0; j < 3; j++) c2[j] = -(R[j] * tt[0] + R[3 + j] * tt[1] + R[6 + j] * tt[2]) + y[3 + j];
            for (int i = 0; i < 3; i++) t2[i] = -(R2[3 * i] * c2[0] + R2[3 * i + 1] * c2[1] + R2[3 * i + 2] * c2[2]);
            for (int i = 0; i < 6; i++) {
                double s = 0.;
                for (int m = 0; m < 6; m++) s += Mx[i][m] * y[m];
                x[i] = s;
            }
        } else {
            t2[0] = tt[0] + y[3], t2[1] = tt[1] + y[4], t2[2] = tt[2] + y[5];
        }
        store_pose(g.state + BS_CAND + 12 * t, R2, t2);
        for (int q = 0; q < 6; q++) g.state[BS_STEP + 6 * t + q] = x[q];
    }
    if (t == 0) {
        g.state[BS_SOLVED] = ok ? 1. : 0.;
        g.state[BS_COST] = scalars[0];
    }
}

// ---- stage 4: every point's own step and candidate, the cost under the candidate poses ---------------------------------
__global__ __launch_bounds__(256) void k_bundle_evaluate(BundleArgs g)
{
    __shared__ double sh[4 * 4];
    if (g.state[BS_SOLVED] == 0.) return;  // no step: k_bundle_update rejects (the whole workgroup leaves)
    const Chunk k = chunk_of(g, blockIdx.x);
    View qa, qb;
    load_view(g.state, BS_POSES, k.a, qa);
    load_view(g.state, BS_POSES, k.b, qb);
    double X[3] = {0., 0., 1.}, ua[2] = {0., 0.}, ub[2] = {0., 0.}, s[4] = {};
    if (k.on) load_used(g, k.at, g.X, X, ua, ub);
    PointTerms o;
    point_terms(qa, qb, X, ua, ub, g.state[BS_LAMBDA], o);
    const double *da = g.state + BS_STEP + 6 * k.a, *db = g.state + BS_STEP + 6 * k.b;
    double r[3], d[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        double sa = 0., sb = 0.;
#pragma unroll
        for (int p = 0; p < 6; p++) sa += o.Za[q][p] * da[p], sb += o.Zb[q][p] * db[p];
        r[q] = -(o.y[q] + (sa + sb));
    }
    d[2] = r[2] * o.il[2];
    d[1] = (r[1] - o.L[4] * d[2]) * o.il[1];
    d[0] = (r[0] - o.L[1] * d[1] - o.L[3] * d[2]) * o.il[0];
    const double Y[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
    load_view(g.state, BS_CAND, k.a, qa);
    load_view(g.state, BS_CAND, k.b, qb);
    double ra[2], rb[2];
    const double za = observe<false>(qa, Y, ua, ra, nullptr, nullptr), zb = observe<false>(qb, Y, ub, rb, nullptr, nullptr);
    if (k.on) {
        g.Xc[3 * k.at] = Y[0], g.Xc[3 * k.at + 1] = Y[1], g.Xc[3 * k.at + 2] = Y[2];
        const double c = (ra[0] * ra[0] + ra[1] * ra[1]) + (rb[0] * rb[0] + rb[1] * rb[1]);
        const bool good = o.ok && za > 0. && zb > 0. && isfinite(c);
        s[BE_COST] = good ? c : 0.;
        s[BE_STEP] = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        s[BE_NORM] = X[0] * X[0] + X[1] * X[1] + X[2] * X[2];
        s[BE_BAD] = good ? 0. : 1.;
    }
    const double v = block_sums<4>(s, sh);
    if (threadIdx.x < 4) g.epartials[(size_t)blockIdx.x * BUNDLE_EVAL + threadIdx.x] = v;
}

// ---- stage 5: accept or reject, lambda, the stop (one wavefront) --------------------------------------------------------
__global__ __launch_bounds__(64) void k_bundle_update(BundleArgs g, int max_evaluations)
{
    const int lane = threadIdx.x;
    const bool solved = g.state[BS_SOLVED] != 0.;
    double s[4] = {};
    if (solved)
        for (int p = lane; p < g.pairs; p += 64) {
#pragma unroll
            for (int q = 0; q < 4; q++) s[q] += g.epairblk[(size_t)p * BUNDLE_EVAL + q];
        }
    wave_sum_all<4>(s);
    double step = s[BE_STEP], norm = s[BE_NORM];
    for (int v = 0; v < g.views; v++) {
        for (int q = 0; q < 6; q++) step += g.state[BS_STEP + 6 * v + q] * g.state[BS_STEP + 6 * v + q];
        norm += pose_norm2(g.state + BS_POSES + 12 * v + 9);
    }
    const double c = g.state[BS_COST], c2 = s[BE_BAD] == 0. ? s[BE_COST] : INFINITY;  // a point behind a view: infinite
    const bool better = lm_update(g.state, lane, solved, c, c2, step, norm, max_evaluations);
    if (lane == 0 && g.state[BS_EVALS] == 1.) g.state[BS_COST0] = c;  // (the count lm_update has just written)
    if (better)
        for (int e = lane; e < 12 * g.views; e += 64) g.state[BS_POSES + e] = g.state[BS_CAND + e];
}

// ---- stage 6: the points back to their rows, and every used point's depth in both of its views ------------------------
__global__ __launch_bounds__(256) void k_bundle_rows(BundleArgs g)
{
    const Chunk k = chunk_of(g, blockIdx.x);
    if (!k.on) return;
    View qa, qb;
    load_view(g.state, BS_POSES, k.a, qa);
    load_view(g.state, BS_POSES, k.b, qb);
    double X[3], ua[2], ub[2], ra[2], rb[2];
    load_used(g, k.at, g.X, X, ua, ub);
    const double za = observe<false>(qa, X, ua, ra, nullptr, nullptr), zb = observe<false>(qb, X, ub, rb, nullptr, nullptr);
    const long long row = g.src[k.at];
    if (row >= 0 && row < g.matches) g.points[3 * row] = X[0], g.points[3 * row + 1] = X[1], g.points[3 * row + 2] = X[2];
    if (g.rows_a && g.rows_b) {
        double *oa = g.rows_a + 4 * k.at, *ob = g.rows_b + 4 * k.at;
        oa[0] = ua[0], oa[1] = ua[1], oa[2] = za, oa[3] = g.state[BS_LABEL + k.b];
        ob[0] = ub[0], ob[1] = ub[1], ob[2] = zb, ob[3] = g.state[BS_LABEL + k.a];
    }
}

static bool aligned(const void* p, size_t a) { return p && (uintptr_t)p % a == 0; }

enum { NEED_MATCHES = 1, NEED_USED = 2 };
static int bundle_args(const char* who, const camd_bundle* b, int needs, BundleArgs& a)
{
    const bool head = b && b->views >= 3 && b->views <= BUNDLE_MAX_VIEWS && b->pairs >= 1 &&
                      b->pairs <= BUNDLE_MAX_VIEWS * (BUNDLE_MAX_VIEWS - 1) / 2 && float_type_ok(b->uv_type) && b->matches >= 1 &&
                      b->matches < (1ll << 31) && b->segments >= 1 && aligned(b->pair_views, 4) && aligned(b->pair_start, 8) &&
                      aligned(b->seg_first, 8) && aligned(b->seg_n, 4) && aligned(b->status, 4) && doubles_ok(b->points) &&
                      aligned(b->rowoff, 8) && aligned(b->rowcount, 4) && doubles_ok(b->state);
    const size_t e = b && b->uv_type == CAMD_VALUE_F64 ? 8 : 4;
    const bool matches = !(needs & NEED_MATCHES) || (head && aligned(b->uv_a, e) && aligned(b->uv_b, e));
    const bool used = !(needs & NEED_USED) ||
                      (head && b->used >= 1 && b->used <= b->matches && b->chunks >= 1 && aligned(b->uv_used_a, e) && aligned(b->uv_used_b, e) &&
                       doubles_ok(b->X) && doubles_ok(b->candidate) && aligned(b->src, 8) && aligned(b->chunk_table, 4) &&
                       aligned(b->pair_chunk, 8) && doubles_ok(b->partials) && doubles_ok(b->pair_blocks) &&
                       doubles_ok(b->eval_partials) && doubles_ok(b->eval_blocks) && doubles_ok(b->pair_error) &&
                       (!b->rows_a) == (!b->rows_b) && (!b->rows_a || (doubles_ok(b->rows_a) && doubles_ok(b->rows_b))));
    if (!head || !matches || !used) {
        set_error("%s: bad arguments (views 3 .. %d, pairs 1 .. views (views - 1) / 2, 1 <= matches < 2^31, uv_type float32 / "
                  "float64, every array of include/calibrating_amd.h's camd_bundle on the device and aligned to its element)",
                  who, BUNDLE_MAX_VIEWS);
        return CAMD_ERR_BAD_ARG;
    }
    a.uv_a = b->uv_a, a.uv_b = b->uv_b, a.uv_type = b->uv_type, a.views = b->views, a.pairs = b->pairs, a.segments = b->segments;
    a.chunks = b->chunks, a.matches = b->matches, a.used = b->used;
    a.threshold2 = b->threshold >= 0. ? b->threshold * b->threshold : -1.;
    a.pair_views = b->pair_views, a.pair_start = b->pair_start, a.seg_first = b->seg_first, a.seg_n = b->seg_n;
    a.chunk_table = b->chunk_table, a.pair_chunk = b->pair_chunk, a.status = b->status, a.points = b->points;
    a.rowoff = b->rowoff, a.rowcount = b->rowcount, a.cuv_a = b->uv_used_a, a.cuv_b = b->uv_used_b, a.X = b->X, a.Xc = b->candidate;
    a.src = b->src, a.partials = b->partials, a.pairblk = b->pair_blocks, a.epartials = b->eval_partials;
    a.epairblk = b->eval_blocks, a.state = b->state, a.pair_error = b->pair_error, a.rows_a = b->rows_a, a.rows_b = b->rows_b;
    return CAMD_OK;
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_bundle_start(const camd_bundle* bundle, long long max_pair_rows, void* queue)
{
    BundleArgs a = {};
    int rc = bundle_args("camd_bundle_start", bundle, NEED_MATCHES, a);
    if (rc != CAMD_OK) return rc;
    if (max_pair_rows < 1 || max_pair_rows > a.matches) {
        set_error("camd_bundle_start: max_pair_rows is the largest pair's rows, 1 .. matches, got %lld", max_pair_rows);
        return CAMD_ERR_BAD_ARG;
    }
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    hipLaunchKernelGGL(k_bundle_start, dim3(div_up(max_pair_rows, 256), a.pairs), dim3(256), 0, st, a);
    CAMD_LAUNCH_CHECK();
    row_count(BundleUsed{a}, BUNDLE_SEGMENT, a.segments, a.rowcount, st);
    CAMD_LAUNCH_CHECK();
    row_scan(a.rowcount, a.segments, a.rowoff, a.rowoff + a.segments, st);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_bundle_emit(const camd_bundle* bundle, void* queue)
{
    BundleArgs a = {};
    int rc = bundle_args("camd_bundle_emit", bundle, NEED_MATCHES | NEED_USED, a);
    if (rc != CAMD_OK) return rc;
    CAMD_NEED_DEVICE();
    row_emit(BundleUsed{a}, BUNDLE_SEGMENT, a.segments, a.rowoff, (size_t)a.used, nullptr, (hipStream_t)queue);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_bundle_step(const camd_bundle* bundle, void* queue)
{
    BundleArgs a = {};
    int rc = bundle_args("camd_bundle_step", bundle, NEED_USED, a);
    if (rc != CAMD_OK) return rc;
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    hipLaunchKernelGGL(k_bundle_linearise<false>, dim3(a.chunks), dim3(256), 0, st, a);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bundle_pair_sum<BUNDLE_PARTIAL>, dim3(a.pairs), dim3(64), 0, st, a, (const double*)a.partials, a.pairblk);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bundle_solve<false>, dim3(1), dim3(256), 0, st, a);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bundle_evaluate, dim3(a.chunks), dim3(256), 0, st, a);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bundle_pair_sum<BUNDLE_EVAL>, dim3(a.pairs), dim3(64), 0, st, a, (const double*)a.epartials, a.epairblk);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bundle_update, dim3(1), dim3(64), 0, st, a, BUNDLE_MAX_EVALUATIONS);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_bundle_finish(const camd_bundle* bundle, void* queue)
{
    BundleArgs a = {};
    int rc = bundle_args("camd_bundle_finish", bundle, NEED_USED, a);
    if (rc != CAMD_OK) return rc;
    CAMD_NEED_DEVICE();
    hipStream_t st = (hipStream_t)queue;
    hipLaunchKernelGGL(k_bundle_linearise<true>, dim3(a.chunks), dim3(256), 0, st, a);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bundle_pair_sum<BUNDLE_PARTIAL>, dim3(a.pairs), dim3(64), 0, st, a, (const double*)a.partials, a.pairblk);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bundle_solve<true>, dim3(1), dim3(256), 0, st, a);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bundle_rows, dim3(a.chunks), dim3(256), 0, st, a);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
