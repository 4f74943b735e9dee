// calibrate.hip -- a camera's intrinsics and the target's pose in every frame from detected points.
//
// Replaces (file:line in the reference's calibrating/):
//   camera.py:63-93   cv2.calibrateCamera(object_points, image_points, xy, None, None, flags) -> retval, K, D, rvecs, tvecs
// for the 5-coefficient model (fx fy cx cy | k1 k2 p1 p2 k3).  A bundle adjustment whose normal matrix is an arrow: six
// unknowns per frame (pnp.hip's local perturbation R <- exp([w]x) R, t <- t + d) and one block of nine shared by all
// frames.  Per frame i the sums over its points are A_i (6 x 6), B_i (6 x 9), C_i (9 x 9), gp_i, gk_i, c_i: 136 doubles in
// the workspace.  The block is solved from the reduced system
//   sum_i (C_i - B_i^T (A_i + l diag A_i)^-1 B_i) + l diag sum_i C_i,
// and every frame's step follows by back-substitution.
//
// Shared with stereo_calibrate.hip, in joint_common.hpp: the frame's workspace (ArrowBlock<9>), its three passes over the
// points (arrow_linearise), its back-substitution (arrow_frame_step), its candidate row, and the accept / damp / stop
// bookkeeping (lm_update, bundle.hip's too).  Kept here: point_terms (the Jacobian in the intrinsics), the single-level
// sum over frames with the frame's Schur nest written out in k_calib_solve (arrow_frame_schur's, accumulating), the
// block's solve with its mask and the order of FINAL's scaling, the move of the poses and of K in the update, the
// start's homographies.
//
// Kernels.  k_calib_linearise and k_calib_evaluate sum over a frame's points: one wavefront per frame, four frames per
// workgroup, no workgroup barrier, the butterfly of pnp_common.hpp.  k_calib_solve and k_calib_update sum over FRAMES: one
// wavefront, lane l takes frames l, l + 64, ... in rising order, then the same butterfly -- a fixed order without atomics,
// so the same input gives the same bits on every run.  Lambda, the costs, the accept decision, both parameter sets and
// the stop flag live in `state` on the device; the host reads two numbers per evaluation.
//
// cv2's own iteration is UNPINNED.
#include "joint_common.hpp"

namespace camd {

constexpr int CALIB_MAX_EVALUATIONS = 100;      // every case of tests/calibrate_cases.py ends below half of it
constexpr int CALIB_WS = CAMD_CALIB_WORKSPACE_DOUBLES, CALIB_CAND = CAMD_CALIB_CANDIDATE_DOUBLES;
using WS = ArrowBlock<9>;  // the workspace of one frame
// the state beyond lm_update's places (doubles; include/calibrating_amd.h names the places the host reads and writes)
enum {
    CS_LAMBDA = CAMD_CALIB_LAMBDA, CS_COST = CAMD_CALIB_COST, CS_STATUS = CAMD_CALIB_STATUS, CS_CONVERGED = CAMD_CALIB_CONVERGED,
    CS_K = CAMD_CALIB_K, CS_DK = CAMD_CALIB_DK, CS_MASK = CAMD_CALIB_MASK, CS_SOLVED = CAMD_CALIB_SOLVED, CS_PIVOT = CAMD_CALIB_PIVOT
};

struct CalibArgs {
    camd_pnp_points p;
    const int* used;  // the frames of the joint problem, rising
    int used_n;
    double* state;
    double* poses;  // used_n x 12: R, t of the current estimate
    double* cand;   // used_n x 16: R, t of the candidate, its cost, |step|^2, |parameters|^2
    double* ws;     // used_n x 136
    double* error;  // used_n: sqrt(c_i / n_i)
};

__device__ __forceinline__ void load_intrinsics(const double* k, Pinhole& cam, Lens& lens)
{
    cam = {k[0], k[1], k[2], k[3], 0., 0.};
    lens = {k[4], k[5], k[6], k[7], k[8], 0., 0., 0., 0., 0., 0., 0.};
}

// one point under R, t, cam, lens: pose_terms' residual r and 2 x 6 Jacobian Jp with respect to the pose, and the 2 x 9
// Jacobian Jk with respect to fx fy cx cy k1 k2 p1 p2 k3; returned: the point's cost |r|^2
using PointTerms = ArrowTerms<9, false>;
__device__ __forceinline__ double point_terms(const camd_pnp_points& p, const Frame& fr, int i, const Pinhole& cam, const Lens& k,
                                              const double* R, const double* t, PointTerms& o)
{
    const Projected n = pose_terms(p, fr, i, cam, k, R, t, o.r, o.Jp);
    const double x = n.x, y = n.y, xd = n.xd, yd = n.yd;
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
    o.Jk[0][0] = xd, o.Jk[0][1] = 0., o.Jk[0][2] = 1., o.Jk[0][3] = 0.;
    o.Jk[1][0] = 0., o.Jk[1][1] = yd, o.Jk[1][2] = 0., o.Jk[1][3] = 1.;
    o.Jk[0][4] = cam.fx * (x * r2), o.Jk[0][5] = cam.fx * (x * r4), o.Jk[0][6] = cam.fx * a1, o.Jk[0][7] = cam.fx * a2;
    o.Jk[0][8] = cam.fx * (x * r6);
    o.Jk[1][4] = cam.fy * (y * r2), o.Jk[1][5] = cam.fy * (y * r4), o.Jk[1][6] = cam.fy * a3, o.Jk[1][7] = cam.fy * a1;
    o.Jk[1][8] = cam.fy * (y * r6);
    return o.r[0] * o.r[0] + o.r[1] * o.r[1];
}

// ---- the sums over a frame's points -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_calib_linearise(CalibArgs a)
{
    const int lane = threadIdx.x & 63, u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= a.used_n) return;  // (the whole wave; there is no barrier to miss)
    const Frame fr = used_frame(a.p, a.used, u);
    Pinhole cam;
    Lens k;
    load_intrinsics(a.state + CS_K, cam, k);
    double R[9], t[3];
    load_pose(a.poses + (size_t)u * 12, R, t);
    arrow_linearise<9, false>([&](int i, PointTerms& o) { return point_terms(a.p, fr, i, cam, k, R, t, o); }, fr.n, lane,
                              a.ws + (size_t)u * CALIB_WS);
}

// the candidate of one frame: its step by back-substitution from the block's step, its pose, and the cost there
__global__ __launch_bounds__(256) void k_calib_evaluate(CalibArgs a)
{
    const int lane = threadIdx.x & 63, u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= a.used_n) return;
    if (!uniform(a.state[CS_SOLVED] != 0.)) return;  // no step: k_calib_update rejects
    const Frame fr = used_frame(a.p, a.used, u);
    double d[6], k2[9], t[3], R2[9], t2[3];
    arrow_frame_step<9>(a.ws + (size_t)u * CALIB_WS, a.state[CS_LAMBDA], a.state + CS_DK, a.poses + (size_t)u * 12, d, t, R2, t2);
#pragma unroll
    for (int q = 0; q < 9; q++) k2[q] = a.state[CS_K + q] + a.state[CS_DK + q];
    Pinhole cam;
    Lens k;
    load_intrinsics(k2, cam, k);
    double c = 0.;
    for (int i = lane; i < fr.n; i += 64) {
        PointTerms o;
        c += point_terms(a.p, fr, i, cam, k, R2, t2, o);
    }
    c = wave_sum(c);
    if (lane == 0) arrow_candidate_store(a.cand + (size_t)u * CALIB_CAND, R2, t2, c, d, t);
}

// ---- the sums over frames: one wavefront ---------------------------------------------------------------------------
// The reduced system of the block for the current lambda and its step (FINAL = false); or, once the iteration has ended,
// the undamped reduced matrix scaled to a unit diagonal, its smallest pivot, the camera's status, the cost and every
// frame's error (FINAL = true).
template <bool FINAL>
__global__ __launch_bounds__(64) void k_calib_solve(CalibArgs a)
{
    const int lane = threadIdx.x;
    const double lambda = FINAL ? 0. : a.state[CS_LAMBDA];
    double S[45] = {}, g[9] = {}, dC[9] = {}, cost = 0.;
    int bad = 0;
    for (int u = lane; u < a.used_n; u += 64) {
        const double* w = a.ws + (size_t)u * CALIB_WS;
        // arrow_frame_schur's nest, adding each finished number where it is made (joint_common.hpp says why it is not called)
        double L[21], y[6], frame_pivot;
        damped<6>(w + WS::A, lambda, L);
        bad |= !cholesky<6>(L, frame_pivot);
#pragma unroll
        for (int p = 0; p < 6; p++) y[p] = w[WS::GP + p];
        cholesky_solve<6>(L, y);
#pragma unroll
        for (int q = 0; q < 9; q++) {
            double s = w[WS::GK + q];
#pragma unroll
            for (int p = 0; p < 6; p++) s -= w[WS::B + p * 9 + q] * y[p];
            g[q] += s;
        }
#pragma unroll
        for (int j = 0; j < 9; j++) {
#pragma unroll
            for (int p = 0; p < 6; p++) y[p] = w[WS::B + p * 9 + j];
            cholesky_solve<6>(L, y);
#pragma unroll
            for (int q = 0; q <= j; q++) {
                double s = w[WS::C + j * (j + 1) / 2 + q];
#pragma unroll
                for (int p = 0; p < 6; p++) s -= w[WS::B + p * 9 + q] * y[p];
                S[j * (j + 1) / 2 + q] += s;
            }
            dC[j] += w[WS::C + j * (j + 1) / 2 + j];
        }
        if (FINAL) {
            cost += w[WS::COST];
            const Frame fr = used_frame(a.p, a.used, u);
            a.error[u] = sqrt(__ddiv_rn(w[WS::COST], (double)(fr.n > 0 ? fr.n : 1)));
        }
    }
    wave_sum_all<45>(S);
    wave_sum_all<9>(g);
    wave_sum_all<9>(dC);
    bool ok = wave_or(bad) == 0;
    double scale[9], pivot;
#pragma unroll
    for (int q = 0; q < 9; q++) {
        if (FINAL) scale[q] = __ddiv_rn(1., sqrt(S[q * (q + 1) / 2 + q]));
        else S[q * (q + 1) / 2 + q] += lambda * dC[q];
    }
    // a fixed entry: a unit row and column, a zero right-hand side.  (FINAL is pnp_common.hpp's rank test written out, not
    // unit_diagonal_pivot: the scale comes from the unmasked diagonal and the mask goes over the scaled entries, in this order)
#pragma unroll
    for (int p = 0; p < 9; p++) {
        const bool fp = a.state[CS_MASK + p] == 0.;
#pragma unroll
        for (int q = 0; q <= p; q++) {
            const bool fq = a.state[CS_MASK + q] == 0.;
            double v = S[p * (p + 1) / 2 + q];
            if (FINAL) v = v * scale[p] * scale[q];
            S[p * (p + 1) / 2 + q] = (fp || fq) ? (p == q ? 1. : 0.) : v;
        }
        g[p] = fp ? 0. : -g[p];
    }
    ok = cholesky<9>(S, pivot) && ok;
    if (FINAL) {
        cost = wave_sum(cost);
        if (lane == 0) {
            const bool good = ok && pivot >= SINGULAR_PIVOT && isfinite(cost) && a.state[CS_CONVERGED] != 0.;
            a.state[CS_STATUS] = good ? 0. : 3.;
            a.state[CS_PIVOT] = pivot;
            a.state[CS_COST] = cost;
        }
    } else {
        if (ok) cholesky_solve<9>(S, g);
#pragma unroll
        for (int q = 0; q < 9; q++) ok = ok && isfinite(g[q]);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 9; q++) a.state[CS_DK + q] = ok ? g[q] : 0.;
            a.state[CS_SOLVED] = ok ? 1. : 0.;
        }
    }
}

// accept or reject the candidate, move lambda, decide whether to stop (lm_update); after a step that is taken the frames'
// poses and the intrinsics move here
__global__ __launch_bounds__(64) void k_calib_update(CalibArgs a, int max_evaluations)
{
    const int lane = threadIdx.x;
    const bool solved = a.state[CS_SOLVED] != 0.;
    double c = 0., c2 = 0., step = 0., norm = 0.;
    for (int u = lane; u < a.used_n; u += 64) {
        c += a.ws[(size_t)u * CALIB_WS + WS::COST];
        if (solved) {
            const double* o = a.cand + (size_t)u * CALIB_CAND;
            c2 += o[12], step += o[13], norm += o[14];
        }
    }
    c = wave_sum(c), c2 = wave_sum(c2), step = wave_sum(step), norm = wave_sum(norm);
    double k[9], dk[9];
#pragma unroll
    for (int q = 0; q < 9; q++) {
        k[q] = a.state[CS_K + q], dk[q] = a.state[CS_DK + q];
        step += dk[q] * dk[q], norm += k[q] * k[q];
    }
    if (!lm_update(a.state, lane, solved, c, c2, step, norm, max_evaluations)) return;
    for (int u = lane; u < a.used_n; u += 64)
        for (int q = 0; q < 12; q++) a.poses[(size_t)u * 12 + q] = a.cand[(size_t)u * CALIB_CAND + q];
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 9; q++) a.state[CS_K + q] = k[q] + dk[q];
    }
}

// ---- the start: one homography per frame, object plane -> raw pixels ------------------------------------------------
__global__ __launch_bounds__(256) void k_calib_homography(PnpArgs a, double* __restrict__ H)
{
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= a.p.frames) return;
    const Frame fr = frame_rows(a.p, f, a.min_points);
    bool ok = fr.status == PNP_OK && !frame_nonfinite(a.p, fr, lane);
    double G[9], c[3];
    if (uniform(ok)) ok = direct_linear_transform<3>(a, fr, lane, G, c);
    if (lane == 0)
        for (int q = 0; q < 9; q++) H[(size_t)f * 9 + q] = ok ? G[q] : NAN;
}

// the arguments every part of an evaluation shares
static int calib_args(const char* who, const camd_pnp_points* p, const int* used, int used_n, double* state, CalibArgs& a)
{
    if (!points_ok(p) || used_n < 0 || (used_n > 0 && (!used || (uintptr_t)used % 4 != 0 || !doubles_ok(state) || p->frames == 0))) {
        set_error("%s: bad arguments (points as in camd_pnp_init; used: used_n >= 0 device int32, got %d; state: "
                  "CAMD_CALIB_STATE_DOUBLES device doubles)", who, used_n);
        return CAMD_ERR_BAD_ARG;
    }
    a.p = *p, a.used = used, a.used_n = used_n, a.state = state;
    return CAMD_OK;
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_calib_homography(const camd_pnp_points* points, const double plane[9], double* H, void* queue)
{
    if (!points_ok(points) || !plane || (points->frames > 0 && !doubles_ok(H))) {
        set_error("camd_calib_homography: bad arguments (points as in camd_pnp_init; plane: 9 host doubles; H: frames x 9 device "
                  "doubles)");
        return CAMD_ERR_BAD_ARG;
    }
    PnpArgs a = {};
    a.p = *points, a.cam = {1., 1., 0., 0., 1., 1.}, a.planar = 1, a.min_points = 4;  // an identity camera without a lens
    for (int q = 0; q < 9; q++) a.plane[q] = plane[q];
    if (a.p.frames == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_calib_homography, dim3(div_up(a.p.frames, 4)), dim3(256), 0, (hipStream_t)queue, a, H);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_calib_linearise(const camd_pnp_points* points, const int* used, int used_n, double* state, double* poses,
                         double* workspace, void* queue)
{
    CalibArgs a = {};
    int rc = calib_args("camd_calib_linearise", points, used, used_n, state, a);
    if (rc != CAMD_OK) return rc;
    if (used_n > 0 && (!doubles_ok(poses) || !doubles_ok(workspace))) {
        set_error("camd_calib_linearise: bad arguments (poses: used_n x 12, workspace: used_n x 136 device doubles)");
        return CAMD_ERR_BAD_ARG;
    }
    a.poses = poses, a.ws = workspace;
    if (used_n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_calib_linearise, dim3(div_up(used_n, 4)), dim3(256), 0, (hipStream_t)queue, a);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_calib_step(const camd_pnp_points* points, const int* used, int used_n, double* state, double* poses,
                    double* candidate, double* workspace, void* queue)
{
    CalibArgs a = {};
    int rc = calib_args("camd_calib_step", points, used, used_n, state, a);
    if (rc != CAMD_OK) return rc;
    if (used_n > 0 && (!doubles_ok(poses) || !doubles_ok(candidate) || !doubles_ok(workspace))) {
        set_error("camd_calib_step: bad arguments (poses: used_n x 12, candidate: used_n x 16, workspace: used_n x 136 device "
                  "doubles)");
        return CAMD_ERR_BAD_ARG;
    }
    a.poses = poses, a.cand = candidate, a.ws = workspace;
    if (used_n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_calib_solve<false>, dim3(1), dim3(64), 0, (hipStream_t)queue, a);
    hipLaunchKernelGGL(k_calib_evaluate, dim3(div_up(used_n, 4)), dim3(256), 0, (hipStream_t)queue, a);
    hipLaunchKernelGGL(k_calib_update, dim3(1), dim3(64), 0, (hipStream_t)queue, a, CALIB_MAX_EVALUATIONS);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_calib_finish(const camd_pnp_points* points, const int* used, int used_n, double* state, double* workspace,
                      double* frame_error, void* queue)
{
    CalibArgs a = {};
    int rc = calib_args("camd_calib_finish", points, used, used_n, state, a);
    if (rc != CAMD_OK) return rc;
    if (used_n > 0 && (!doubles_ok(workspace) || !doubles_ok(frame_error))) {
        set_error("camd_calib_finish: bad arguments (workspace: used_n x 136, frame_error: used_n device doubles)");
        return CAMD_ERR_BAD_ARG;
    }
    a.ws = workspace, a.error = frame_error;
    if (used_n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_calib_solve<true>, dim3(1), dim3(64), 0, (hipStream_t)queue, a);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_calib_read(const double* state, int count, double* out, void* queue)
{
    if (count < 0 || count > CAMD_CALIB_STATE_DOUBLES || (count > 0 && (!doubles_ok(state) || !out))) {
        set_error("camd_calib_read: bad arguments (state: device doubles; count 0 .. CAMD_CALIB_STATE_DOUBLES, got %d; out: "
                  "count host doubles)", count);
        return CAMD_ERR_BAD_ARG;
    }
    if (count == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    CAMD_HIP(hipMemcpyAsync(out, state, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)queue));
    CAMD_HIP(hipStreamSynchronize((hipStream_t)queue));
    return CAMD_OK;
}

}  // extern "C"
