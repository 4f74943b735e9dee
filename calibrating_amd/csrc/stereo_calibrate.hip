// stereo_calibrate.hip -- a rig's R, t (camera 1 -> camera 2) and the board's pose in every frame from the points both
// cameras detected, with both cameras' intrinsics fixed.
//
// Replaces (file:line in the reference's calibrating/):
//   stereo_camera.py:95-123   cv2.stereoCalibrate(object, image1, image2, K1, D1, K2, D2, xy, flags=CALIB_FIX_INTRINSIC)
// A bundle adjustment whose normal matrix is an arrow, as in calibrate.hip: six unknowns per frame (the board in camera
// 1, pnp.hip's local perturbation R_i <- exp([w_i]x) R_i, t_i <- t_i + d_i) and one block of six shared by all frames (the
// rig, x2 = R x1 + t, R <- exp([w]x) R, t <- t + d).  Camera 1 is the frame of reference: there is no gauge freedom.  Per
// frame i the sums over its points are A_i (6 x 6, both cameras), B_i (6 x 6), C_i (6 x 6, camera 2), gp_i, gr_i, c_i: 91
// doubles in the workspace.  The rig's step is solved from the reduced system
//   sum_i (C_i - B_i^T (A_i + l diag A_i)^-1 B_i) + l diag sum_i C_i,
// and every frame's step follows by back-substitution.
//
// Shared with calibrate.hip, in joint_common.hpp: the frame's workspace (ArrowBlock<6>), its three passes over the points
// (arrow_linearise), its contribution to the reduced system (arrow_frame_schur), its back-substitution
// (arrow_frame_step), its candidate row, and the accept / damp / stop bookkeeping (lm_update, bundle.hip's too).  Kept
// here: rig_terms with compose (two cameras, the Jacobians in the rig), the two-level sum over frames, the rig's solve and
// candidate, the move of the frames' poses in the NEXT linearisation.
//
// Camera 2's terms come from pose_terms at the composed pose (R R_i, R t_i + t), whose 2 x 6 Jacobian J2 = [Jw | Jd] gives
//   with respect to the frame:  [Jw R | Jd R]                    (exp([R w_i]x) R R_i = R exp([w_i]x) R_i)
//   with respect to the rig:    [Jw + (R t_i) x Jd | Jd]         (the rotation also turns R t_i)
// (tests/stereo_calibrate_ref.py checks both against finite differences).
//
// Kernels.  k_stereo_linearise and k_stereo_evaluate sum over a frame's points: one wavefront per frame, four frames per
// workgroup, no workgroup barrier, the butterfly of pnp_common.hpp.  The sums over FRAMES have two levels,
// unlike calibrate.hip's: k_stereo_reduce gives every used frame a lane of its own, which factors the frame's damped
// block and forms its contribution to the reduced system (21 + 6 doubles, diag C_i, the cost); the 64 frames of a
// workgroup are summed by the butterfly into one partial.  k_stereo_solve, one wavefront, then adds the partials -- lane l
// takes partials l, l + 64, ... in rising order, then the butterfly -- and solves the 6 x 6.  It sees used_n / 64 partials
// of 34 doubles and no factorization of a frame.  No atomics: the same input gives the same bits on every run.
// Lambda, the costs, the accept decision, both rigs and the stop flag live in `state` on the device; the host reads two
// numbers per evaluation (camd_calib_read: the first two places of the state are calibrate.hip's).
//
// cv2's own iteration and its 1e-5 stop are UNPINNED.
#include "joint_common.hpp"

namespace camd {

constexpr int STEREO_MAX_EVALUATIONS = 100;  // every case of tests/stereo_calibrate_cases.py ends below half of it
constexpr int STEREO_WS = CAMD_STEREO_WORKSPACE_DOUBLES, STEREO_CAND = CAMD_STEREO_CANDIDATE_DOUBLES;
constexpr int STEREO_PARTIAL = CAMD_STEREO_PARTIAL_DOUBLES;
using WS = ArrowBlock<6>;  // the workspace of one frame
// a partial of the reduced system: S 21, g 6, diag C 6, the cost, then the count of frames whose block did not factor
enum { SP_S = 0, SP_G = 21, SP_DC = 27, SP_COST = 33, SP_BAD = 34 };
// the state beyond lm_update's places (doubles; include/calibrating_amd.h names the places the host reads and writes)
enum {
    SS_ACCEPT = CAMD_STEREO_ACCEPT, SS_LAMBDA = CAMD_STEREO_LAMBDA, SS_COST = CAMD_STEREO_COST, SS_STATUS = CAMD_STEREO_STATUS,
    SS_CONVERGED = CAMD_STEREO_CONVERGED, SS_RIG = CAMD_STEREO_RIG, SS_STEP = CAMD_STEREO_STEP,
    SS_CAND = CAMD_STEREO_CANDIDATE, SS_SOLVED = CAMD_STEREO_SOLVED, SS_PIVOT = CAMD_STEREO_PIVOT
};

struct StereoArgs {
    camd_pnp_points p1, p2;  // the same object rows and frames; the image rows of camera 1 and of camera 2
    Pinhole cam1, cam2;
    Lens k1, k2;
    const int* used;  // the frames of the joint problem, rising
    int used_n;
    double* state;
    double* poses;    // used_n x 12: R_i, t_i of the current estimate (the board in camera 1)
    double* cand;     // used_n x 16: R_i, t_i of the candidate, its cost, |step|^2, |parameters|^2
    double* ws;       // used_n x 91
    double* partial;  // ceil(used_n / 64) x 36
    double* error;    // used_n: sqrt(c_i / 2 n_i)
};

// a frame's pose in camera 2: Rc = R Ri, tc = R ti + t; rt = R ti
__device__ __forceinline__ void compose(const double* R, const double* t, const double* Ri, const double* ti, double* Rc, double* tc,
                                        double* rt)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Rc[3 * i + j] = R[3 * i] * Ri[j] + R[3 * i + 1] * Ri[3 + j] + R[3 * i + 2] * Ri[6 + j];
        rt[i] = R[3 * i] * ti[0] + R[3 * i + 1] * ti[1] + R[3 * i + 2] * ti[2];
        tc[i] = rt[i] + t[i];
    }
}

// one frame at one estimate: its pose in both cameras
struct RigPose {
    double Ri[9], ti[3], R[9], Rc[9], tc[3], rt[3];
};

// the cost of one point in both cameras, grouped as every sum of it here is
__device__ __forceinline__ double rig_cost(const double* r1, const double* r2)
{
    return (r1[0] * r1[0] + r1[1] * r1[1]) + (r2[0] * r2[0] + r2[1] * r2[1]);
}

// one point in both cameras.  Camera 1 sees the frame alone: its residual r0 and Jacobian J0 with respect to the frame.
// Camera 2 sees the rig too: its residual r, its Jacobian with respect to the frame (Jp) and to the rig (Jk).  Returned:
// the point's cost
using RigTerms = ArrowTerms<6, true>;
__device__ __forceinline__ double rig_terms(const StereoArgs& a, const Frame& fr, int i, const RigPose& q, RigTerms& o)
{
    double J2[2][6];
    pose_terms(a.p1, fr, i, a.cam1, a.k1, q.Ri, q.ti, o.r0, o.J0);
    pose_terms(a.p2, fr, i, a.cam2, a.k2, q.Rc, q.tc, o.r, J2);
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const double* g = J2[e] + 3;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            o.Jp[e][j] = J2[e][0] * q.R[j] + J2[e][1] * q.R[3 + j] + J2[e][2] * q.R[6 + j];
            o.Jp[e][3 + j] = g[0] * q.R[j] + g[1] * q.R[3 + j] + g[2] * q.R[6 + j];
            o.Jk[e][3 + j] = g[j];
        }
        o.Jk[e][0] = J2[e][0] + (q.rt[1] * g[2] - q.rt[2] * g[1]);
        o.Jk[e][1] = J2[e][1] + (q.rt[2] * g[0] - q.rt[0] * g[2]);
        o.Jk[e][2] = J2[e][2] + (q.rt[0] * g[1] - q.rt[1] * g[0]);
    }
    return rig_cost(o.r0, o.r);
}

// ---- the sums over a frame's points -------------------------------------------------------------------------------
// Where the last step was taken ([ACCEPT] != 0) the frame's candidate becomes its pose first; k_stereo_update has
// already moved the rig.
__global__ __launch_bounds__(256) void k_stereo_linearise(StereoArgs a)
{
    const int lane = threadIdx.x & 63, u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= a.used_n) return;  // (the whole wave; there is no barrier to miss)
    const Frame fr = used_frame(a.p1, a.used, u);  // (camera 1's image rows; camera 2's lie at the same places)
    RigPose q;
    double t[3];
    double* pose = a.poses + (size_t)u * 12;
    if (uniform(a.state[SS_ACCEPT] != 0.)) {
        load_pose(a.cand + (size_t)u * STEREO_CAND, q.Ri, q.ti);
        if (lane == 0) store_pose(pose, q.Ri, q.ti);
    } else {
        load_pose(pose, q.Ri, q.ti);
    }
    load_pose(a.state + SS_RIG, q.R, t);
    compose(q.R, t, q.Ri, q.ti, q.Rc, q.tc, q.rt);
    arrow_linearise<6, true>([&](int i, RigTerms& o) { return rig_terms(a, fr, i, q, o); }, fr.n, lane, a.ws + (size_t)u * STEREO_WS);
}

// the candidate of one frame: its step by back-substitution from the rig's step, its pose, and the cost there in both
// cameras under the candidate rig
__global__ __launch_bounds__(256) void k_stereo_evaluate(StereoArgs a)
{
    const int lane = threadIdx.x & 63, u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= a.used_n) return;
    if (!uniform(a.state[SS_SOLVED] != 0.)) return;  // no step: k_stereo_update rejects
    const Frame fr = used_frame(a.p1, a.used, u);
    RigPose q;
    double d[6], ti[3], t2[3];
    arrow_frame_step<6>(a.ws + (size_t)u * STEREO_WS, a.state[SS_LAMBDA], a.state + SS_STEP, a.poses + (size_t)u * 12, d, ti, q.Ri, q.ti);
    load_pose(a.state + SS_CAND, q.R, t2);
    compose(q.R, t2, q.Ri, q.ti, q.Rc, q.tc, q.rt);
    double c = 0.;
    for (int i = lane; i < fr.n; i += 64) {
        double r1[2], r2[2], J[2][6];
        pose_terms(a.p1, fr, i, a.cam1, a.k1, q.Ri, q.ti, r1, J);
        pose_terms(a.p2, fr, i, a.cam2, a.k2, q.Rc, q.tc, r2, J);
        c += rig_cost(r1, r2);
    }
    c = wave_sum(c);
    if (lane == 0) {
        double* o = a.cand + (size_t)u * STEREO_CAND;
        arrow_candidate_store(o, q.Ri, q.ti, c, d, ti);
        o[15] = 0.;
    }
}

// ---- the sums over frames: two levels -----------------------------------------------------------------------------
// Level one: a lane per used frame.  The frame's contribution to the reduced system for the current lambda (FINAL = false)
// or undamped, with the frame's error (FINAL = true); the workgroup's 64 contributions summed into partial[blockIdx.x].
template <bool FINAL>
__global__ __launch_bounds__(64) void k_stereo_reduce(StereoArgs a)
{
    const int lane = threadIdx.x;
    const long long u = (long long)blockIdx.x * 64 + lane;
    const double lambda = FINAL ? 0. : a.state[SS_LAMBDA];
    double S[21] = {}, g[6] = {}, dC[6] = {}, cost = 0.;
    int bad = 0;
    if (u < a.used_n) {
        const double* w = a.ws + (size_t)u * STEREO_WS;
        bad = arrow_frame_schur<6>(w, lambda, S, g, dC);
        cost = w[WS::COST];
        if (FINAL) {
            const Frame fr = used_frame(a.p1, a.used, (int)u);
            a.error[u] = sqrt(__ddiv_rn(cost, 2. * (double)(fr.n > 0 ? fr.n : 1)));
        }
    }
    wave_sum_all<21>(S);
    wave_sum_all<6>(g);
    wave_sum_all<6>(dC);
    cost = wave_sum(cost);
    bad = wave_or(bad);
    if (lane == 0) {
        double* o = a.partial + (size_t)blockIdx.x * STEREO_PARTIAL;
#pragma unroll
        for (int p = 0; p < 21; p++) o[SP_S + p] = S[p];
#pragma unroll
        for (int p = 0; p < 6; p++) o[SP_G + p] = g[p], o[SP_DC + p] = dC[p];
        o[SP_COST] = cost;
        o[SP_BAD] = bad ? 1. : 0.;
        o[SP_BAD + 1] = 0.;
    }
}

// Level two, one wavefront: the partials in rising order, then the rig's step and its candidate (FINAL = false); or, once
// the iteration has ended, the undamped reduced matrix scaled to a unit diagonal, its smallest pivot, the rig's status
// and the cost (FINAL = true).
template <bool FINAL>
__global__ __launch_bounds__(64) void k_stereo_solve(StereoArgs a, int partials)
{
    const int lane = threadIdx.x;
    double S[21] = {}, g[6] = {}, dC[6] = {}, cost = 0., bad = 0.;
    for (int b = lane; b < partials; b += 64) {
        const double* o = a.partial + (size_t)b * STEREO_PARTIAL;
#pragma unroll
        for (int p = 0; p < 21; p++) S[p] += o[SP_S + p];
#pragma unroll
        for (int p = 0; p < 6; p++) g[p] += o[SP_G + p], dC[p] += o[SP_DC + p];
        cost += o[SP_COST];
        bad += o[SP_BAD];
    }
    wave_sum_all<21>(S);
    wave_sum_all<6>(g);
    wave_sum_all<6>(dC);
    cost = wave_sum(cost);
    bool ok = wave_sum(bad) == 0.;
    double pivot;
    if (FINAL) {
        ok = unit_diagonal_pivot<6>(S, pivot) && ok;
        if (lane == 0) {
            const bool good = ok && pivot >= SINGULAR_PIVOT && isfinite(cost) && a.state[SS_CONVERGED] != 0.;
            a.state[SS_STATUS] = good ? 0. : 3.;
            a.state[SS_PIVOT] = pivot;
            a.state[SS_COST] = cost;
        }
    } else {
        const double lambda = a.state[SS_LAMBDA];
#pragma unroll
        for (int p = 0; p < 6; p++) S[p * (p + 1) / 2 + p] += lambda * dC[p], g[p] = -g[p];
        ok = cholesky<6>(S, pivot) && ok;
        if (ok) cholesky_solve<6>(S, g);
#pragma unroll
        for (int p = 0; p < 6; p++) ok = ok && isfinite(g[p]);
        double R[9], t[3], R2[9];
        load_pose(a.state + SS_RIG, R, t);
#pragma unroll
        for (int p = 0; p < 6; p++) g[p] = ok ? g[p] : 0.;
        rotate_left(g, R, R2);
        const double t2[3] = {t[0] + g[3], t[1] + g[4], t[2] + g[5]};
        if (lane == 0) {
#pragma unroll
            for (int p = 0; p < 6; p++) a.state[SS_STEP + p] = g[p];
            store_pose(a.state + SS_CAND, R2, t2);
            a.state[SS_SOLVED] = ok ? 1. : 0.;
        }
    }
}

// accept or reject the candidate, move lambda, decide whether to stop (lm_update); after a step that is taken the rig
// moves here, the frames' poses follow in k_stereo_linearise
__global__ __launch_bounds__(64) void k_stereo_update(StereoArgs a, int max_evaluations)
{
    const int lane = threadIdx.x;
    const bool solved = a.state[SS_SOLVED] != 0.;
    double c = 0., c2 = 0., step = 0., norm = 0.;
    for (int u = lane; u < a.used_n; u += 64) {
        c += a.ws[(size_t)u * STEREO_WS + WS::COST];
        if (solved) {
            const double* o = a.cand + (size_t)u * STEREO_CAND;
            c2 += o[12], step += o[13], norm += o[14];
        }
    }
    c = wave_sum(c), c2 = wave_sum(c2), step = wave_sum(step), norm = wave_sum(norm);
    double rig[12], rig2[12];
#pragma unroll
    for (int p = 0; p < 12; p++) rig[p] = a.state[SS_RIG + p], rig2[p] = a.state[SS_CAND + p];
#pragma unroll
    for (int p = 0; p < 6; p++) step += a.state[SS_STEP + p] * a.state[SS_STEP + p];
    norm += pose_norm2(rig + 9);
    if (lm_update(a.state, lane, solved, c, c2, step, norm, max_evaluations) && lane == 0) {
#pragma unroll
        for (int p = 0; p < 12; p++) a.state[SS_RIG + p] = rig2[p];
    }
}

// the arguments every entry point shares; `needs`: which of poses, candidate, partials, frame_error the caller uses
enum { NEED_POSES = 1, NEED_CAND = 2, NEED_PARTIAL = 4, NEED_ERROR = 8 };
static int stereo_args(const char* who, const camd_stereo_rig* rig, int needs, StereoArgs& a)
{
    if (!rig) {
        set_error("%s: bad arguments (rig: a camd_stereo_rig)", who);
        return CAMD_ERR_BAD_ARG;
    }
    const camd_pnp_points *p = &rig->points1, *q = &rig->points2;
    const bool same = points_ok(p) && points_ok(q) && p->frames == q->frames && p->object == q->object && p->start == q->start &&
                      p->object_rows == q->object_rows && p->image_rows == q->image_rows && p->object_type == q->object_type &&
                      p->object_stride == q->object_stride && p->object_shared == q->object_shared;
    const int n = rig->used_n;
    const bool live = n > 0;
    if (!same || n < 0 || !rig->K1 || !rig->K2 ||
        (live && (!rig->used || (uintptr_t)rig->used % 4 != 0 || !doubles_ok(rig->state) || !doubles_ok(rig->workspace) ||
                  p->frames == 0 || ((needs & NEED_POSES) && !doubles_ok(rig->poses)) ||
                  ((needs & NEED_CAND) && !doubles_ok(rig->candidate)) || ((needs & NEED_PARTIAL) && !doubles_ok(rig->partials)) ||
                  ((needs & NEED_ERROR) && !doubles_ok(rig->frame_error))))) {
        set_error("%s: bad arguments (points1, points2: as in camd_pnp_init, the same object rows, start and frames, their own "
                  "image rows of equal count; K1, K2: 9 host doubles; used: used_n >= 0 device int32, got %d; state: CAMD_STEREO_STATE_DOUBLES, poses: "
                  "used_n x 12, candidate: used_n x 16, workspace: used_n x 91, partials: ceil(used_n / 64) x 36, frame_error: "
                  "used_n device doubles)", who, n);
        return CAMD_ERR_BAD_ARG;
    }
    const int nd[2] = {rig->ndist1, rig->ndist2};
    const double* dist[2] = {rig->dist1, rig->dist2};
    for (int c = 0; c < 2; c++)
        if ((nd[c] != 0 && nd[c] != 4 && nd[c] != 5 && nd[c] != 8 && nd[c] != 12 && nd[c] != 14) || (nd[c] > 0 && !dist[c])) {
            set_error("%s: bad arguments (ndist%d is 0, 4, 5, 8, 12 or 14 host doubles, got %d)", who, c + 1, nd[c]);
            return CAMD_ERR_BAD_ARG;
        }
    a.p1 = *p, a.p2 = *q, a.used = rig->used, a.used_n = n, a.state = rig->state, a.poses = rig->poses, a.cand = rig->candidate;
    a.ws = rig->workspace, a.partial = rig->partials, a.error = rig->frame_error;
    int rc = unpack_camera(who, rig->K1, rig->dist1, rig->ndist1, &a.cam1, &a.k1);
    if (rc != CAMD_OK) return rc;
    return unpack_camera(who, rig->K2, rig->dist2, rig->ndist2, &a.cam2, &a.k2);
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_stereo_linearise(const camd_stereo_rig* rig, void* queue)
{
    StereoArgs a = {};
    int rc = stereo_args("camd_stereo_linearise", rig, NEED_POSES | NEED_CAND, a);
    if (rc != CAMD_OK) return rc;
    if (a.used_n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_stereo_linearise, dim3(div_up(a.used_n, 4)), dim3(256), 0, (hipStream_t)queue, a);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_stereo_step(const camd_stereo_rig* rig, void* queue)
{
    StereoArgs a = {};
    int rc = stereo_args("camd_stereo_step", rig, NEED_POSES | NEED_CAND | NEED_PARTIAL, a);
    if (rc != CAMD_OK) return rc;
    if (a.used_n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    const int partials = div_up(a.used_n, 64);
    hipLaunchKernelGGL(k_stereo_reduce<false>, dim3(partials), dim3(64), 0, (hipStream_t)queue, a);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stereo_solve<false>, dim3(1), dim3(64), 0, (hipStream_t)queue, a, partials);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stereo_evaluate, dim3(div_up(a.used_n, 4)), dim3(256), 0, (hipStream_t)queue, a);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stereo_update, dim3(1), dim3(64), 0, (hipStream_t)queue, a, STEREO_MAX_EVALUATIONS);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_stereo_finish(const camd_stereo_rig* rig, void* queue)
{
    StereoArgs a = {};
    int rc = stereo_args("camd_stereo_finish", rig, NEED_PARTIAL | NEED_ERROR, a);
    if (rc != CAMD_OK) return rc;
    if (a.used_n == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    const int partials = div_up(a.used_n, 64);
    hipLaunchKernelGGL(k_stereo_reduce<true>, dim3(partials), dim3(64), 0, (hipStream_t)queue, a);
    CAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stereo_solve<true>, dim3(1), dim3(64), 0, (hipStream_t)queue, a, partials);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
