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
// and every frame's step follows by back-substitution.  Damping, stopping and the acceptance of a step are
// pnp_common.hpp's (LM_*, lm_better).
//
// Camera 2's terms come from pose_terms at the composed pose (R R_i, R t_i + t), whose 2 x 6 Jacobian J2 = [Jw | Jd] gives
//   with respect to the frame:  [Jw R | Jd R]                    (exp([R w_i]x) R R_i = R exp([w_i]x) R_i)
//   with respect to the rig:    [Jw + (R t_i) x Jd | Jd]         (the rotation also turns R t_i)
// (tests/stereo_calibrate_ref.py checks both against finite differences).
//
// Kernels.  k_stereo_linearise and k_stereo_evaluate sum over a frame's points: one wavefront per frame, four frames per
// workgroup, no workgroup barrier, the butterfly of pnp_common.hpp; 91 accumulators do not fit beside two Jacobians, so
// the linearisation makes three passes over the points: A gp c, then B, then C gr.  The sums over FRAMES have two levels,
// unlike calibrate.hip's: k_stereo_reduce gives every used frame a lane of its own, which factors the frame's damped
// block and forms its contribution to the reduced system (21 + 6 doubles, diag C_i, the cost); the 64 frames of a
// workgroup are summed by the butterfly into one partial.  k_stereo_solve, one wavefront, then adds the partials -- lane l
// takes partials l, l + 64, ... in rising order, then the butterfly -- and solves the 6 x 6.  It sees used_n / 64 partials
// of 34 doubles and no factorization of a frame.  No atomics: the same input gives the same bits on every run.
// Lambda, the costs, the accept decision, both rigs and the stop flag live in `state` on the device; the host reads two
// numbers per evaluation (camd_calib_read: the first two places of the state are calibrate.hip's).
//
// cv2's own iteration and its 1e-5 stop are UNPINNED.
#include "pnp_common.hpp"

namespace camd {

constexpr int STEREO_MAX_EVALUATIONS = 100;  // every case of tests/stereo_calibrate_cases.py ends below half of it
constexpr int STEREO_WS = CAMD_STEREO_WORKSPACE_DOUBLES, STEREO_CAND = CAMD_STEREO_CANDIDATE_DOUBLES;
constexpr int STEREO_PARTIAL = CAMD_STEREO_PARTIAL_DOUBLES;
// the workspace of one frame
enum { SW_A = 0, SW_B = 21, SW_C = 57, SW_GP = 78, SW_GR = 84, SW_COST = 90 };
// a partial of the reduced system: S 21, g 6, diag C 6, the cost, then the count of frames whose block did not factor
enum { SP_S = 0, SP_G = 21, SP_DC = 27, SP_COST = 33, SP_BAD = 34 };
// the state (doubles; include/calibrating_amd.h names the places the host reads and writes)
enum {
    SS_DONE = CAMD_STEREO_DONE, SS_ACCEPT = CAMD_STEREO_ACCEPT, SS_LAMBDA = CAMD_STEREO_LAMBDA, SS_COST = CAMD_STEREO_COST,
    SS_EVALS = CAMD_STEREO_EVALUATIONS, SS_ITERS = CAMD_STEREO_ITERATIONS, SS_STATUS = CAMD_STEREO_STATUS,
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

// the rows of used frame u (camera 1's image rows; camera 2's lie at the same places); a frame index or a range outside
// the arrays reads nothing
__device__ __forceinline__ Frame used_frame(const StereoArgs& a, int u)
{
    const int f = a.used[u];
    Frame none = {0, 0, 0, PNP_NONFINITE};
    if (f < 0 || f >= a.p1.frames) return none;
    Frame fr = frame_rows(a.p1, f, 1);
    if (fr.status != PNP_OK) fr.n = 0;
    return fr;
}

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

// one point in both cameras: the residuals, camera 1's Jacobian with respect to the frame (J1), camera 2's with respect to
// the frame (Jf) and to the rig (Jr)
struct RigTerms {
    double r1[2], r2[2], J1[2][6], Jf[2][6], Jr[2][6];
};
__device__ __forceinline__ void rig_terms(const StereoArgs& a, const Frame& fr, int i, const RigPose& q, RigTerms& o)
{
    double J2[2][6];
    pose_terms(a.p1, fr, i, a.cam1, a.k1, q.Ri, q.ti, o.r1, o.J1);
    pose_terms(a.p2, fr, i, a.cam2, a.k2, q.Rc, q.tc, o.r2, J2);
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const double* g = J2[e] + 3;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            o.Jf[e][j] = J2[e][0] * q.R[j] + J2[e][1] * q.R[3 + j] + J2[e][2] * q.R[6 + j];
            o.Jf[e][3 + j] = g[0] * q.R[j] + g[1] * q.R[3 + j] + g[2] * q.R[6 + j];
            o.Jr[e][3 + j] = g[j];
        }
        o.Jr[e][0] = J2[e][0] + (q.rt[1] * g[2] - q.rt[2] * g[1]);
        o.Jr[e][1] = J2[e][1] + (q.rt[2] * g[0] - q.rt[0] * g[2]);
        o.Jr[e][2] = J2[e][2] + (q.rt[0] * g[1] - q.rt[1] * g[0]);
    }
}

// ---- the sums over a frame's points -------------------------------------------------------------------------------
// Where the last step was taken ([ACCEPT] != 0) the frame's candidate becomes its pose first; k_stereo_update has
// already moved the rig.
__global__ __launch_bounds__(256) void k_stereo_linearise(StereoArgs a)
{
    const int lane = threadIdx.x & 63, u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= a.used_n) return;  // (the whole wave; there is no barrier to miss)
    const Frame fr = used_frame(a, u);
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
    double* w = a.ws + (size_t)u * STEREO_WS;
    {  // pass 1: A, gp, c
        double A[21] = {}, g[6] = {}, c = 0.;
        for (int i = lane; i < fr.n; i += 64) {
            RigTerms o;
            rig_terms(a, fr, i, q, o);
            add_outer<6>(A, o.J1[0], o.J1[1]);
            add_outer<6>(A, o.Jf[0], o.Jf[1]);
            add_gradient<6>(g, o.J1[0], o.J1[1], o.r1);
            add_gradient<6>(g, o.Jf[0], o.Jf[1], o.r2);
            c += (o.r1[0] * o.r1[0] + o.r1[1] * o.r1[1]) + (o.r2[0] * o.r2[0] + o.r2[1] * o.r2[1]);
        }
        wave_sum_all<21>(A);
        wave_sum_all<6>(g);
        c = wave_sum(c);
        if (lane == 0) {
#pragma unroll
            for (int p = 0; p < 21; p++) w[SW_A + p] = A[p];
#pragma unroll
            for (int p = 0; p < 6; p++) w[SW_GP + p] = g[p];
            w[SW_COST] = c;
        }
    }
    {  // pass 2: B
        double B[36] = {};
        for (int i = lane; i < fr.n; i += 64) {
            RigTerms o;
            rig_terms(a, fr, i, q, o);
#pragma unroll
            for (int p = 0; p < 6; p++)
#pragma unroll
                for (int r = 0; r < 6; r++) B[p * 6 + r] += o.Jf[0][p] * o.Jr[0][r] + o.Jf[1][p] * o.Jr[1][r];
        }
        wave_sum_all<36>(B);
        if (lane == 0) {
#pragma unroll
            for (int p = 0; p < 36; p++) w[SW_B + p] = B[p];
        }
    }
    {  // pass 3: C, gr
        double C[21] = {}, g[6] = {};
        for (int i = lane; i < fr.n; i += 64) {
            RigTerms o;
            rig_terms(a, fr, i, q, o);
            add_outer<6>(C, o.Jr[0], o.Jr[1]);
            add_gradient<6>(g, o.Jr[0], o.Jr[1], o.r2);
        }
        wave_sum_all<21>(C);
        wave_sum_all<6>(g);
        if (lane == 0) {
#pragma unroll
            for (int p = 0; p < 21; p++) w[SW_C + p] = C[p];
#pragma unroll
            for (int p = 0; p < 6; p++) w[SW_GR + p] = g[p];
        }
    }
}

// the candidate of one frame: its step by back-substitution from the rig's step, its pose, and the cost there in both
// cameras under the candidate rig
__global__ __launch_bounds__(256) void k_stereo_evaluate(StereoArgs a)
{
    const int lane = threadIdx.x & 63, u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= a.used_n) return;
    if (!uniform(a.state[SS_SOLVED] != 0.)) return;  // no step: k_stereo_update rejects
    const Frame fr = used_frame(a, u);
    const double* w = a.ws + (size_t)u * STEREO_WS;
    double L[21], d[6], Ri[9], ti[3], pivot;
    damped<6>(w + SW_A, a.state[SS_LAMBDA], L);
    cholesky<6>(L, pivot);  // (k_stereo_reduce factored it: it did not fail)
#pragma unroll
    for (int p = 0; p < 6; p++) {
        double s = w[SW_GP + p];
#pragma unroll
        for (int r = 0; r < 6; r++) s += w[SW_B + p * 6 + r] * a.state[SS_STEP + r];
        d[p] = -s;
    }
    cholesky_solve<6>(L, d);
    load_pose(a.poses + (size_t)u * 12, Ri, ti);
    RigPose q;
    double t2[3];
    rotate_left(d, Ri, q.Ri);
    q.ti[0] = ti[0] + d[3], q.ti[1] = ti[1] + d[4], q.ti[2] = ti[2] + d[5];
    load_pose(a.state + SS_CAND, q.R, t2);
    compose(q.R, t2, q.Ri, q.ti, q.Rc, q.tc, q.rt);
    double c = 0.;
    for (int i = lane; i < fr.n; i += 64) {
        double r1[2], r2[2], J[2][6];
        pose_terms(a.p1, fr, i, a.cam1, a.k1, q.Ri, q.ti, r1, J);
        pose_terms(a.p2, fr, i, a.cam2, a.k2, q.Rc, q.tc, r2, J);
        c += (r1[0] * r1[0] + r1[1] * r1[1]) + (r2[0] * r2[0] + r2[1] * r2[1]);
    }
    c = wave_sum(c);
    if (lane == 0) {
        double* o = a.cand + (size_t)u * STEREO_CAND;
        store_pose(o, q.Ri, q.ti);
        o[12] = c;
        o[13] = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5];
        o[14] = pose_norm2(ti);
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
        double L[21], y[6], frame_pivot;
        damped<6>(w + SW_A, lambda, L);
        bad = !cholesky<6>(L, frame_pivot);
#pragma unroll
        for (int p = 0; p < 6; p++) y[p] = w[SW_GP + p];
        cholesky_solve<6>(L, y);
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double s = w[SW_GR + r];
#pragma unroll
            for (int p = 0; p < 6; p++) s -= w[SW_B + p * 6 + r] * y[p];
            g[r] = s;
        }
#pragma unroll
        for (int j = 0; j < 6; j++) {
#pragma unroll
            for (int p = 0; p < 6; p++) y[p] = w[SW_B + p * 6 + j];
            cholesky_solve<6>(L, y);
#pragma unroll
            for (int r = 0; r <= j; r++) {
                double s = w[SW_C + j * (j + 1) / 2 + r];
#pragma unroll
                for (int p = 0; p < 6; p++) s -= w[SW_B + p * 6 + r] * y[p];
                S[j * (j + 1) / 2 + r] = s;
            }
            dC[j] = w[SW_C + j * (j + 1) / 2 + j];
        }
        cost = w[SW_COST];
        if (FINAL) {
            const Frame fr = used_frame(a, (int)u);
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

// accept or reject the candidate, move lambda, decide whether to stop (the LM rule on the joint step and parameters);
// the frames' poses follow in k_stereo_linearise
__global__ __launch_bounds__(64) void k_stereo_update(StereoArgs a, int max_evaluations)
{
    const int lane = threadIdx.x;
    const bool solved = a.state[SS_SOLVED] != 0.;
    double c = 0., c2 = 0., step = 0., norm = 0.;
    for (int u = lane; u < a.used_n; u += 64) {
        c += a.ws[(size_t)u * STEREO_WS + SW_COST];
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
    const bool small = solved && lm_small(step, norm);
    const bool better = uniform(solved && lm_better(c2, c));
    if (lane == 0) {
        const double lambda = lm_next(a.state[SS_LAMBDA], better), evals = a.state[SS_EVALS] + 1.;
        const bool stopped = lm_stopped(small, lambda);
        if (better) {
#pragma unroll
            for (int p = 0; p < 12; p++) a.state[SS_RIG + p] = rig2[p];
            a.state[SS_ITERS] += 1.;
        }
        a.state[SS_LAMBDA] = lambda;
        a.state[SS_EVALS] = evals;
        a.state[SS_ACCEPT] = better ? 1. : 0.;
        a.state[SS_CONVERGED] = stopped ? 1. : 0.;
        a.state[SS_DONE] = (stopped || evals >= (double)max_evaluations) ? 1. : 0.;
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
