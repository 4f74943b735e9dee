// joint_common.hpp -- what the joint Levenberg-Marquardt solvers share on top of pnp_common.hpp's primitives.
//
// calibrate.hip and stereo_calibrate.hip solve the same arrow: six unknowns per frame (pnp.hip's local perturbation
// R <- exp([w]x) R, t <- t + d) and one block of NK shared by all frames (the intrinsics, NK = 9; the rig, NK = 6).  Here:
//   used_frame          the checked rows of a frame of the joint problem
//   ArrowBlock<NK>      the places of a frame's sums A, B, C, gp, gk, c in its workspace
//   ArrowTerms<NK, ..>  what one point gives those sums; the solver's functor fills it (point_terms, rig_terms)
//   arrow_linearise     the three passes over a frame's points, one wavefront, with their butterflies and stores
//   arrow_frame_schur   a frame's contribution C - B^T (A + l diag A)^-1 B, gk - B^T (..)^-1 gp (k_stereo_reduce; see there)
//   arrow_frame_step    a frame's own step by back-substitution from the shared block's, and its candidate pose
//   arrow_candidate_store   what a frame's candidate leaves for the update: its pose, cost, |step|^2, |pose|^2
// and for all three (bundle.hip too, whose arrow runs the other way: 3 x 3 point blocks, the views shared):
//   LM_DONE ... LM_CONVERGED, lm_update   the accept decision and the bookkeeping of the state's places 0-7
// Header-only: the library is linked without relocatable device code, every translation unit instantiates its own.
// -ffp-contract=off: the grouping and the order of every sum here are part of the result's bits.
#pragma once

#include "pnp_common.hpp"

namespace camd {

// the rows of used frame u; a frame index or a range outside the arrays reads nothing
__device__ __forceinline__ Frame used_frame(const camd_pnp_points& p, const int* used, int u)
{
    const int f = used[u];
    Frame none = {0, 0, 0, PNP_NONFINITE};
    if (f < 0 || f >= p.frames) return none;
    Frame fr = frame_rows(p, f, 1);
    if (fr.status != PNP_OK) fr.n = 0;
    return fr;
}

// the workspace of one frame: A (6 x 6, packed), B (6 x NK), C (NK x NK, packed), gp, gk, the cost
template <int NK>
struct ArrowBlock {
    static constexpr int A = 0, B = 21, C = B + 6 * NK, GP = C + NK * (NK + 1) / 2, GK = GP + 6, COST = GK + NK, SIZE = COST + 1;
};
static_assert(ArrowBlock<9>::SIZE == CAMD_CALIB_WORKSPACE_DOUBLES && ArrowBlock<6>::SIZE == CAMD_STEREO_WORKSPACE_DOUBLES, "");
static_assert(ArrowBlock<9>::B == 21 && ArrowBlock<9>::C == 75 && ArrowBlock<9>::GP == 120 && ArrowBlock<9>::GK == 126 &&
              ArrowBlock<9>::COST == 135, "calibrate's workspace");
static_assert(ArrowBlock<6>::B == 21 && ArrowBlock<6>::C == 57 && ArrowBlock<6>::GP == 78 && ArrowBlock<6>::GK == 84 &&
              ArrowBlock<6>::COST == 90, "stereo_calibrate's workspace");

// One point: the observation that sees the shared block -- its residual r, its 2 x 6 Jacobian Jp in the frame and 2 x NK
// Jacobian Jk in the block -- and with ALSO a second one that sees the frame alone (r0, J0), summed before it.
template <int NK, bool ALSO>
struct ArrowTerms {
    double r[2], Jp[2][6], Jk[2][NK];
};
template <int NK>
struct ArrowTerms<NK, true> : ArrowTerms<NK, false> {
    double r0[2], J0[2][6];
};

// The sums over a frame's n points into its workspace w, one wavefront.  terms(i, o) fills point i's ArrowTerms and returns
// its cost, grouped as the solver sums it.  All the accumulators do not fit beside the Jacobians, so the points are passed
// three times: A gp c, then B, then C gk, each set of accumulators in a scope of its own.
template <int NK, bool ALSO, class F>
__device__ __forceinline__ void arrow_linearise(F terms, int n, int lane, double* w)
{
    using W = ArrowBlock<NK>;
    {  // pass 1: A, gp, c
        double A[21] = {}, g[6] = {}, c = 0.;
        for (int i = lane; i < n; i += 64) {
            ArrowTerms<NK, ALSO> o;
            const double ci = terms(i, o);
            if constexpr (ALSO) add_outer<6>(A, o.J0[0], o.J0[1]);
            add_outer<6>(A, o.Jp[0], o.Jp[1]);
            if constexpr (ALSO) add_gradient<6>(g, o.J0[0], o.J0[1], o.r0);
            add_gradient<6>(g, o.Jp[0], o.Jp[1], o.r);
            c += ci;
        }
        wave_sum_all<21>(A);
        wave_sum_all<6>(g);
        c = wave_sum(c);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 21; q++) w[W::A + q] = A[q];
#pragma unroll
            for (int q = 0; q < 6; q++) w[W::GP + q] = g[q];
            w[W::COST] = c;
        }
    }
    {  // pass 2: B
        double B[6 * NK] = {};
        for (int i = lane; i < n; i += 64) {
            ArrowTerms<NK, ALSO> o;
            terms(i, o);
#pragma unroll
            for (int p = 0; p < 6; p++)
#pragma unroll
                for (int q = 0; q < NK; q++) B[p * NK + q] += o.Jp[0][p] * o.Jk[0][q] + o.Jp[1][p] * o.Jk[1][q];
        }
        wave_sum_all<6 * NK>(B);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 6 * NK; q++) w[W::B + q] = B[q];
        }
    }
    {  // pass 3: C, gk
        double C[NK * (NK + 1) / 2] = {}, g[NK] = {};
        for (int i = lane; i < n; i += 64) {
            ArrowTerms<NK, ALSO> o;
            terms(i, o);
            add_outer<NK>(C, o.Jk[0], o.Jk[1]);
            add_gradient<NK>(g, o.Jk[0], o.Jk[1], o.r);
        }
        wave_sum_all<NK * (NK + 1) / 2>(C);
        wave_sum_all<NK>(g);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < NK * (NK + 1) / 2; q++) w[W::C + q] = C[q];
#pragma unroll
            for (int q = 0; q < NK; q++) w[W::GK + q] = g[q];
        }
    }
}

// One frame's contribution to the reduced system at lambda, assigned to S (NK x NK, packed), g and dC = diag C; returned:
// whether the frame's damped block did not factor.  Every B[p][.] y[p] is subtracted in rising p.  k_stereo_reduce calls
// it, a lane per frame.  k_calib_solve, a lane's running sum over its frames, writes the same nest out and adds each
// finished number where it is made: through a helper the compiler schedules that loop otherwise, measured 0.8 % slower.
template <int NK>
__device__ __forceinline__ bool arrow_frame_schur(const double* w, double lambda, double* S, double* g, double* dC)
{
    using W = ArrowBlock<NK>;
    double L[21], y[6], pivot;
    damped<6>(w + W::A, lambda, L);
    const bool bad = !cholesky<6>(L, pivot);
#pragma unroll
    for (int p = 0; p < 6; p++) y[p] = w[W::GP + p];
    cholesky_solve<6>(L, y);
#pragma unroll
    for (int q = 0; q < NK; q++) {
        double s = w[W::GK + q];
#pragma unroll
        for (int p = 0; p < 6; p++) s -= w[W::B + p * NK + q] * y[p];
        g[q] = s;
    }
#pragma unroll
    for (int j = 0; j < NK; j++) {
#pragma unroll
        for (int p = 0; p < 6; p++) y[p] = w[W::B + p * NK + j];
        cholesky_solve<6>(L, y);
#pragma unroll
        for (int q = 0; q <= j; q++) {
            double s = w[W::C + j * (j + 1) / 2 + q];
#pragma unroll
            for (int p = 0; p < 6; p++) s -= w[W::B + p * NK + q] * y[p];
            S[j * (j + 1) / 2 + q] = s;
        }
        dC[j] = w[W::C + j * (j + 1) / 2 + j];
    }
    return bad;
}

// A frame's own step d = -(A + lambda diag A)^-1 (gp + B shared_step) and its candidate R2 = exp([d_w]x) R, t2 = t + d_t
// from its pose (whose t comes back too).  The frame's block was factored when the shared step was solved: it did not fail.
template <int NK>
__device__ __forceinline__ void arrow_frame_step(const double* w, double lambda, const double* shared_step, const double* pose,
                                                 double* d, double* t, double* R2, double* t2)
{
    using W = ArrowBlock<NK>;
    double L[21], R[9], pivot;
    damped<6>(w + W::A, lambda, L);
    cholesky<6>(L, pivot);
#pragma unroll
    for (int p = 0; p < 6; p++) {
        double s = w[W::GP + p];
#pragma unroll
        for (int q = 0; q < NK; q++) s += w[W::B + p * NK + q] * shared_step[q];
        d[p] = -s;
    }
    cholesky_solve<6>(L, d);
    load_pose(pose, R, t);
    t2[0] = t[0] + d[3], t2[1] = t[1] + d[4], t2[2] = t[2] + d[5];
    rotate_left(d, R, R2);
}

// a frame's candidate row: R2, t2, its cost c there, |d|^2 of its step and |p|^2 of the pose it left (t)
__device__ __forceinline__ void arrow_candidate_store(double* out, const double* R2, const double* t2, double c, const double* d,
                                                      const double* t)
{
    store_pose(out, R2, t2);
    out[12] = c;
    out[13] = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5];
    out[14] = pose_norm2(t);
}

// ---- the state's places every joint solver numbers alike (the host reads the first two through camd_calib_read) ----
enum {
    LM_DONE = CAMD_CALIB_DONE, LM_ACCEPT = CAMD_CALIB_ACCEPT, LM_LAMBDA = CAMD_CALIB_LAMBDA, LM_EVALS = CAMD_CALIB_EVALUATIONS,
    LM_ITERS = CAMD_CALIB_ITERATIONS, LM_CONVERGED = CAMD_CALIB_CONVERGED  // (COST and STATUS are written by each solver's finish)
};
#define CAMD_SAME_PLACE(NAME) (CAMD_STEREO_##NAME == CAMD_CALIB_##NAME && CAMD_BUNDLE_##NAME == CAMD_CALIB_##NAME)
static_assert(CAMD_SAME_PLACE(DONE) && CAMD_SAME_PLACE(ACCEPT) && CAMD_SAME_PLACE(LAMBDA) && CAMD_SAME_PLACE(COST) &&
              CAMD_SAME_PLACE(EVALUATIONS) && CAMD_SAME_PLACE(ITERATIONS) && CAMD_SAME_PLACE(STATUS) && CAMD_SAME_PLACE(CONVERGED),
              "the joint solvers number the state's places 0-7 alike");
#undef CAMD_SAME_PLACE

// Accept or reject the candidate, move lambda, decide whether to stop: the LM rule on the joint step and parameters.
// c, c2: the cost at the estimate and at the candidate; step, norm: |step|^2 and |parameters|^2 over every unknown; solved:
// there is a step at all.  One wavefront with the same numbers in every lane; lane 0 writes the places.  The answer is
// uniform: what the caller moves after an accepted step may be strided over the lanes.
__device__ __forceinline__ bool lm_update(double* state, int lane, bool solved, double c, double c2, double step, double norm,
                                          int max_evaluations)
{
    const bool small = solved && lm_small(step, norm);
    const bool better = uniform(solved && lm_better(c2, c));
    if (lane == 0) {
        const double lambda = lm_next(state[LM_LAMBDA], better), evals = state[LM_EVALS] + 1.;
        const bool stopped = lm_stopped(small, lambda);
        if (better) state[LM_ITERS] += 1.;
        state[LM_LAMBDA] = lambda;
        state[LM_EVALS] = evals;
        state[LM_ACCEPT] = better ? 1. : 0.;
        state[LM_CONVERGED] = stopped ? 1. : 0.;
        state[LM_DONE] = (stopped || evals >= (double)max_evaluations) ? 1. : 0.;
    }
    return better;
}

}  // namespace camd
