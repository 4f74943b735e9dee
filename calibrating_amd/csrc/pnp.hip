// pnp.hip -- the pose of a target in every frame of a recording from its detected points (batched PnP).
//
// Replaces (file:line in the reference's calibrating/):
//   camera.py:266-273   cv2.solvePnPGeneric(object_points, image_points[:, None], K, D) -> rvecs[0], tvecs[0], RMS
// One wavefront per frame, four frames per 256-thread workgroup and NO workgroup barrier anywhere: the waves of a group
// belong to different frames and run different numbers of iterations.  The lanes of a wave stride over the frame's
// points and keep partial sums; an xor butterfly of fixed order leaves the same bits of every sum in every lane, so all
// that follows (a 6x6 / 9x9 / 12x12 Cholesky, the damping rule, the stopping rule) is computed by every lane, redundantly
// and uniformly, and a frame's result depends on nothing but its own rows: alone or at any place of a batch it gets
// the same bits.  Every loop has a trip count bounded by a constant or by the frame's point count.
//
// cv2's own solver is UNPINNED: this is a float64 Levenberg-Marquardt on raw, distorted
// pixels run to float64 convergence; cv2 stops after 20 iterations at FLT_EPSILON.
#include "pnp_common.hpp"

namespace camd {

// ---- refinement -------------------------------------------------------------------------------------------------
struct Normal {
    double A[21], g[6], c;  // J^T J (lower triangle packed), J^T r, r^T r
};

// pose_terms at every point of the frame; their sums, reduced over the wave
__device__ __forceinline__ void normal_equations(const PnpArgs& a, const Frame& fr, int lane, const double* R, const double* t,
                                                 Normal& S)
{
#pragma unroll
    for (int q = 0; q < 21; q++) S.A[q] = 0.;
#pragma unroll
    for (int q = 0; q < 6; q++) S.g[q] = 0.;
    S.c = 0.;
    for (int i = lane; i < fr.n; i += 64) {
        double r[2], J[2][6];
        pose_terms(a.p, fr, i, a.cam, a.k, R, t, r, J);
        add_outer<6>(S.A, J[0], J[1]);
        add_gradient<6>(S.g, J[0], J[1], r);
        S.c += r[0] * r[0] + r[1] * r[1];
    }
    wave_sum_all<21>(S.A);
    wave_sum_all<6>(S.g);
    S.c = wave_sum(S.c);
}

__device__ __forceinline__ void store_frame(int lane, int f, const double* R, const double* t, double rms, int iterations,
                                            int status, double* pose, double* rms_out, int* iterations_out, int* status_out)
{
    if (lane != 0) return;
    store_pose(pose + (size_t)f * 12, R, t, status == PNP_OK);
    rms_out[f] = status == PNP_OK ? rms : NAN;
    iterations_out[f] = iterations;
    status_out[f] = status;
}

__global__ __launch_bounds__(256) void k_pnp_refine(PnpArgs a, const double* __restrict__ pose0, int pose0_stride,
                                                    double* __restrict__ pose, double* __restrict__ rms_out,
                                                    int* __restrict__ iterations_out, int* __restrict__ status_out)
{
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= a.p.frames) return;  // (the whole wave; there is no barrier to miss)
    double R[9], t[3];
    const Frame fr = frame_rows(a.p, f, a.min_points);
    int status = fr.status;
    if (status == PNP_OK && frame_nonfinite(a.p, fr, lane)) status = PNP_NONFINITE;
    // a start pose that is not finite: none could be made (camd_pnp_init on a degenerate frame)
    if (status == PNP_OK && !uniform(load_pose(pose0 + (size_t)f * pose0_stride, R, t))) status = PNP_SINGULAR;
    if (status != PNP_OK) {
        store_frame(lane, f, R, t, 0., 0, status, pose, rms_out, iterations_out, status_out);
        return;
    }
    Normal S, S2;
    normal_equations(a, fr, lane, R, t, S);
    double lambda = LM_LAMBDA_START;
    int it = 0;
    bool stopped = false;
    while (uniform(it < PNP_MAX_ITERATIONS && !stopped)) {
        it++;
        double L[21], d[6], pivot;
        damped<6>(S.A, lambda, L);
#pragma unroll
        for (int q = 0; q < 6; q++) d[q] = -S.g[q];
        bool better = false, small = false;
        if (uniform(cholesky<6>(L, pivot))) {
            cholesky_solve<6>(L, d);
            double R2[9], t2[3] = {t[0] + d[3], t[1] + d[4], t[2] + d[5]};
            rotate_left(d, R, R2);
            normal_equations(a, fr, lane, R2, t2, S2);
            small = lm_small(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5], pose_norm2(t));
            better = S2.c < S.c;  // (the bare comparison; calibrate.hip's rule also takes a cost within its rounding)
            if (uniform(better)) {
#pragma unroll
                for (int q = 0; q < 9; q++) R[q] = R2[q];
#pragma unroll
                for (int q = 0; q < 3; q++) t[q] = t2[q];
                S = S2;
            }
        }
        lambda = lm_next(lambda, uniform(better));
        stopped = uniform(lm_stopped(small, lambda));
    }
    // a pose is one only where the undamped system has full rank
    double pivot;
    const bool ok = unit_diagonal_pivot<6>(S.A, pivot);
    if (!uniform(ok && pivot >= SINGULAR_PIVOT && isfinite(S.c) && stopped)) status = PNP_SINGULAR;
    store_frame(lane, f, R, t, sqrt(__ddiv_rn(S.c, 2. * fr.n)), it, status, pose, rms_out, iterations_out, status_out);
}

// ---- start pose -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void normalise3(double* v)
{
    const double s = __ddiv_rn(1., sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
    v[0] *= s, v[1] *= s, v[2] *= s;
}

// H or P -> R, t of the target in the camera: scale, the sign that puts the target in front, Gram-Schmidt; poses come
// back in the caller's object frame (planar: through the plane's rotation)
__global__ __launch_bounds__(256) void k_pnp_init(PnpArgs a, double* __restrict__ pose)
{
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= a.p.frames) return;
    const Frame fr = frame_rows(a.p, f, a.min_points);
    bool ok = fr.status == PNP_OK && !frame_nonfinite(a.p, fr, lane);
    double R[9], t[3];
    if (uniform(ok)) {
        if (a.planar) {
            double H[9], c[3];
            ok = direct_linear_transform<3>(a, fr, lane, H, c);
            const double z0 = c[2];
            double c1[3] = {H[0], H[3], H[6]}, c2[3] = {H[1], H[4], H[7]};
            const double n1 = sqrt(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
            const double n2 = sqrt(c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2]);
            double s = __ddiv_rn(2., n1 + n2);
            if (H[6] * c[0] + H[7] * c[1] + H[8] < 0.) s = -s;  // the depth of the points' centre decides the sign
            for (int q = 0; q < 3; q++) c1[q] *= s, c2[q] *= s;
            normalise3(c1);
            const double dot = c1[0] * c2[0] + c1[1] * c2[1] + c1[2] * c2[2];
            for (int q = 0; q < 3; q++) c2[q] -= dot * c1[q];
            normalise3(c2);
            const double c3[3] = {c1[1] * c2[2] - c1[2] * c2[1], c1[2] * c2[0] - c1[0] * c2[2], c1[0] * c2[1] - c1[1] * c2[0]};
            // R' = [c1 c2 c3] takes the plane's frame to the camera; t' = s h3 - c3 z0; R = R' plane
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) R[3 * i + j] = c1[i] * a.plane[j] + c2[i] * a.plane[3 + j] + c3[i] * a.plane[6 + j];
                t[i] = s * H[3 * i + 2] - c3[i] * z0;
            }
        } else {
            double P[12], c[3];
            ok = direct_linear_transform<4>(a, fr, lane, P, c);
            double r3[3] = {P[8], P[9], P[10]}, r1[3] = {P[0], P[1], P[2]};
            double s = __ddiv_rn(1., sqrt(r3[0] * r3[0] + r3[1] * r3[1] + r3[2] * r3[2]));
            if (P[8] * c[0] + P[9] * c[1] + P[10] * c[2] + P[11] < 0.) s = -s;  // the depth of the points' centre decides the sign
            for (int q = 0; q < 3; q++) r3[q] *= s, r1[q] *= s;
            normalise3(r3);
            const double dot = r1[0] * r3[0] + r1[1] * r3[1] + r1[2] * r3[2];
            for (int q = 0; q < 3; q++) r1[q] -= dot * r3[q];
            normalise3(r1);
            const double r2[3] = {r3[1] * r1[2] - r3[2] * r1[1], r3[2] * r1[0] - r3[0] * r1[2], r3[0] * r1[1] - r3[1] * r1[0]};
            for (int q = 0; q < 3; q++) R[q] = r1[q], R[3 + q] = r2[q], R[6 + q] = r3[q], t[q] = s * P[4 * q + 3];
        }
    }
    if (lane == 0) store_pose(pose + (size_t)f * 12, R, t, ok);
}

static int pnp_args(const char* who, const camd_pnp_points* p, const double K[9], const double* dist, int ndist, PnpArgs& a)
{
    const bool bad_dist = (ndist != 0 && ndist != 4 && ndist != 5 && ndist != 8 && ndist != 12 && ndist != 14) || (ndist > 0 && !dist);
    if (!points_ok(p) || !K || bad_dist) {
        set_error("%s: bad arguments (points: object / image rows of CAMD_VALUE_F64 or _F32, aligned to an element, strides >= 3 "
                  "/ >= 2; start: frames + 1 device int64; K is 9 host doubles; ndist is 0, 4, 5, 8, 12 or 14, got %d)", who, ndist);
        return CAMD_ERR_BAD_ARG;
    }
    a.p = *p;
    return unpack_camera(who, K, dist, ndist, &a.cam, &a.k);
}

}  // namespace camd

using namespace camd;

extern "C" {

int camd_pnp_init(const camd_pnp_points* points, const double K[9], const double* dist, int ndist, int planar,
                  const double plane[9], double* pose, void* queue)
{
    PnpArgs a = {};
    int rc = pnp_args("camd_pnp_init", points, K, dist, ndist, a);
    if (rc != CAMD_OK) return rc;
    if ((planar && !plane) || (a.p.frames > 0 && !doubles_ok(pose))) {
        set_error("camd_pnp_init: bad arguments (a planar target needs its plane's rotation, 9 host doubles; pose: frames x 12 "
                  "device doubles)");
        return CAMD_ERR_BAD_ARG;
    }
    a.planar = planar != 0, a.min_points = planar ? 4 : 6;
    for (int q = 0; q < 9; q++) a.plane[q] = planar ? plane[q] : (q % 4 == 0 ? 1. : 0.);
    if (a.p.frames == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_pnp_init, dim3(div_up(a.p.frames, 4)), dim3(256), 0, (hipStream_t)queue, a, pose);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

int camd_pnp_refine(const camd_pnp_points* points, const double K[9], const double* dist, int ndist, int min_points,
                    const double* pose0, int pose0_stride, double* pose, double* rms, int* iterations, int* status, void* queue)
{
    PnpArgs a = {};
    int rc = pnp_args("camd_pnp_refine", points, K, dist, ndist, a);
    if (rc != CAMD_OK) return rc;
    if (min_points < 3 || (pose0_stride != 0 && pose0_stride != 12) ||
        (a.p.frames > 0 && (!doubles_ok(pose0) || !doubles_ok(pose) || !doubles_ok(rms) || !iterations || !status ||
                            (uintptr_t)iterations % 4 != 0 || (uintptr_t)status % 4 != 0))) {
        set_error("camd_pnp_refine: bad arguments (min_points >= 3, got %d; pose0_stride is 12, or 0 for one start pose, got %d; "
                  "pose0, pose, rms, iterations, status: device arrays)", min_points, pose0_stride);
        return CAMD_ERR_BAD_ARG;
    }
    a.min_points = min_points;
    if (a.p.frames == 0) return CAMD_OK;
    CAMD_NEED_DEVICE();
    hipLaunchKernelGGL(k_pnp_refine, dim3(div_up(a.p.frames, 4)), dim3(256), 0, (hipStream_t)queue, a, pose0, pose0_stride, pose,
                       rms, iterations, status);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

}  // extern "C"
