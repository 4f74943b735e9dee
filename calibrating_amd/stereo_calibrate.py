"""A rig's ``R, t`` (camera 1 -> camera 2) from the points both cameras detected, on the GPU (csrc/stereo_calibrate.hip).

Replaces ``cv2.stereoCalibrate(object_points, image_points1, image_points2, K1, D1, K2, D2, xy, flags=CALIB_FIX_INTRINSIC)``
of the reference's ``Stereo.get_R_t_by_stereo_calibrate`` (stereo_camera.py:95-123).  The start is cv2's: the batched PnP
(``camd_pnp_init`` + ``camd_pnp_refine``) in each camera, per frame ``T2_i inv(T1_i)`` as a Rodrigues vector and a
translation, and the component-wise median over the frames.  Then a joint float64 Levenberg-Marquardt over the rig's six
unknowns and six per frame (the board in camera 1), solved through the Schur complement on the rig's block, with
``calibrate_camera``'s damping, acceptance and stopping rules.  Lambda, the costs, the accept decision and both rigs stay
on the device; per evaluation the host reads two numbers.  cv2's own iteration and its 1e-5 stop are UNPINNED (DESIGN.md
section 2, U30).
"""
import ctypes

import numpy as np

from . import _lm, _native, geometry, pnp
from ._arrays import K9, dist, dtype_name, to_caller, to_device
from ._lm import STATUS_OK, STATUS_SINGULAR, STATUS_TEXT  # noqa: F401

# cv2's values
CALIB_FIX_INTRINSIC = 0x00100
CALIB_USE_EXTRINSIC_GUESS = 0x400000

FRAME_STATUS_TEXT = {0: "ok", 1: "too few points", 2: "non-finite input in either camera", 3: "no start pose in either camera"}


def _camera(K, D, which):
    Kn = np.asarray(K, np.float64)
    if Kn.shape != (3, 3) or not np.isfinite(Kn).all():
        raise ValueError("K%d must be a finite (3, 3) matrix, got shape %s" % (which, Kn.shape))
    Dv, dptr, nd = dist(D)
    if nd not in (0, 4, 5, 8, 12, 14):
        raise ValueError("D%d must hold 0, 4, 5, 8, 12 or 14 coefficients, got %d" % (which, nd))
    if nd == 14 and (Dv[12] != 0 or Dv[13] != 0):
        raise ValueError("D%d: tilted-sensor distortion (tauX, tauY) not implemented" % which)
    return K9(Kn), Dv, dptr, nd


def rig_start(T1, T2):
    """cv2's start of the rig from the start poses both cameras solved, (m, 4, 4) each: per frame ``T2 inv(T1)``, its
    Rodrigues vector and translation; the component-wise median -> (R (3, 3), t (3,)).  Host, ``geometry``'s 3 x 3 algebra."""
    rs, ts = [], []
    for A, B in zip(np.asarray(T1, np.float64), np.asarray(T2, np.float64)):
        R = B[:3, :3] @ A[:3, :3].T
        rs.append(geometry.rodrigues(R).reshape(3))
        ts.append(B[:3, 3] - R @ A[:3, 3])
    return geometry.rodrigues(np.median(np.array(rs), axis=0)), np.median(np.array(ts), axis=0)


def stereo_calibrate(object_points, image_points1, image_points2, K1, D1, K2, D2, counts=None, flags=CALIB_FIX_INTRINSIC,
                     R=None, t=None):
    """``cv2.stereoCalibrate`` with both cameras' intrinsics fixed -> ``dict(retval, R (3, 3), t (3, 1), T (f, 4, 4),
    reprojection_error (f,), iterations, status (f,), evaluations)``.

    The points are given as in ``calibrate_camera``: ``image_points1`` / ``image_points2`` (f, n, 2) raw pixels of camera
    1 / camera 2 with ``object_points`` (f, n, 3) or one shared (n, 3) board, or ragged rows with ``counts``; float32 or
    float64, ndarrays or CUDA tensors, read in place.  The two image arrays agree in shape, dtype and kind.  ``D1``, ``D2``:
    whatever ``solve_pnp_batch`` accepts.  ``R``, ``t`` (``x2 = R x1 + t``, cv2's convention) and ``retval`` are host
    float64; ``T`` (the board in camera 1), the per-frame ``reprojection_error`` and ``status`` follow the kind of the
    input.  ``retval = sqrt(sum (|r1|^2 + |r2|^2) / 2N)`` over the N board points used, cv2's definition; the per-frame
    error is the same quantity over the frame's points.  ``E`` and ``F`` are not returned (the reference discards them).

    ``flags``: ``CALIB_FIX_INTRINSIC`` is required; with ``CALIB_USE_EXTRINSIC_GUESS`` the iteration starts from ``R``,
    ``t`` instead of the median of the frames' own.  Frame ``status``: 0 ok, 1 too few points, 2 a non-finite coordinate
    in either camera, 3 no start pose in either camera; a frame that is not 0 is left out of the joint problem and has NaN
    in ``T`` and its error, and the rest is, bit for bit, the call without it.  Refused with ``ValueError`` before the device is
    touched: any other flag or a call without ``CALIB_FIX_INTRINSIC``, wrong shapes and dtypes, image arrays that disagree,
    a ``K`` that is not a finite 3 x 3, a ``D`` the PnP refuses, no frame with the PnP's minimum of points, the guess flag
    without ``R, t``.  A rig whose reduced matrix is singular, or whose iteration has not stopped at the cap of 100
    evaluations, raises ``ValueError`` with status 3."""
    import torch
    what = "stereo_calibrate"
    was_np = pnp.check_points(object_points, image_points1)
    if pnp.check_points(object_points, image_points2) != was_np or tuple(image_points1.shape) != tuple(image_points2.shape) or \
            dtype_name(image_points1) != dtype_name(image_points2):
        raise ValueError("image_points1 and image_points2 must agree in shape, dtype and kind, got %s %s and %s %s"
                         % (tuple(image_points1.shape), image_points1.dtype, tuple(image_points2.shape), image_points2.dtype))
    flags = int(flags)
    if not flags & CALIB_FIX_INTRINSIC:
        raise ValueError("stereo_calibrate: CALIB_FIX_INTRINSIC is required (both cameras' K and D stay as given)")
    if flags & ~(CALIB_FIX_INTRINSIC | CALIB_USE_EXTRINSIC_GUESS):
        raise ValueError("stereo_calibrate: flags 0x%x are not implemented (honoured: CALIB_FIX_INTRINSIC, CALIB_USE_EXTRINSIC_GUESS)"
                         % (flags & ~(CALIB_FIX_INTRINSIC | CALIB_USE_EXTRINSIC_GUESS)))
    guess = bool(flags & CALIB_USE_EXTRINSIC_GUESS)
    if guess:
        if R is None or t is None:
            raise ValueError("CALIB_USE_EXTRINSIC_GUESS needs R and t")
        R0, t0 = np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(-1)
        if R0.shape != (3, 3) or t0.shape != (3,) or not (np.isfinite(R0).all() and np.isfinite(t0).all()):
            raise ValueError("R must be a finite (3, 3) matrix and t hold 3 finite numbers, got shapes %s and %s" % (R0.shape, t0.shape))
    cams = [_camera(K1, D1, 1), _camera(K2, D2, 2)]
    frames, lengths, shared = pnp.batch_layout(object_points, image_points1, counts)
    if lengths.max() < 4:
        raise ValueError("every frame has fewer than 4 points")
    planar, plane = pnp.plane_of(object_points if was_np else object_points.detach().cpu().numpy())
    min_points = 4 if planar else 6
    if lengths.max() < min_points:
        raise ValueError("every frame has fewer than 6 points (non-planar target)")

    pts1, dev, alive1 = pnp.pack_points(object_points, image_points1, lengths, shared)
    img2 = to_device(image_points2, device=dev).reshape(-1, 2)  # camera 2 shares camera 1's object rows and start
    pts2 = _native.PnpPoints(pts1.object, img2.data_ptr(), pts1.start, pts1.object_rows, img2.shape[0], pts1.object_type,
                             pts1.image_type, 3, 2, pts1.object_shared, pts1.frames)
    f64 = dict(dtype=torch.float64, device=dev)
    # start poses: the batched PnP as it is, once per camera
    start, status = [], []
    for p, (Kf, _, dptr, nd) in zip((pts1, pts2), cams):
        pose, st = pnp.start_poses(p, Kf, dptr, nd, planar, plane, min_points, dev, what)
        start.append(pose), status.append(st)
    s1, s2 = status[0].cpu().numpy(), status[1].cpu().numpy()
    # 1 and 2 are properties of the rows (the object rows and the counts are shared: 1 comes from both or neither)
    host_status = np.where(s1 == 1, 1, np.where((s1 == 2) | (s2 == 2), 2, np.where((s1 != 0) | (s2 != 0), 3, 0))).astype(np.int32)
    used_host = np.flatnonzero(host_status == 0).astype(np.int32)
    n_used, n_points = len(used_host), int(lengths[used_host].sum())
    if n_used == 0:
        raise ValueError("stereo_calibrate: status 3 (%s): no frame has a start pose in both cameras" % STATUS_TEXT[3])
    used = torch.from_numpy(used_host).to(dev)
    cur = start[0][used.long()].contiguous()
    if not guess:
        R0, t0 = rig_start(pnp.poses_to_T(cur).cpu().numpy(), pnp.poses_to_T(start[1][used.long()]).cpu().numpy())
    host_state = np.zeros(_native.STEREO_STATE_DOUBLES)
    host_state[_native.STEREO_LAMBDA] = 1e-3
    host_state[_native.STEREO_RIG:_native.STEREO_RIG + 9] = np.asarray(R0, np.float64).reshape(9)
    host_state[_native.STEREO_RIG + 9:_native.STEREO_RIG + 12] = t0
    state = torch.from_numpy(host_state).to(dev)
    cand = torch.empty((n_used, _native.STEREO_CANDIDATE_DOUBLES), **f64)
    ws = torch.empty((n_used, _native.STEREO_WORKSPACE_DOUBLES), **f64)
    partials = torch.empty(((n_used + 63) // 64, _native.STEREO_PARTIAL_DOUBLES), **f64)
    err = torch.empty(n_used, **f64)
    rig = _native.StereoRig(pts1, pts2, cams[0][0].ctypes.data, cams[0][2], cams[1][0].ctypes.data, cams[1][2], used.data_ptr(),
                            state.data_ptr(), cur.data_ptr(), cand.data_ptr(), ws.data_ptr(), partials.data_ptr(), err.data_ptr(),
                            cams[0][3], cams[1][3], n_used, 0)
    # (a linearisation after a step that was taken gives the frames their candidates first)
    _lm.iterate(state, dev, what, lambda: _native.call("camd_stereo_step", dev, ctypes.byref(rig), what=what),
                lambda: _native.call("camd_stereo_linearise", dev, ctypes.byref(rig), what=what))
    _native.call("camd_stereo_finish", dev, ctypes.byref(rig), what=what)
    s = _lm.read_state(state, dev, _native.STEREO_STATE_DOUBLES, what)
    _lm.check_status(what, s[_native.STEREO_STATUS], s[_native.STEREO_EVALUATIONS], s[_native.STEREO_PIVOT])
    T = pnp.poses_to_T(cur, fill=(frames, used.long()))
    error = torch.full((frames,), float("nan"), **f64)
    error[used.long()] = err
    frame_status = torch.from_numpy(host_status).to(dev)
    T, error, frame_status = to_caller((T, error, frame_status), was_np)
    rig_pose = s[_native.STEREO_RIG:_native.STEREO_RIG + 12]
    return dict(retval=float(np.sqrt(s[_native.STEREO_COST] / (2.0 * n_points))), R=rig_pose[:9].reshape(3, 3).copy(),
                t=rig_pose[9:].reshape(3, 1).copy(), T=T, reprojection_error=error, iterations=int(s[_native.STEREO_ITERATIONS]),
                status=frame_status, evaluations=int(s[_native.STEREO_EVALUATIONS]))
