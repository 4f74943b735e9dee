"""A camera's intrinsics from the detected points of a target in many frames, on the GPU (csrc/calibrate.hip).

Replaces ``cv2.calibrateCamera(object_points, image_points, xy, None, None, flags=flags)`` of the reference's
``Cam.calibrate`` (camera.py:63-93) for the 5-coefficient model ``fx fy cx cy | k1 k2 p1 p2 k3``.  The start is cv2's:
one homography per frame (``camd_calib_homography``), the principal point at the image centre and the focal lengths from
the homographies' vanishing points, no lens; start poses from ``camd_pnp_init`` + ``camd_pnp_refine`` under that start.
Then a joint float64 Levenberg-Marquardt over the nine shared unknowns and six per frame, solved through the Schur
complement on the shared block, with ``pnp``'s damping and stopping rules.  Lambda, the costs, the accept decision and
both parameter sets stay on the device; per evaluation the host reads two numbers.  cv2's own iteration is UNPINNED
(DESIGN.md section 2, U29).
"""
import ctypes

import numpy as np

from . import _lm, _native, pnp
from ._arrays import to_caller
from ._lm import STATUS_OK, STATUS_SINGULAR, STATUS_TEXT  # noqa: F401

# cv2's values
CALIB_USE_INTRINSIC_GUESS = 0x00001
CALIB_FIX_ASPECT_RATIO = 0x00002
CALIB_FIX_PRINCIPAL_POINT = 0x00004
CALIB_ZERO_TANGENT_DIST = 0x00008
CALIB_FIX_FOCAL_LENGTH = 0x00010
CALIB_FIX_K1 = 0x00020
CALIB_FIX_K2 = 0x00040
CALIB_FIX_K3 = 0x00080
CALIB_FIX_K4 = 0x00800
CALIB_FIX_K5 = 0x01000
CALIB_FIX_K6 = 0x02000
CALIB_RATIONAL_MODEL = 0x04000
CALIB_THIN_PRISM_MODEL = 0x08000
CALIB_FIX_S1_S2_S3_S4 = 0x10000
CALIB_TILTED_MODEL = 0x40000
CALIB_FIX_TAUX_TAUY = 0x80000
FLAG_NAMES = ["CALIB_USE_INTRINSIC_GUESS", "CALIB_FIX_PRINCIPAL_POINT", "CALIB_FIX_FOCAL_LENGTH", "CALIB_ZERO_TANGENT_DIST",
              "CALIB_FIX_K1", "CALIB_FIX_K2", "CALIB_FIX_K3", "CALIB_FIX_K4", "CALIB_FIX_K5", "CALIB_FIX_K6"]
HONOURED = (CALIB_USE_INTRINSIC_GUESS | CALIB_FIX_PRINCIPAL_POINT | CALIB_FIX_FOCAL_LENGTH | CALIB_ZERO_TANGENT_DIST |
            CALIB_FIX_K1 | CALIB_FIX_K2 | CALIB_FIX_K3)
WITHOUT_EFFECT = CALIB_FIX_K4 | CALIB_FIX_K5 | CALIB_FIX_K6  # coefficients this model does not have
# the reference's ``undistorted=True`` (camera.py:69-79)
UNDISTORTED_FLAGS = (CALIB_ZERO_TANGENT_DIST | CALIB_FIX_K1 | CALIB_FIX_K2 | CALIB_FIX_K3 | CALIB_FIX_K4 | CALIB_FIX_K5 |
                     CALIB_FIX_K6)

FRAME_STATUS_TEXT = {0: "ok", 1: "too few points", 2: "non-finite input", 3: "no start pose"}


def free_mask(flags):
    """1 for a free entry of ``fx fy cx cy k1 k2 p1 p2 k3``, 0 for one the flags fix."""
    m = np.ones(9)
    if flags & CALIB_FIX_FOCAL_LENGTH:
        m[0:2] = 0
    if flags & CALIB_FIX_PRINCIPAL_POINT:
        m[2:4] = 0
    if flags & CALIB_ZERO_TANGENT_DIST:
        m[6:8] = 0
    for bit, at in ((CALIB_FIX_K1, 4), (CALIB_FIX_K2, 5), (CALIB_FIX_K3, 8)):
        if flags & bit:
            m[at] = 0
    return m


def initial_camera_matrix(H, xy):
    """cv2's ``initIntrinsicParams2D``: the principal point at ``((w - 1) / 2, (h - 1) / 2)``; ``1 / fx^2, 1 / fy^2`` by
    least squares (the normal equations) from two equations per homography -- the vanishing points of the plane's axes
    are orthogonal, and so are those of its diagonals.  ``H``: (f, 3, 3), plane -> raw pixels; rows with a NaN are left out."""
    H = np.asarray(H, np.float64).reshape(-1, 3, 3)
    H = H[np.isfinite(H).all((1, 2))]
    cx, cy = (xy[0] - 1) * 0.5, (xy[1] - 1) * 0.5
    A, b = [], []
    for G in H:
        G = G.copy()
        G[0] -= G[2] * cx
        G[1] -= G[2] * cy
        h, v = G[:, 0], G[:, 1]
        d1, d2 = (h + v) * 0.5, (h - v) * 0.5
        h, v, d1, d2 = (a / np.sqrt((a * a).sum()) for a in (h, v, d1, d2))
        A += [[h[0] * v[0], h[1] * v[1]], [d1[0] * d2[0], d1[1] * d2[1]]]
        b += [-h[2] * v[2], -d1[2] * d2[2]]
    A, b = np.array(A).reshape(-1, 2), np.array(b)
    with np.errstate(all="ignore"):
        try:
            f = np.linalg.solve(A.T @ A, A.T @ b)
        except np.linalg.LinAlgError:
            f = np.full(2, np.nan)
        fx, fy = np.sqrt(np.abs(1.0 / f))
    if not (np.isfinite(fx) and np.isfinite(fy)):
        raise ValueError("calibrate_camera: the homographies give no focal length (every frame sees the target head-on?)")
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])


def calibrate_camera(object_points, image_points, xy, counts=None, flags=0, K=None, D=None):
    """``cv2.calibrateCamera`` for ``fx fy cx cy | k1 k2 p1 p2 k3`` -> ``dict(retval, K (3, 3), D (1, 5), T (f, 4, 4),
    reprojection_error (f,), iterations, status (f,), evaluations)``.

    The points are given as in ``solve_pnp_batch``: ``image_points`` (f, n, 2) raw pixels with ``object_points`` (f, n, 3)
    or one shared (n, 3) board, or ragged rows with ``counts``; float32 or float64, ndarrays or CUDA tensors, read in
    place.  ``xy`` = (width, height).  ``K``, ``D`` and ``retval`` are host float64; ``T`` (object -> camera), the per-frame
    ``reprojection_error`` and ``status`` follow the kind of the input.  ``retval = sqrt(sum |r|^2 / N)`` over the N points
    used: cv2's per-POINT RMS, not the per-component RMS of ``solve_pnp_batch`` (which is smaller by sqrt 2); the
    per-frame error is the same quantity over the frame's points.  ``iterations`` counts the accepted steps,
    ``evaluations`` all of them.

    ``flags`` carry cv2's values: ``CALIB_USE_INTRINSIC_GUESS`` (start from ``K`` and, if given, ``D``: the only way in
    for a target with depth), ``CALIB_FIX_PRINCIPAL_POINT``, ``CALIB_FIX_FOCAL_LENGTH``, ``CALIB_ZERO_TANGENT_DIST``,
    ``CALIB_FIX_K1 / K2 / K3``; ``CALIB_FIX_K4 / K5 / K6`` are accepted without effect.  Frame ``status``: 0 ok, 1 fewer than
    4 points, 2 a non-finite coordinate, 3 no start pose; a frame that is not 0 is left out of the joint problem and has
    NaN in R, t and its error.  Refused with ``ValueError`` before the device is touched: any other flag, wrong shapes
    and dtypes, no frame of 4 points, a target with depth without a guess, fewer equations than free unknowns.  A camera
    whose reduced matrix is singular, or whose iteration has not stopped at the cap of evaluations, raises ``ValueError``
    with status 3."""
    import torch
    was_np = pnp.check_points(object_points, image_points)
    flags = int(flags)
    if flags & ~(HONOURED | WITHOUT_EFFECT):
        raise ValueError("calibrate_camera: flags 0x%x are not implemented (honoured: %s)" % (flags & ~(HONOURED | WITHOUT_EFFECT),
                                                                                           ", ".join(FLAG_NAMES)))
    w, h = int(xy[0]), int(xy[1])
    if len(xy) != 2 or w <= 0 or h <= 0:
        raise ValueError("xy must be a positive (width, height), got %s" % (tuple(xy),))
    guess = bool(flags & CALIB_USE_INTRINSIC_GUESS)
    if guess and K is None:
        raise ValueError("CALIB_USE_INTRINSIC_GUESS needs K")
    k0 = np.zeros(9)
    if guess:
        K = np.asarray(K, np.float64)
        if K.shape != (3, 3) or not np.isfinite(K).all():
            raise ValueError("K must be a finite (3, 3) matrix, got shape %s" % (K.shape,))
        k0[:4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        if D is not None:
            Dv = np.asarray(D, np.float64).reshape(-1)
            if Dv.size not in (4, 5) or not np.isfinite(Dv).all():
                raise ValueError("D must hold 4 or 5 finite coefficients (k1 k2 p1 p2 k3), got %d" % Dv.size)
            k0[4:4 + Dv.size] = Dv
    mask = free_mask(flags)
    if flags & CALIB_ZERO_TANGENT_DIST:
        k0[6:8] = 0
    frames, lengths, shared = pnp.batch_layout(object_points, image_points, counts)
    if lengths.max() < 4:
        raise ValueError("every frame has fewer than 4 points")
    planar, plane = pnp.plane_of(object_points if was_np else object_points.detach().cpu().numpy())
    if not planar and not guess:
        raise ValueError("a target with depth needs CALIB_USE_INTRINSIC_GUESS and K: the start comes from a plane's homographies")
    min_points = 4 if planar else 6
    unknowns = lambda n: int(mask.sum()) + 6 * n  # noqa: E731
    enough = lengths >= 4
    if 2 * int(lengths[enough].sum()) < unknowns(int(enough.sum())):
        raise ValueError("singular: %d equations for %d free unknowns" % (2 * int(lengths[enough].sum()), unknowns(int(enough.sum()))))

    pts, dev, alive = pnp.pack_points(object_points, image_points, lengths, shared)
    f64 = dict(dtype=torch.float64, device=dev)
    what = "calibrate_camera"
    if not guess:
        H = torch.empty((frames, 9), **f64)
        _native.call("camd_calib_homography", dev, ctypes.byref(pts), plane.ctypes.data, H.data_ptr(), what=what)
        K0 = initial_camera_matrix(H.cpu().numpy(), (w, h))
        k0[:4] = K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2]
    # start poses under the start intrinsics: the batched PnP as it is
    K0 = np.array([k0[0], 0, k0[2], 0, k0[1], k0[3], 0, 0, 1.0])
    D0 = np.ascontiguousarray(k0[4:])
    poses, status = pnp.start_poses(pts, K0, D0.ctypes.data, 5, planar, plane, min_points, dev, what)
    used_host = np.flatnonzero(status.cpu().numpy() == 0).astype(np.int32)
    n_used, n_points = len(used_host), int(lengths[used_host].sum())
    if n_used == 0:
        raise ValueError("calibrate_camera: status 3 (%s): no frame has a start pose" % STATUS_TEXT[3])
    if 2 * n_points < unknowns(n_used):
        raise ValueError("calibrate_camera: status 3 (%s): %d equations for %d free unknowns" % (STATUS_TEXT[3], 2 * n_points, unknowns(n_used)))
    used = torch.from_numpy(used_host).to(dev)
    cur = poses[used.long()].contiguous()
    host_state = np.zeros(_native.CALIB_STATE_DOUBLES)
    host_state[_native.CALIB_LAMBDA] = 1e-3
    host_state[_native.CALIB_K:_native.CALIB_K + 9] = k0
    host_state[_native.CALIB_MASK:_native.CALIB_MASK + 9] = mask
    state = torch.from_numpy(host_state).to(dev)
    cand = torch.empty((n_used, _native.CALIB_CANDIDATE_DOUBLES), **f64)
    ws = torch.empty((n_used, _native.CALIB_WORKSPACE_DOUBLES), **f64)
    err = torch.empty(n_used, **f64)
    common = (ctypes.byref(pts), used.data_ptr(), n_used, state.data_ptr())
    _lm.iterate(state, dev, what,
                lambda: _native.call("camd_calib_step", dev, *common, cur.data_ptr(), cand.data_ptr(), ws.data_ptr(), what=what),
                lambda: _native.call("camd_calib_linearise", dev, *common, cur.data_ptr(), ws.data_ptr(), what=what))
    _native.call("camd_calib_finish", dev, *common, ws.data_ptr(), err.data_ptr(), what=what)
    s = _lm.read_state(state, dev, _native.CALIB_STATE_DOUBLES, what)
    _lm.check_status(what, s[_native.CALIB_STATUS], s[_native.CALIB_EVALUATIONS], s[_native.CALIB_PIVOT])
    k = s[_native.CALIB_K:_native.CALIB_K + 9]
    T = pnp.poses_to_T(cur, fill=(frames, used.long()))
    error = torch.full((frames,), float("nan"), **f64)
    error[used.long()] = err
    T, error, status = to_caller((T, error, status), was_np)
    return dict(retval=float(np.sqrt(s[_native.CALIB_COST] / n_points)), K=np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]]),
                D=k[4:].reshape(1, 5).copy(), T=T, reprojection_error=error, iterations=int(s[_native.CALIB_ITERATIONS]),
                status=status, evaluations=int(s[_native.CALIB_EVALUATIONS]))
