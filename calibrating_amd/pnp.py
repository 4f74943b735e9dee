"""The pose of a target in every frame of a recording from its detected points: batched PnP on the GPU (csrc/pnp.hip).

Replaces ``cv2.solvePnPGeneric(object_points, image_points[:, None], K, D)`` of the reference's
``Cam.perspective_n_point`` (camera.py:266-273), which solves one frame per call on one CPU thread.  Here all frames go
through one launch of ``camd_pnp_init`` (a start pose from the direct linear transform; skipped with ``T0``) and one of
``camd_pnp_refine`` (a float64 Levenberg-Marquardt per frame, one wavefront each).  Detection of the points stays with
the caller.  cv2's solver is UNPINNED.
"""
import ctypes

import numpy as np

from . import _native
from ._arrays import FLOAT_TYPES, K9, check_array, dist, dtype_name, is_np, to_caller, to_device

STATUS_OK, STATUS_FEW_POINTS, STATUS_NONFINITE, STATUS_SINGULAR = 0, 1, 2, 3
STATUS_TEXT = {0: "ok", 1: "too few points", 2: "non-finite input", 3: "singular or not converged at the cap"}
PLANAR_RATIO = 1e-3  # planar: the smallest singular value of the centred object points below this part of the middle one


def check_points(object_points, image_points):
    """The refusals every entry point begins with -> whether the points are NumPy arrays (CUDA tensors otherwise)."""
    for a, width, what in ((object_points, 3, "object_points"), (image_points, 2, "image_points")):
        check_array(a, what)
        if dtype_name(a) not in FLOAT_TYPES:
            raise ValueError("%s must be float32 or float64, got %s" % (what, a.dtype))
        if a.ndim not in (2, 3) or a.shape[-1] != width:
            raise ValueError("%s must be (n, %d) or (f, n, %d), got %s" % (what, width, width, tuple(a.shape)))
    if is_np(object_points) != is_np(image_points):
        raise TypeError("object_points and image_points must both be NumPy arrays or both be CUDA tensors")
    return is_np(image_points)


def pack_points(object_points, image_points, lengths, shared):
    """The hand-over -> (``camd_pnp_points``, device, the tensors it points into: keep them alive while it is used)."""
    import torch
    img2 = to_device(image_points).reshape(-1, 2)
    obj2 = to_device(object_points, device=img2.device).reshape(-1, 3)
    start = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(img2.device)
    pts = _native.PnpPoints(obj2.data_ptr(), img2.data_ptr(), start.data_ptr(), obj2.shape[0], img2.shape[0],
                            FLOAT_TYPES[dtype_name(obj2)], FLOAT_TYPES[dtype_name(img2)], 3, 2, int(shared), len(lengths))
    return pts, img2.device, (obj2, img2, start)


def poses_to_T(pose, fill=None):
    """(f, 12) R, t -> (f, 4, 4); ``fill = (frames, at)``: they are the frames ``at`` of ``frames``, the others get NaN."""
    frames, at = (len(pose), slice(None)) if fill is None else fill
    T = pose.new_zeros((frames, 4, 4))
    if fill is not None:
        T[:, :3] = float("nan")
    T[at, :3, :3] = pose[:, :9].view(-1, 3, 3)
    T[at, :3, 3] = pose[:, 9:]
    T[:, 3, 3] = 1
    return T


def plane_of(object_points):
    """(planar, rotation): one float64 SVD of the centred object points.  Planar when the smallest singular value is below
    ``PLANAR_RATIO`` of the middle one; the rotation's rows are the principal axes, the plane's normal last, so that it
    lays the plane on z = const (the identity when z is constant already)."""
    X = np.asarray(object_points, np.float64).reshape(-1, 3)
    X = X[np.isfinite(X).all(1)]
    if len(X) < 3:
        return False, np.eye(3)
    if np.ptp(X[:, 2]) == 0:  # a board in its own coordinates: no rotation, so the start pose of a frame does not depend on
        return True, np.eye(3)  # which other frames share its batch (the SVD's bits would)
    _, s, Vt = np.linalg.svd(X - X.mean(0), full_matrices=False)
    if np.linalg.det(Vt) < 0:
        Vt = Vt * np.array([[1.0], [1.0], [-1.0]])
    return bool(s[2] < PLANAR_RATIO * s[1]), np.ascontiguousarray(Vt)


def batch_layout(object_points, image_points, counts):
    """(frames, lengths (frames,) int64, shared) of the three ways a batch is given: (f, n, .) with per-frame or one shared
    block of object points, or ragged rows with ``counts``.  Refuses everything else; nothing touches the device."""
    shared = False
    if counts is None:
        if image_points.ndim != 3:
            raise ValueError("image_points must be (f, n, 2) unless counts is given, got %s" % (tuple(image_points.shape),))
        frames, n = int(image_points.shape[0]), int(image_points.shape[1])
        shared = object_points.ndim == 2
        if tuple(object_points.shape) != ((n, 3) if shared else (frames, n, 3)):
            raise ValueError("object_points must be (%d, %d, 3) or a shared (%d, 3), got %s" % (frames, n, n, tuple(object_points.shape)))
        lengths = np.full(frames, n, np.int64)
    else:
        lengths = np.asarray(counts)
        if image_points.ndim != 2 or object_points.ndim != 2:
            raise ValueError("with counts, the points are ragged rows (N, 2) and (N, 3)")
        if lengths.ndim != 1 or lengths.dtype.kind not in "iu" or (lengths < 0).any():
            raise ValueError("counts must be a 1-d array of non-negative integers")
        lengths = lengths.astype(np.int64)
        frames = len(lengths)
        if int(lengths.sum()) != image_points.shape[0] or object_points.shape[0] != image_points.shape[0]:
            raise ValueError("counts sum to %d rows, the points have %d and %d" % (lengths.sum(), image_points.shape[0], object_points.shape[0]))
    if frames == 0:
        raise ValueError("no frames")
    return frames, lengths, shared


def start_poses(pts, K, dist_ptr, ndist, planar, plane, min_points, dev, what):
    """The batched PnP as it is, for a joint solver's start: ``camd_pnp_init`` + ``camd_pnp_refine`` under ``K`` (9 host
    doubles) and ``ndist`` coefficients at ``dist_ptr`` -> (poses (frames, 12) float64, status (frames,) int32), on ``dev``."""
    import torch
    f64 = dict(dtype=torch.float64, device=dev)
    pose0, poses = torch.empty((pts.frames, 12), **f64), torch.empty((pts.frames, 12), **f64)
    rms, its = torch.empty(pts.frames, **f64), torch.empty(pts.frames, dtype=torch.int32, device=dev)
    status = torch.empty(pts.frames, dtype=torch.int32, device=dev)
    _native.call("camd_pnp_init", dev, ctypes.byref(pts), K.ctypes.data, dist_ptr, ndist, int(planar), plane.ctypes.data,
                 pose0.data_ptr(), what=what)
    _native.call("camd_pnp_refine", dev, ctypes.byref(pts), K.ctypes.data, dist_ptr, ndist, min_points, pose0.data_ptr(), 12,
                 poses.data_ptr(), rms.data_ptr(), its.data_ptr(), status.data_ptr(), what=what)
    return poses, status


def _start_poses(T0, frames):
    T0 = np.asarray(T0, np.float64)
    if T0.shape not in ((4, 4), (frames, 4, 4)):
        raise ValueError("T0 must be (4, 4) or (%d, 4, 4), got %s" % (frames, T0.shape))
    T = T0.reshape(-1, 4, 4)
    return np.ascontiguousarray(np.concatenate([T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]], 1))


def solve_pnp_batch(object_points, image_points, K, D=None, counts=None, T0=None):
    """Poses of one target in ``f`` frames -> ``dict(T=(f, 4, 4) float64, reprojection_error=(f,) float64, iterations=(f,)
    int32, status=(f,) int32)``, ndarrays for ndarray points and CUDA tensors for CUDA tensors.

    ``image_points``: (f, n, 2) raw pixels with ``object_points`` (f, n, 3) or one shared (n, 3) block (one board); or
    ragged rows (N, 2) / (N, 3) with ``counts``, the ``f`` frame lengths.  float32 or float64, read in place.  ``T0``,
    (f, 4, 4) or (4, 4) on the host, starts the refinement and skips the initialisation (tracking: the previous frame's
    pose).  A batch is one target: planarity is decided once for all its object points (``plane_of``).

    ``T`` takes object coordinates into the camera.  ``reprojection_error`` is the RMS over the 2n residual components
    in pixels.  ``status``: 0 ok, 1 too few points in that frame, 2 a non-finite coordinate, 3 singular or not converged
    within 100 evaluations; a frame whose status is not 0 has NaN in R and t (the three
    upper rows of ``T``) and in the error.  Refused before the device is
    touched: wrong shapes and dtypes, tilted-sensor coefficients, and a batch without one frame of at least 4 points; and
    before anything is launched: a batch of a target with depth, without ``T0``, that has no frame of 6 points (CUDA
    object points are read back once for the planarity test; with ``T0`` nothing is)."""
    import torch
    was_np = check_points(object_points, image_points)
    Dv, dptr, nd = dist(D)
    if nd not in (0, 4, 5, 8, 12, 14):
        raise ValueError("D must hold 0, 4, 5, 8, 12 or 14 coefficients, got %d" % nd)
    if nd == 14 and (Dv[12] != 0 or Dv[13] != 0):
        raise ValueError("tilted-sensor distortion (tauX, tauY) not implemented")
    Kf = K9(K)
    frames, lengths, shared = batch_layout(object_points, image_points, counts)
    pose0 = None if T0 is None else _start_poses(T0, frames)
    if lengths.max() < 4:
        raise ValueError("every frame has fewer than 4 points")
    if pose0 is not None:
        planar, plane, min_points = False, np.eye(3), 4  # a start pose is given: the plane is never used, nothing is copied
    else:
        # planarity is a property of the batch, decided on the host: for CUDA points one read-back of the object rows
        # (a shared board: its n rows), no launch
        planar, plane = plane_of(object_points if was_np else object_points.detach().cpu().numpy())
        min_points = 4 if planar else 6
        if lengths.max() < min_points:
            raise ValueError("every frame has fewer than 6 points (non-planar target)")

    pts, dev, alive = pack_points(object_points, image_points, lengths, shared)
    pose = torch.empty((frames, 12), dtype=torch.float64, device=dev)
    rms = torch.empty(frames, dtype=torch.float64, device=dev)
    iterations = torch.empty(frames, dtype=torch.int32, device=dev)
    status = torch.empty(frames, dtype=torch.int32, device=dev)
    if pose0 is None:
        start_pose, stride = torch.empty((frames, 12), dtype=torch.float64, device=dev), 12
        _native.call("camd_pnp_init", dev, ctypes.byref(pts), Kf.ctypes.data, dptr, nd, int(planar), plane.ctypes.data,
                     start_pose.data_ptr(), what="solve_pnp_batch")
    else:
        start_pose, stride = torch.from_numpy(pose0).to(dev), (12 if len(pose0) > 1 or frames == 1 else 0)
    _native.call("camd_pnp_refine", dev, ctypes.byref(pts), Kf.ctypes.data, dptr, nd, min_points, start_pose.data_ptr(), stride,
                 pose.data_ptr(), rms.data_ptr(), iterations.data_ptr(), status.data_ptr(), what="solve_pnp_batch")
    T, rms, iterations, status = to_caller((poses_to_T(pose), rms, iterations, status), was_np)
    return dict(T=T, reprojection_error=rms, iterations=iterations, status=status)
