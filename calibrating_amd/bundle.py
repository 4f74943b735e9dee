"""The poses of N views and one world point per match refined together on the GPU (csrc/bundle.hip): the joint refinement
after ``ReconstructionExtrinsics``' propagation.  The reference has none; the contract is this project's own
(DESIGN.md section 4.3n).

Every match of a pair ``(a, b)`` is one world point with exactly two observations (tracks over three or more views are not
represented: ``set2ds`` does not carry them).  A float64 Levenberg-Marquardt on pixel residuals over three unknowns per
used match and six per view, solved through the Schur complement on the views' block, with ``calibrate_camera``'s damping,
acceptance and stopping rules.  Lambda, the costs, the accept decision and both sets of poses stay on the device; per
evaluation the host reads two numbers.
"""
import ctypes

import numpy as np

from . import _lm, _native
from ._arrays import FLOAT_TYPES, check_array, dtype_name, is_np, to_caller, to_device
from ._lm import STATUS_OK, STATUS_SINGULAR, STATUS_TEXT  # noqa: F401

MATCH_STATUS_TEXT = {0: "ok", 1: "a non-finite coordinate", 2: "no start point: the rays are nearly parallel or meet behind a view",
                     3: "the start's reprojection error exceeds the threshold"}
MIN_VIEWS, MAX_VIEWS = 3, _native.BUNDLE_MAX_VIEWS
MIN_OBSERVATIONS = 6  # used observations a view needs: as many as it has unknowns


def poses_from_T(T):
    """camera to world (N, 4, 4) -> world to camera R (N, 3, 3), t (N, 3): ``R = T[:3, :3]^T``, ``t = -R c``"""
    R = np.ascontiguousarray(np.swapaxes(T[:, :3, :3], 1, 2))
    c = T[:, :3, 3]
    t = -np.stack([R[:, i, 0] * c[:, 0] + R[:, i, 1] * c[:, 1] + R[:, i, 2] * c[:, 2] for i in range(3)], 1)
    return R, t


def T_from_poses(R, t):
    T = np.zeros((len(R), 4, 4))
    T[:, 3, 3] = 1
    T[:, :3, :3] = np.swapaxes(R, 1, 2)
    T[:, :3, 3] = -np.stack([R[:, 0, j] * t[:, 0] + R[:, 1, j] * t[:, 1] + R[:, 2, j] * t[:, 2] for j in range(3)], 1)
    return T


def gauge(T, fixed_view):
    """(anchor view, axis): the view whose start centre is farthest from the fixed view's and the coordinate of largest
    magnitude of ``c_anchor - c_fixed``, which the anchor keeps; ties go to the lower view and the lower axis."""
    c = T[:, :3, 3]
    d2 = ((c - c[fixed_view]) ** 2).sum(1)
    d2[fixed_view] = -1.0
    anchor = int(np.argmax(d2))
    return anchor, int(np.argmax(np.abs(c[anchor] - c[fixed_view])))


def check_arguments(K, T, pairs, uvs_a, uvs_b, counts, fixed_view=0, threshold=None):
    """Every refusal that needs no device -> (K (N, 3, 3), T (N, 4, 4), pairs (P, 2) int32, counts (P,) int64, was_np)."""
    K, T = np.asarray(K, np.float64), np.asarray(T, np.float64)
    if K.ndim != 3 or K.shape[1:] != (3, 3) or T.shape != (K.shape[0], 4, 4):
        raise ValueError("K must be (N, 3, 3) and T (N, 4, 4), got %s and %s" % (K.shape, T.shape))
    N = K.shape[0]
    if not MIN_VIEWS <= N <= MAX_VIEWS:
        raise ValueError("bundle_adjust_pairs takes %d .. %d views, got %d (the reduced system of more views does not fit one "
                         "workgroup's LDS)" % (MIN_VIEWS, MAX_VIEWS, N))
    if not (np.isfinite(K).all() and np.isfinite(T).all()):
        raise ValueError("K and T must be finite")
    if isinstance(fixed_view, bool) or int(fixed_view) != fixed_view or not 0 <= int(fixed_view) < N:
        raise ValueError("fixed_view must be a view 0 .. %d, got %r" % (N - 1, fixed_view))
    if threshold is not None and not float(threshold) >= 0:
        raise ValueError("threshold must be None or >= 0 pixels, got %r" % (threshold,))
    pairs = np.asarray(pairs)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1 or pairs.dtype.kind not in "iu":
        raise ValueError("pairs must be (P, 2) integers with P >= 1, got shape %s dtype %s" % (pairs.shape, pairs.dtype))
    pairs = pairs.astype(np.int64)
    if (pairs < 0).any() or (pairs >= N).any():
        raise ValueError("a pair names a view outside 0 .. %d" % (N - 1))
    if (pairs[:, 0] >= pairs[:, 1]).any():
        raise ValueError("every pair (a, b) must have a < b")
    if len({(int(a), int(b)) for a, b in pairs}) != len(pairs):
        raise ValueError("a pair is given more than once")
    missing = sorted(set(range(N)) - set(int(v) for v in pairs.reshape(-1)))
    if missing:
        raise ValueError("views %s are touched by no pair" % missing)
    check_array(uvs_a, "uvs_a")
    check_array(uvs_b, "uvs_b")
    was_np = is_np(uvs_a)
    if is_np(uvs_b) != was_np or tuple(uvs_a.shape) != tuple(uvs_b.shape) or dtype_name(uvs_a) != dtype_name(uvs_b):
        raise ValueError("uvs_a and uvs_b must agree in shape, dtype and kind, got %s %s and %s %s"
                         % (tuple(uvs_a.shape), uvs_a.dtype, tuple(uvs_b.shape), uvs_b.dtype))
    if len(uvs_a.shape) != 2 or uvs_a.shape[1] != 2 or dtype_name(uvs_a) not in FLOAT_TYPES:
        raise ValueError("uvs_a and uvs_b must be (M, 2) float32 or float64, got %s %s" % (tuple(uvs_a.shape), uvs_a.dtype))
    counts = np.asarray(counts)
    if counts.shape != (len(pairs),) or counts.dtype.kind not in "iu" or (counts < 0).any():
        raise ValueError("counts must be (P,) non-negative integers, got shape %s dtype %s" % (counts.shape, counts.dtype))
    counts = counts.astype(np.int64)
    M = int(uvs_a.shape[0])
    if int(counts.sum()) != M:
        raise ValueError("counts sum to %d, uvs_a has %d rows" % (int(counts.sum()), M))
    if not 1 <= M < 2 ** 31:
        raise ValueError("1 <= M < 2^31 matches are required, got %d" % M)
    return K, T, pairs.astype(np.int32), counts, was_np


def _segments(counts):
    """(first row, rows) of the compaction's segments: a pair's rows in runs of BUNDLE_SEGMENT, never across two pairs"""
    first, n, at, W = [], [], 0, _native.BUNDLE_SEGMENT
    for c in counts:
        for s in range(0, int(c), W):
            first.append(at + s)
            n.append(min(W, int(c) - s))
        at += int(c)
    return np.array(first, np.int64), np.array(n, np.int32)


def _chunks(used_counts):
    """(chunk table (chunks, 4) int32, the pairs' chunk ranges (P + 1,) int64)"""
    table, ranges, at, C = [], [0], 0, _native.BUNDLE_CHUNK
    for p, c in enumerate(used_counts):
        for s in range(0, int(c), C):
            table.append((p, at + s, min(C, int(c) - s), 0))
        at += int(c)
        ranges.append(len(table))
    return np.array(table, np.int32).reshape(-1, 4), np.array(ranges, np.int64)


def bundle_adjust_pairs(K, T, pairs, uvs_a, uvs_b, counts, fixed_view=0, threshold=None, return_points=True, return_start=False,
                        return_rows=False, view_labels=None):
    """Refine the camera-to-world poses ``T`` (N, 4, 4) of N views (3 .. 16) with intrinsics ``K`` (N, 3, 3) and one world point
    per match from the matched pinhole pixels of P pairs ``pairs[p] = (a, b)``, ``a < b``: ``uvs_a`` / ``uvs_b`` (M, 2) float32
    or float64, ndarrays or CUDA tensors read in place, the pairs' rows one after the other, ``counts`` (P,) rows each.  The
    pixels are undistorted (what ``EssentialMatrixStereo`` takes): the residual has no lens.

    -> ``dict(T (N, 4, 4), points (M, 3), status (M,) int32, retval, cost0, cost, pair_error (P,), iterations, evaluations,
    anchor=(view, axis))``.  ``status``: 0 used, 1 a non-finite coordinate, 2 no start point (the midpoint of the two rays
    lies at ``z <= 0`` in either view, or ``|d_a x d_b| < 0.03`` for the unit rays, a triangulation angle under 1.7 degrees), 3 the start's reprojection error exceeds
    ``threshold`` pixels in either view (only when ``threshold`` is given).  The used matches are decided once; the rest is,
    bit for bit, the call without them.  ``points`` is NaN where the status is not 0 (``None`` with ``return_points=False``);
    ``retval`` and ``pair_error`` are the RMS pixel residual over all / the pair's used observations.  ``points``,
    ``status`` and ``pair_error`` follow the kind of the input; ``T``, ``retval`` and the costs are host float64.

    The gauge: view ``fixed_view`` keeps its pose; the view whose start centre is farthest from it (``anchor[0]``) keeps
    coordinate ``anchor[1]`` of its centre, the one of largest magnitude of ``c_anchor - c_fixed``.

    ``ValueError`` before the device is touched: N outside 3 .. 16; a pair out of range, repeated or with ``a >= b``; shapes
    or dtypes that disagree; ``counts`` that do not sum to M; a non-finite ``K`` or ``T``; a view no pair touches;
    ``fixed_view`` that is no view.  After the start: a view left with fewer than 6 used observations; at the end: a
    singular reduced matrix or no stop after 100 evaluations (status 3, with the smallest pivot).

    ``return_start`` adds ``start`` (M, 3), the start points; ``return_rows`` adds ``rows_a`` / ``rows_b`` (used, 4) float64,
    ``[u, v, z, other view]`` of every used point in view a / b of its pair, and ``used_counts`` (P,); ``view_labels`` (N,)
    are the numbers written for the views there (default: their indices)."""
    import torch
    what = "bundle_adjust_pairs"
    K, T, pairs, counts, was_np = check_arguments(K, T, pairs, uvs_a, uvs_b, counts, fixed_view, threshold)
    N, P, M = len(K), len(pairs), int(uvs_a.shape[0])
    labels = np.arange(N, dtype=np.float64) if view_labels is None else np.asarray(view_labels, np.float64).reshape(-1)
    if labels.shape != (N,):
        raise ValueError("view_labels must hold one number per view")
    fixed_view = int(fixed_view)
    anchor, axis = gauge(T, fixed_view)
    R0, t0 = poses_from_T(T)

    name = dtype_name(uvs_a)
    ua = to_device(uvs_a, dtype=name)
    dev = ua.device
    ub = to_device(uvs_b, dtype=name, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    host_state = np.zeros(_native.BUNDLE_STATE_DOUBLES)
    host_state[_native.BUNDLE_LAMBDA] = 1e-3
    host_state[_native.BUNDLE_FIXED], host_state[_native.BUNDLE_ANCHOR], host_state[_native.BUNDLE_AXIS] = fixed_view, anchor, axis
    host_state[_native.BUNDLE_LABEL:_native.BUNDLE_LABEL + N] = labels
    poses = np.concatenate([R0.reshape(N, 9), t0], 1)
    host_state[_native.BUNDLE_POSES:_native.BUNDLE_POSES + 12 * N] = poses.reshape(-1)
    host_state[_native.BUNDLE_K:_native.BUNDLE_K + 4 * N] = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1).reshape(-1)
    state = torch.from_numpy(host_state).to(dev)
    seg_first, seg_n = _segments(counts)
    pair_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    d_pairs, d_start = torch.from_numpy(pairs.reshape(-1).copy()).to(dev), torch.from_numpy(pair_start).to(dev)
    d_seg_first, d_seg_n = torch.from_numpy(seg_first).to(dev), torch.from_numpy(seg_n).to(dev)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    points = torch.empty((M, 3), **f64)
    rowoff = torch.empty(len(seg_n) + 1, dtype=torch.int64, device=dev)
    rowcount = torch.empty(len(seg_n), dtype=torch.int32, device=dev)
    b = _native.Bundle()
    b.uv_a, b.uv_b, b.pair_views, b.pair_start = ua.data_ptr(), ub.data_ptr(), d_pairs.data_ptr(), d_start.data_ptr()
    b.seg_first, b.seg_n, b.status, b.points = d_seg_first.data_ptr(), d_seg_n.data_ptr(), status.data_ptr(), points.data_ptr()
    b.rowoff, b.rowcount, b.state = rowoff.data_ptr(), rowcount.data_ptr(), state.data_ptr()
    b.threshold = -1.0 if threshold is None else float(threshold)
    b.matches, b.uv_type, b.views, b.pairs, b.segments = M, FLOAT_TYPES[name], N, P, len(seg_n)
    _native.call("camd_bundle_start", dev, ctypes.byref(b), int(counts.max()), what=what)
    start = points.clone() if return_start else None

    # the used matches of every pair: the scan at the pairs' first segments
    off = rowoff.cpu().numpy()
    seg_of_pair = np.concatenate([[0], np.cumsum((counts + _native.BUNDLE_SEGMENT - 1) // _native.BUNDLE_SEGMENT)])
    used_counts = np.diff(off[seg_of_pair]).astype(np.int64)
    U = int(off[-1])
    observations = np.zeros(N, np.int64)
    np.add.at(observations, pairs[:, 0], used_counts)
    np.add.at(observations, pairs[:, 1], used_counts)
    for v in range(N):
        if observations[v] < MIN_OBSERVATIONS:
            raise ValueError("%s: view %d is left with %d used observations (at least %d are needed)"
                             % (what, v, observations[v], MIN_OBSERVATIONS))
    table, ranges = _chunks(used_counts)
    d_table, d_ranges = torch.from_numpy(table.reshape(-1).copy()).to(dev), torch.from_numpy(ranges).to(dev)
    cua, cub = torch.empty((U, 2), dtype=ua.dtype, device=dev), torch.empty((U, 2), dtype=ua.dtype, device=dev)
    X, Xc = torch.empty((U, 3), **f64), torch.empty((U, 3), **f64)
    src = torch.empty(U, dtype=torch.int64, device=dev)
    chunks = len(table)
    partials = torch.empty((chunks, _native.BUNDLE_PARTIAL_DOUBLES), **f64)
    pair_blocks = torch.empty((P, _native.BUNDLE_PARTIAL_DOUBLES), **f64)
    eval_partials = torch.empty((chunks, _native.BUNDLE_EVAL_DOUBLES), **f64)
    eval_blocks = torch.empty((P, _native.BUNDLE_EVAL_DOUBLES), **f64)
    pair_error = torch.empty(P, **f64)
    rows_a = rows_b = None
    if return_rows:
        rows_a, rows_b = torch.empty((U, 4), **f64), torch.empty((U, 4), **f64)
        b.rows_a, b.rows_b = rows_a.data_ptr(), rows_b.data_ptr()
    b.chunk_table, b.pair_chunk, b.uv_used_a, b.uv_used_b = d_table.data_ptr(), d_ranges.data_ptr(), cua.data_ptr(), cub.data_ptr()
    b.X, b.candidate, b.src, b.partials, b.pair_blocks = X.data_ptr(), Xc.data_ptr(), src.data_ptr(), partials.data_ptr(), pair_blocks.data_ptr()
    b.eval_partials, b.eval_blocks, b.pair_error = eval_partials.data_ptr(), eval_blocks.data_ptr(), pair_error.data_ptr()
    b.used, b.chunks = U, chunks
    _native.call("camd_bundle_emit", dev, ctypes.byref(b), what=what)
    _lm.iterate(state, dev, what, lambda: _native.call("camd_bundle_step", dev, ctypes.byref(b), what=what))
    _native.call("camd_bundle_finish", dev, ctypes.byref(b), what=what)
    s = state.cpu().numpy()
    _lm.check_status(what, s[_native.BUNDLE_STATUS], s[_native.BUNDLE_EVALUATIONS], s[_native.BUNDLE_PIVOT])
    final = s[_native.BUNDLE_POSES:_native.BUNDLE_POSES + 12 * N].reshape(N, 12)
    T_out = T_from_poses(final[:, :9].reshape(N, 3, 3), final[:, 9:])
    T_out[fixed_view] = T[fixed_view]
    out = dict(T=T_out, retval=float(np.sqrt(s[_native.BUNDLE_COST] / (2.0 * U))), cost0=float(s[_native.BUNDLE_COST0]),
               cost=float(s[_native.BUNDLE_COST]), iterations=int(s[_native.BUNDLE_ITERATIONS]),
               evaluations=int(s[_native.BUNDLE_EVALUATIONS]), anchor=(anchor, axis))
    out["status"], out["pair_error"] = to_caller((status, pair_error), was_np)
    out["points"] = to_caller(points, was_np) if return_points else None
    if return_start:
        out["start"] = to_caller(start, was_np)
    if return_rows:
        out["rows_a"], out["rows_b"] = to_caller((rows_a, rows_b), was_np)
        out["used_counts"] = used_counts
    return out
