"""A LiDAR cloud and a camera: the workflow of the reference's
``example/calibrate_lidar2cam_by_PnP/calibrate_lidar2cam_pnp.py`` in this package's names.

``xyzs_to_dense_depth`` turns a cloud into a dense depth image of the camera (csrc/lidar.hip: projection, filter and scale in
one pass; the nearest sample inside the samples' convex hull; then the float32 bilinear ``resize``); a user annotates pixel
pairs between the photo and that picture; ``uvs_on_depth_to_xyzs`` lifts the annotated depth pixels back to points and
``calibrate_lidar2cam`` solves the LiDAR's pose from them by PnP; ``xyzs_to_dense_depth(..., T=pose, rate=1, sparse=True)``
projects the cloud again to check the alignment.  INTEGRATION.md section L has the filter, the ``rate=None`` rule and what is
refused.  NumPy in -> NumPy out, CUDA in -> CUDA out.
"""
import numpy as np

from . import _native, sparse as _sparse
from ._arrays import FLOAT_TYPES, K9, check_array, dtype_name, is_np, mat, positive_wh, to_caller, to_device
from ._native import call
from .resize import resize

__all__ = ["xyzs_to_dense_depth", "uvs_on_depth_to_xyzs", "calibrate_lidar2cam"]


def _auto_rate(n_positive, h, w):
    """The example's rule (:25-29), on the number of points in front of the camera."""
    return (n_positive / h / w) ** 0.5 if n_positive > 5000 else 0.25


def _grid_hw(h, w, rate):
    grid = (int(round(h * rate)), int(round(w * rate)))
    if grid[0] <= 0 or grid[1] <= 0:
        raise ValueError("rate %r leaves an empty grid %s of the %d x %d image" % (rate, grid, w, h))
    return grid


def _cloud_on_device(xyzs):
    """(tensor, elements between two points): float32 / float64 rows read in place where their columns are adjacent (a column
    view of a wider CUDA array), else a contiguous copy; other dtypes as float64."""
    name = dtype_name(xyzs)
    if is_np(xyzs) or name not in FLOAT_TYPES:
        t = to_device(xyzs, dtype=name if name in FLOAT_TYPES else "float64", cast=True)
        return t, 3
    if int(xyzs.shape[0]) > 1 and (xyzs.stride(1) != 1 or xyzs.stride(0) < 3):
        xyzs = xyzs.contiguous()
    if int(xyzs.shape[0]) <= 1:
        return xyzs.contiguous(), 3
    return xyzs, int(xyzs.stride(0))


def xyzs_to_dense_depth(xyzs, cam, T=None, rate=0.5, sparse=False, distance=2, return_info=False):
    """The depth image of camera ``cam`` that the cloud ``xyzs`` (n, 3) gives (calibrate_lidar2cam_pnp.py:13-42).

    In float64: ``X' = R X + t`` of the 4x4 ``T`` (None: the cloud is in the camera's frame), ``p = K X'`` with all of
    ``cam.K`` (``cam.D`` is ignored, as in the example), ``u, v = p0 / p2, p1 / p2``; a point stays iff ``p2 > 0``,
    ``min(u, v) >= 0``, ``u < w`` and ``v < h``.  The rows ``(rate u, rate v, X'_z)`` go to the grid ``[int(round(h * rate)),
    int(round(w * rate))]``: ``sparse=False`` fills every pixel inside the rows' convex hull with the nearest row's z
    (``sparse.interpolate_uvzs_in_hull(inter_type="nearest", distance=distance)``), ``sparse=True`` scatters them
    (``uvzs_to_arr2d``, in the cloud's dtype); the grid is then upsized to ``(h, w)`` by the float32 bilinear ``resize``.
    ``rate=None``: ``(n_pos / h / w) ** 0.5`` if ``n_pos > 5000`` else 0.25, ``n_pos`` the points with ``p2 > 0`` (one
    read-back).  A float64 cloud with ``sparse=True`` and a grid other than ``(h, w)`` raises ``NotImplementedError``: there is
    no float64 resize.  An empty cloud, or one that loses every point, gives zeros.
    ``return_info`` adds ``dict(rows, grid_hw, rate, hull_counts, status)``: the rows kept, the hull's vertices and the status
    bits of ``interpolate_uvzs_in_hull`` (1: no row)."""
    import torch
    check_array(xyzs, "xyzs")
    if len(xyzs.shape) != 2 or xyzs.shape[1] != 3:
        raise ValueError("xyzs must be (n, 3), got %s" % (tuple(xyzs.shape),))
    n = int(xyzs.shape[0])
    if n >= 2 ** 31:
        raise ValueError("%d points do not fit the 32-bit point index" % n)
    w, h = positive_wh(cam.xy, "cam.xy")
    K = K9(cam.K)
    T16 = None
    if T is not None:
        T16 = np.asarray(T, np.float64)
        if T16.shape != (4, 4):
            raise ValueError("T must be 4x4, got %s" % (T16.shape,))
        T16 = mat(T16, 16)
    if rate is not None:
        rate = float(rate)
        if not (rate > 0 and np.isfinite(rate)):
            raise ValueError("rate must be a positive number or None, got %r" % (rate,))
    distance = _sparse._check_nearest_distance(distance)
    was_np = is_np(xyzs)
    out_name = dtype_name(xyzs) if (sparse and dtype_name(xyzs) in FLOAT_TYPES) else ("float64" if sparse else "float32")

    def refuse_f64_resize(grid):
        if sparse and out_name == "float64" and grid != (h, w):
            raise NotImplementedError("sparse=True of a float64 cloud on a %s grid needs a float64 resize to %s, which this "
                                      "package does not have: pass rate=1 or a float32 cloud" % (grid, (h, w)))

    def zeros(grid, rate_used):
        refuse_f64_resize(grid)
        z = np.zeros((h, w), out_name) if was_np else torch.zeros((h, w), dtype=getattr(torch, out_name), device=xyzs.device)
        if not return_info:
            return z
        return z, dict(rows=0, grid_hw=grid, rate=rate_used, hull_counts=0, status=_sparse.STATUS_NO_SAMPLE)

    if rate is not None:
        grid = _grid_hw(h, w, rate)
        refuse_f64_resize(grid)
    if n == 0:
        rate = _auto_rate(0, h, w) if rate is None else rate
        return zeros(_grid_hw(h, w, rate), rate)

    # 1. the rows (csrc/lidar.hip a): count, [choose the rate,] emit
    pts, stride = _cloud_on_device(xyzs)
    dev, who = pts.device, "xyzs_to_dense_depth"
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.empty(max(8, _native.lib().camd_cloud_workspace_bytes(n)), dtype=torch.uint8, device=dev)

    def stage(stages, rows, capacity):
        call("camd_cloud_to_uvzs", dev, pts.data_ptr(), FLOAT_TYPES[dtype_name(pts)], n, stride, None if T16 is None else T16.ctypes.data,
             K.ctypes.data, w, h, 1.0 if rate is None else rate, stages, None if rows is None else rows.data_ptr(), capacity,
             counters.data_ptr(), ws.data_ptr(), what=who)

    if rate is None:
        stage(1, None, 0)
        kept, n_positive = (int(x) for x in counters.cpu().numpy())
        rate = _auto_rate(n_positive, h, w)
        grid = _grid_hw(h, w, rate)
        refuse_f64_resize(grid)
        rows = torch.empty((max(kept, 1), 3), dtype=torch.float64, device=dev)
        if kept:
            stage(2, rows, kept)
    else:
        rows = torch.empty((n, 3), dtype=torch.float64, device=dev)
        stage(3, rows, n)
        kept = int(counters[0].item())
    if kept == 0:
        return zeros(grid, rate)
    rows = rows[:kept]

    # 2. the grid: the nearest row inside the rows' hull (b, c), or the scatter
    if sparse:
        values = rows[:, 2].to(getattr(torch, out_name)).contiguous()
        depth = _sparse.uvzs_to_arr2d(rows[:, :2], grid, values=values)
        hull_counts, status = 0, 0
    else:
        # rate v < rate h, and rounding is monotonic: the rows' pixel rows are 0 .. grid[0]
        depth, rec = _sparse._nearest_in_hull(rows, kept, grid, distance, "float64", rows_range=(0, grid[0] + 1), what=who)
        hull_counts, status = rec["hull_counts"], rec["status"]
    # 3. to the camera's size
    if grid != (h, w):
        depth = resize(depth, (h, w))
    depth = to_caller(depth, was_np)
    if not return_info:
        return depth
    if not sparse:
        hull_counts, status = (int(x[0]) for x in to_caller((hull_counts, status), True))
    return depth, dict(rows=kept, grid_hw=grid, rate=rate, hull_counts=hull_counts, status=status)


def uvs_on_depth_to_xyzs(uvs_depth, depth, K):
    """The points under annotated pixels of a depth image (calibrate_lidar2cam_pnp.py:119-121), on the host in float64:
    ``z = depth[v, u]`` and ``xyz = [u, v, 1] * z @ inv(K).T``.  ``uvs_depth``: (n, 2) integer pixels."""
    uvs = np.asarray(uvs_depth)
    if uvs.ndim != 2 or uvs.shape[1] != 2:
        raise ValueError("uvs_depth must be (n, 2), got %s" % (uvs.shape,))
    idx = uvs.astype(np.int64)
    if not np.array_equal(idx, uvs):
        raise ValueError("uvs_depth must hold whole pixels")
    d = depth if is_np(depth) else depth.detach().cpu().numpy()
    if d.ndim != 2:
        raise ValueError("depth must be (h, w), got %s" % (d.shape,))
    if len(idx) and (idx.min() < 0 or idx[:, 0].max() >= d.shape[1] or idx[:, 1].max() >= d.shape[0]):
        raise ValueError("uvs_depth leaves the %d x %d depth image" % (d.shape[1], d.shape[0]))
    z = d[idx[:, 1], idx[:, 0]].astype(np.float64)
    uvz = np.concatenate([idx.astype(np.float64), np.ones((len(idx), 1))], 1) * z[:, None]
    return uvz @ np.linalg.inv(np.asarray(K, np.float64)[:3, :3]).T


def calibrate_lidar2cam(cam, uvs_img, xyzs):
    """The LiDAR's pose from annotated pairs (calibrate_lidar2cam_pnp.py:132-138): ``uvs_img`` (n, 2) pixels of the photo,
    ``xyzs`` (n, 3) the points of the cloud they show (``uvs_on_depth_to_xyzs``) -> ``dict(T, reprojection_error, status)``
    from ``cam.perspective_n_point`` (K and D of the photo's camera); ``T`` (4, 4) is the cloud's frame in the camera's.  Too
    few points (6 for points with depth, 4 on a plane) raise that function's ``ValueError``."""
    res = cam.perspective_n_point(np.asarray(uvs_img, np.float64), np.asarray(xyzs, np.float64))
    return dict(T=res["T"], reprojection_error=res["reprojection_error"], status=0)
