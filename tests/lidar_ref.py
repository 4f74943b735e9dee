"""NumPy restatement of the LiDAR path (test infrastructure; csrc/lidar.hip and calibrating_amd/lidar.py are compared with it
bit for bit).  Built on tests/hull_ref.py (the mask contract) and tests/sparse_ref.py (the nearest fill).

The operation order of the projection, float64, every product and sum rounded on its own (NumPy's elementwise operators
do exactly that):
    X' = ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3]         r = 0, 1, 2; without T: X' = X
    p_r = (K[r,0] X' + K[r,1] Y') + K[r,2] Z'
    u = p0 / p2,  v = p1 / p2;  kept iff p2 > 0, u >= 0, v >= 0, u < w, v < h
    row = (u * rate, v * rate, Z')
The example's own lines (``xyzs @ cam.K.T`` after ``apply_T_to_point_cloud``) are BLAS products whose order and fusing are the
library's; on inputs whose arithmetic is exact the two agree bit for bit (tests/test_lidar_cpu.py asserts it)."""
import numpy as np

import hull_ref
import sparse_ref

MAX_HULL_POINTS = 4096
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


# ---- a. cloud -> rows ------------------------------------------------------------------------------------------------
def cloud_to_uvzs(xyzs, K, wh, T=None, rate=1.0):
    """(rows (k, 3) float64 in input order, the number of points with p2 > 0)"""
    P = np.asarray(xyzs).astype(np.float64)
    K = np.asarray(K, np.float64)
    w, h = wh
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        if T is not None:
            T = np.asarray(T, np.float64)
            x, y, z = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)]
        p = [(K[r, 0] * x + K[r, 1] * y) + K[r, 2] * z for r in range(3)]
        u, v = p[0] / p[2], p[1] / p[2]
        positive = p[2] > 0
        keep = positive & (u >= 0) & (v >= 0) & (u < w) & (v < h)
        rows = np.stack([u * np.float64(rate), v * np.float64(rate), z], 1)[keep]
    return rows, int(positive.sum())


def example_uvzs(xyzs, K, wh, T=None, rate=1.0):
    """The example's plain NumPy lines (calibrate_lidar2cam_pnp.py:14-24, 32, with utils.apply_T_to_point_cloud:152-161)."""
    xyzs = np.asarray(xyzs)
    if T is not None:
        xyzs = (np.asarray(T) @ np.concatenate([xyzs, np.ones_like(xyzs[:, :1])], 1).T).T[:, :3]
    w, h = wh
    xyzs_ = xyzs @ np.asarray(K).T
    z_is_positive = xyzs_[:, 2] > 0
    xyzs_ = xyzs_[z_is_positive]
    xyzs = xyzs[z_is_positive]
    uvs = xyzs_[:, :2] / xyzs_[:, 2:3]
    idx = (uvs.min(-1) >= 0) & (uvs[:, 0] < w) & (uvs[:, 1] < h)
    uvzs = np.concatenate((uvs[idx], xyzs[idx, 2:3]), -1)
    return uvzs * [[rate, rate, 1]], len(xyzs)


def auto_rate(n_positive, h, w):
    return (n_positive / h / w) ** 0.5 if n_positive > 5000 else 0.25


# ---- b. the hull of any number of samples -----------------------------------------------------------------------------
def row_range(uvs):
    """(lowest, highest pixel row, status) of the samples that have a pixel; (INT_MAX, INT_MIN, status) when none has."""
    ys = [y for _, y in hull_ref.pixels(np.asarray(uvs, np.float64)[:, :2])]
    return (min(ys), max(ys), _status(uvs)) if ys else (INT_MAX, INT_MIN, _status(uvs))


def _status(uvs):
    uvs = np.asarray(uvs, np.float64)[:, :2]
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(uvs).all(1)
        return 4 if (fin & (np.abs(np.round(uvs)) > hull_ref.LIMIT).any(1)).any() else 0


def row_extremes(uvs, y0, rows):
    """(table (rows, 2) int32: (xmin, xmax) of the samples on pixel row y0 + r, (INT_MAX, INT_MIN) where none; status)"""
    table = np.empty((rows, 2), np.int32)
    table[:, 0], table[:, 1] = INT_MAX, INT_MIN
    for x, y in hull_ref.pixels(np.asarray(uvs, np.float64)[:, :2]):
        if 0 <= y - y0 < rows:
            table[y - y0, 0] = min(table[y - y0, 0], x)
            table[y - y0, 1] = max(table[y - y0, 1], x)
    return table, _status(uvs)


def candidates(table, y0):
    """[(xmin, y), (xmax, y)] of the non-empty rows, rising y, min before max"""
    out = []
    for r, (lo, hi) in enumerate(table):
        if lo <= hi:
            out += [(int(lo), y0 + r), (int(hi), y0 + r)]
    return out


def hull_in_rounds(points, capacity=MAX_HULL_POINTS):
    """(vertices in the kernel's order, rounds): more than ``capacity`` candidates go as consecutive chunks of ``capacity``,
    each chunk's hull is taken, the vertices are concatenated in chunk order, and the step repeats until one chunk holds
    them.  The order: counter-clockwise (x right, y up) from the lowest (x, y) -- what the monotone chain of hull_ref.hull
    returns and what the kernel's gift wrapping walks."""
    points, rounds = list(points), 1
    while len(points) > capacity:
        nxt = []
        for s in range(0, len(points), capacity):
            nxt += hull_ref.hull(points[s:s + capacity])
        if len(nxt) >= len(points):
            raise ValueError("a round over %d candidates left %d: more than MAX_HULL_POINTS vertices" % (len(points), len(nxt)))
        points, rounds = nxt, rounds + 1
    return hull_ref.hull(points), rounds


def cloud_hull(uvs, rows_range=None):
    """(vertices, rounds, table, status) through the per-row extremes"""
    if rows_range is None:
        lo, hi, _ = row_range(uvs)
        rows_range = (lo, hi - lo + 1) if lo <= hi else (0, 1)
    table, status = row_extremes(uvs, *rows_range)
    cand = candidates(table, rows_range[0])
    vertices, rounds = hull_in_rounds(cand)
    return vertices, rounds, table, status | (0 if cand else 1)


def cloud_hull_mask(uvs, hw):
    return hull_ref.mask_of_hull(cloud_hull(uvs)[0], hw)


# ---- c. the nearest sample inside the hull ----------------------------------------------------------------------------
def nearest_in_hull(uvzs, hw, distance=2, rows_range=None):
    """(float32 (h, w), vertices, status): sparse_ref's nearest fill where the hull's mask is 1, +0.0 elsewhere"""
    uvzs = np.asarray(uvzs)
    vertices, _, _, status = cloud_hull(uvzs[:, :2], rows_range)
    mask = hull_ref.mask_of_hull(vertices, hw)
    if len(uvzs) == 0:
        return np.zeros(hw, np.float32), vertices, status
    near = sparse_ref.nearest_windowed(uvzs, hw, distance)
    return np.where(mask != 0, near, np.float32(0)), vertices, status


# ---- the whole function -------------------------------------------------------------------------------------------------
def xyzs_to_dense_depth(xyzs, K, wh, T=None, rate=0.5, sparse=False, distance=2, resize=None):
    """(depth, info) as calibrating_amd.lidar.xyzs_to_dense_depth; ``resize(img, (h, w))``: the float32 bilinear resize the
    caller trusts (the oracle's)."""
    xyzs = np.asarray(xyzs)
    w, h = wh
    rows, n_positive = cloud_to_uvzs(xyzs, K, wh, T, 1.0)
    if rate is None:
        rate = auto_rate(n_positive, h, w)
    rows, _ = cloud_to_uvzs(xyzs, K, wh, T, rate)
    grid = (int(round(h * rate)), int(round(w * rate)))
    out_dtype = (xyzs.dtype if xyzs.dtype in (np.float32, np.float64) else np.float64) if sparse else np.float32
    info = dict(rows=len(rows), grid_hw=grid, rate=rate, hull_counts=0, status=0 if len(rows) else 1)
    if len(rows) == 0:
        return np.zeros((h, w), out_dtype), info
    if sparse:
        depth = sparse_ref.scatter(rows[:, :2], rows[:, 2].astype(out_dtype), grid)
    else:
        depth, vertices, status = nearest_in_hull(rows, grid, distance, (0, grid[0] + 1))
        info.update(hull_counts=len(vertices), status=status)
    if grid != (h, w):
        depth = resize(depth, (h, w))
    return depth, info


def uvs_on_depth_to_xyzs(uvs_depth, depth, K):
    """calibrate_lidar2cam_pnp.py:119-121, point by point as the example writes them"""
    out = []
    for uv in np.asarray(uvs_depth):
        z = depth[uv[1], uv[0]]
        uvz = np.pad(uv, (0, 1), constant_values=1) * np.float64(z)
        out.append(([uvz] @ np.linalg.inv(K).T)[0])
    return np.float64(out)
