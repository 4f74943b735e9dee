"""NumPy / Python-integer restatement of the hull fill's mask contract (test infrastructure; csrc/hull.hip is compared
with it bit for bit).  Written differently from the kernel on purpose: the hull by the monotone chain on Python integers
(the kernel wraps a gift), the mask by testing every pixel against every hull edge in int64 (the kernel derives row
spans by floor and ceil division), the plane by tests/sparse_ref.py.

The contract: a row (u, v[, z]) is valid when u, v are finite, z is finite and not 0 and
|round(u)|, |round(v)| <= 2**20; its pixel is (int32(round(u)), int32(round(v))), half to even; pixel (x, y) is inside iff
the integer point (x, y) lies in the closed convex hull of the valid rows' pixels."""
import numpy as np

import sparse_ref

LIMIT = 2 ** 20


def valid_rows(rows, hw=None, keep_last_per_pixel=False):
    """Indices of the rows that take part, rising.  ``keep_last_per_pixel``: rows whose pixel is outside ``hw`` are
    dropped and of several rows on one pixel only the highest index stays."""
    rows = np.asarray(rows, np.float64)
    keep = []
    for i, r in enumerate(rows):
        if not (np.isfinite(r[0]) and np.isfinite(r[1])):
            continue
        if rows.shape[1] >= 3 and not (np.isfinite(r[2]) and r[2] != 0):
            continue
        x, y = float(np.round(r[0])), float(np.round(r[1]))
        if abs(x) > LIMIT or abs(y) > LIMIT:
            continue
        if keep_last_per_pixel and not (0 <= x < hw[1] and 0 <= y < hw[0]):
            continue
        keep.append(i)
    if keep_last_per_pixel:
        last = {}
        for i in keep:
            last[(float(np.round(rows[i, 0])), float(np.round(rows[i, 1])))] = i
        keep = sorted(last.values())
    return np.array(keep, np.int64)


def pixels(rows, hw=None, keep_last_per_pixel=False):
    """[(x, y)] Python integers of the rows that take part"""
    rows = np.asarray(rows, np.float64)
    idx = valid_rows(rows, hw, keep_last_per_pixel)
    return [(int(np.int32(np.round(rows[i, 0]))), int(np.int32(np.round(rows[i, 1])))) for i in idx]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(points):
    """The vertices of the convex hull of integer points by the monotone chain: strict turns only, so collinear points
    on an edge and duplicates are no vertices.  One point -> itself, collinear points -> the two ends."""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) <= 2:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def mask_of_hull(vertices, hw):
    """uint8 (h, w): every pixel against every edge of the counter-clockwise (in x right, y up) hull in int64 -- inside
    iff no edge has it strictly on its right; a segment: on the line and within its box; a point: itself."""
    h, w = hw
    out = np.zeros((h, w), np.uint8)
    if not vertices:
        return out
    ys, xs = np.mgrid[:h, :w].astype(np.int64)
    v = [(np.int64(x), np.int64(y)) for x, y in vertices]
    if len(v) == 1:
        inside = (xs == v[0][0]) & (ys == v[0][1])
    elif len(v) == 2:
        (ax, ay), (bx, by) = v
        inside = ((bx - ax) * (ys - ay) - (by - ay) * (xs - ax) == 0)
        inside &= (xs >= min(ax, bx)) & (xs <= max(ax, bx)) & (ys >= min(ay, by)) & (ys <= max(ay, by))
    else:
        inside = np.ones((h, w), bool)
        for k in range(len(v)):
            (ax, ay), (bx, by) = v[k], v[(k + 1) % len(v)]
            inside &= (bx - ax) * (ys - ay) - (by - ay) * (xs - ax) >= 0
    out[inside] = 1
    return out


def mask(rows, hw, keep_last_per_pixel=False):
    return mask_of_hull(hull(pixels(rows, hw, keep_last_per_pixel)), hw)


def fill(uvzs, hw, keep_last_per_pixel=False):
    """(float32 (h, w) image, mask): sparse_ref.plane of the rows that take part (np.linalg.lstsq, minimum norm where the
    plane is not unique) inside the mask, 0 outside"""
    uvzs = np.asarray(uvzs, np.float64)
    m = mask(uvzs, hw, keep_last_per_pixel)
    idx = valid_rows(uvzs, hw, keep_last_per_pixel)
    if not len(idx):
        return np.zeros(hw, np.float32), m
    return np.where(m != 0, sparse_ref.plane(uvzs[idx], hw), np.float32(0)), m
