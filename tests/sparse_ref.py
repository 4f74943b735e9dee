"""NumPy restatements of the sparse <-> dense family (test infrastructure; what the GPU kernels are compared with on
every pixel).  Written from the semantics -- rounding, drop rule, last write wins, float64 distance, lowest index on a
tie -- not from the reference's text; tests/test_sparse_cpu.py holds them against the reference's own output
(tests/golden/reference_sparse.npz) bit for bit."""
from fractions import Fraction

import numpy as np


# ---- scatter ---------------------------------------------------------------------------------------------------------
def scatter(uvs, values, hw=None, bg_value=0, arr2d=None):
    """Row by row, later rows overwrite earlier ones."""
    values = values[:, None] if values.ndim == 1 else values
    c = values.shape[1]
    if arr2d is None:
        if hw is None:
            hw = (int(np.int32(np.round(uvs[:, 0].max()))) + 1, int(np.int32(np.round(uvs[:, 1].max()))) + 1)
        arr2d = np.ones(tuple(hw) + ((c,) if c >= 2 else ()), values.dtype) * bg_value
    h, w = arr2d.shape[:2]
    xs, ys = np.int32(np.round(uvs[:, 0])), np.int32(np.round(uvs[:, 1]))
    for i in range(len(uvs)):
        if 0 <= xs[i] < w and 0 <= ys[i] < h:
            arr2d[ys[i], xs[i]] = values[i] if c >= 2 else values[i, 0]
    return arr2d


def rows_of(arr2d, mask=None):
    """(x, y, value): all pixels x-outer / y-inner, or the masked ones row-major; dtype = int64 promoted with arr2d's."""
    h, w = arr2d.shape
    dt = np.result_type(np.int64, arr2d.dtype)
    if mask is None:
        out = np.empty((w * h, 3), dt)
        for x in range(w):
            out[x * h:(x + 1) * h, 0], out[x * h:(x + 1) * h, 1], out[x * h:(x + 1) * h, 2] = x, np.arange(h), arr2d[:, x]
        return out
    ys, xs = np.nonzero(mask != 0)  # row-major
    out = np.empty((len(ys), 3), dt)
    out[:, 0], out[:, 1], out[:, 2] = xs, ys, arr2d[ys, xs]
    return out


# ---- nearest ---------------------------------------------------------------------------------------------------------
def nearest_brute(uvzs, hw, distance=2, stats=None):
    """Every pixel against every sample: float64 sqrt(dx*dx + dy*dy), argmin (first = lowest index), ``< distance``,
    float32 of the chosen z.  ``stats``: a dict that receives the two margins the bit-for-bit tests rest on."""
    h, w = hw
    u, v, z = (np.asarray(uvzs[:, k], np.float64) for k in range(3))
    out = np.zeros((h, w), np.float32)
    gap, edge = np.inf, np.inf
    xs = np.arange(w, dtype=np.float64)
    for y in range(h):
        dx, dy = xs[:, None] - u[None, :], float(y) - v[None, :]
        d = np.sqrt(dx * dx + dy * dy)
        i = np.argmin(d, 1)
        best = d[np.arange(w), i]
        hit = best < distance
        out[y, hit] = np.float32(uvzs[i[hit], 2])
        if stats is not None:
            ds = np.sort(np.where(d < distance, d, np.inf), 1)
            with np.errstate(invalid="ignore"):
                g = np.diff(ds, axis=1)  # (inf - inf between two samples beyond distance)
            g = g[np.isfinite(g)]
            gap = min(gap, g.min() if g.size else np.inf)
            edge = min(edge, np.abs(best - distance).min())
    if stats is not None:
        stats.update(min_gap=float(gap), min_edge=float(edge))
    return out


def nearest_windowed(uvzs, hw, distance=2, stats=None):
    """The same answer through a bounded window: a sample (u, v) can only be nearer than ``distance`` <= R to the pixels
    floor(u) - R + 1 .. floor(u) + R (and likewise in y), so every sample proposes itself to those (2R)^2 pixels and each
    pixel keeps the proposal with the smallest (distance, index).  Memory ~ (2R)^2 * n: fit for 1080p x 200 000."""
    h, w = hw
    R = max(1, int(np.ceil(distance)))
    u, v = np.asarray(uvzs[:, 0], np.float64), np.asarray(uvzs[:, 1], np.float64)
    fu, fv = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    idx = np.arange(len(u), dtype=np.int64)
    pix, dist, who = [], [], []
    for oy in range(-R + 1, R + 1):
        for ox in range(-R + 1, R + 1):
            x, y = fu + ox, fv + oy
            ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            dx, dy = x[ok].astype(np.float64) - u[ok], y[ok].astype(np.float64) - v[ok]
            pix.append(y[ok] * w + x[ok])
            dist.append(np.sqrt(dx * dx + dy * dy))
            who.append(idx[ok])
    pix, dist, who = np.concatenate(pix), np.concatenate(dist), np.concatenate(who)
    order = np.lexsort((who, dist, pix))
    pix, dist, who = pix[order], dist[order], who[order]
    first = np.r_[True, pix[1:] != pix[:-1]] if len(pix) else np.zeros(0, bool)
    out = np.zeros(h * w, np.float32)
    hit = first & (dist < distance)
    out[pix[hit]] = np.float32(uvzs[who[hit], 2])
    if stats is not None:
        same = (pix[1:] == pix[:-1]) & (dist[1:] < distance)  # consecutive neighbours of one pixel, both within distance
        g = (dist[1:] - dist[:-1])[same]
        stats.update(min_gap=float(g.min()) if g.size else np.inf,
                     min_edge=float(np.abs(dist[first] - distance).min()) if first.any() else np.inf)
    return out.reshape(h, w)


def resize_nearest_scaled(img, hw):
    """The plugin's upsizing: ``img * hw[1] / img.shape[1]`` in float32, then cv2.resize(INTER_NEAREST) to ``hw``."""
    sh, sw = img.shape
    img = img * hw[1] / sw
    xs = np.minimum(np.floor(np.arange(hw[1]) * (1.0 / (hw[1] / sw))).astype(np.int64), sw - 1)
    ys = np.minimum(np.floor(np.arange(hw[0]) * (1.0 / (hw[0] / sh))).astype(np.int64), sh - 1)
    return img[ys[:, None], xs[None, :]]


# ---- plane -----------------------------------------------------------------------------------------------------------
def plane(uvzs, hw):
    """np.linalg.lstsq plane, evaluated as a float32 (x, y, 1) grid times the float64 coefficients."""
    A = np.array(uvzs, np.float64)
    A[:, 2] = 1
    abc = np.linalg.lstsq(A, uvzs[:, 2], rcond=None)[0]
    h, w = hw
    grid = np.ones((w * h, 3), np.float32)
    grid[:, 0], grid[:, 1] = np.repeat(np.arange(w), h), np.tile(np.arange(h), w)
    grid[:, 2] = grid @ abc
    out = np.zeros((h, w), np.float32)
    out[np.int32(grid[:, 1]), np.int32(grid[:, 0])] = grid[:, 2]
    return out


def _solve(M, r):
    """Exact solution of a small square system in Fractions (Gauss-Jordan)."""
    n = len(r)
    M = [list(row) + [r[i]] for i, row in enumerate(M)]
    for c in range(n):
        p = next(i for i in range(c, n) if M[i][c] != 0)
        M[c], M[p] = M[p], M[c]
        M[c] = [x / M[c][c] for x in M[c]]
        for i in range(n):
            if i != c and M[i][c] != 0:
                M[i] = [x - M[i][c] * y for x, y in zip(M[i], M[c])]
    return [M[i][n] for i in range(n)]


def plane_exact(uvzs):
    """(a, b, c) of the least-squares plane as Fractions: the normal equations of the float64 samples, solved exactly."""
    rows = [[Fraction(float(u)), Fraction(float(v)), Fraction(1)] for u, v, _ in uvzs]
    zs = [Fraction(float(z)) for z in uvzs[:, 2]]
    M = [[sum(r[i] * r[j] for r in rows) for j in range(3)] for i in range(3)]
    return _solve(M, [sum(r[i] * z for r, z in zip(rows, zs)) for i in range(3)])


def plane_ulps(img, abc):
    """max over the pixels of |img - exact| in float32 ulps of the exact value."""
    a, b, c = abc
    worst = Fraction(0)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            exact = a * x + b * y + c
            ulp = Fraction(float(np.spacing(np.float32(abs(float(exact))))))
            worst = max(worst, abs(Fraction(float(img[y, x])) - exact) / ulp)
    return float(worst)


# ---- triangulation ---------------------------------------------------------------------------------------------------
def triangulate_exact(uvs1, uvs2, K1, K2, T):
    """(zs1, zs2) as Fractions: X = K^-1 (u, v, 1) with the exact inverse, the 3x2 least squares by its exact normal
    equations."""
    F = lambda a: [[Fraction(float(x)) for x in row] for row in np.asarray(a, np.float64)]  # noqa: E731
    Kf1, Kf2, Tf = F(K1), F(K2), F(T)
    e = [Fraction(1), Fraction(0), Fraction(0)], [Fraction(0), Fraction(1), Fraction(0)], [Fraction(0), Fraction(0), Fraction(1)]
    zs1, zs2 = [], []
    for (u1, v1), (u2, v2) in zip(uvs1, uvs2):
        x1 = _solve([r[:3] for r in Kf1[:3]], [Fraction(float(u1)), Fraction(float(v1)), Fraction(1)])
        x2 = _solve([r[:3] for r in Kf2[:3]], [Fraction(float(u2)), Fraction(float(v2)), Fraction(1)])
        a = [-sum(Tf[i][j] * x1[j] for j in range(3)) for i in range(3)]
        t = [Tf[i][3] for i in range(3)]
        dot = lambda p, q: sum(pi * qi for pi, qi in zip(p, q))  # noqa: E731
        z1, z2 = _solve([[dot(a, a), dot(a, x2)], [dot(a, x2), dot(x2, x2)]], [dot(a, t), dot(x2, t)])
        zs1.append(z1)
        zs2.append(z2)
    del e
    return zs1, zs2


def relerr(got, exact):
    return float(max(abs(Fraction(float(g)) - x) / abs(x) for g, x in zip(got, exact)))
