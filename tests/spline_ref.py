"""NumPy restatement of csrc/spline.hip, stage by stage: the same operations in the same order (every product and sum
rounded on its own, the same elimination order, the same summation order), with ``np.log`` where the device has its own
``log`` -- the one place the two may differ.  And the same spline in mpmath (``exact_image``), the exact reference of the
end-to-end test.  Contract: include/calibrating_amd.h, "sparse samples filled by their thin-plate spline"."""
import numpy as np

NO_SAMPLE, SINGULAR, NON_FINITE = 1, 2, 4


def phi(dx, dy):
    """r == 0 ? 0 : (r * r) * log(r) with r = sqrt(dx * dx + dy * dy)"""
    r = np.sqrt(dx * dx + dy * dy)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (r * r) * np.log(r)
    return np.where(r == 0.0, 0.0, v)


def assemble(uv, smooth):
    """A = Phi - smooth I: the lower triangle computed, the upper its mirror, the diagonal 0 - smooth"""
    uv = np.asarray(uv, np.float64)
    u, v = uv[:, 0], uv[:, 1]
    low = np.tril(phi(u[:, None] - u[None, :], v[:, None] - v[None, :]), -1)
    A = low + low.T
    A[np.diag_indices(len(u))] = 0.0 - float(smooth)
    return A


def lu_solve(A, z, pivots=None):
    """(w, status) of A w = z: partial pivoting by the largest |a|, of equal ones the lowest row (a non-finite entry counts as
    +inf and ends it); elimination row by row, the right-hand side carried along; back-substitution by columns, falling k.
    ``pivots``: a list that receives every step's pivot row."""
    A, b = np.array(A, np.float64), np.array(z, np.float64)
    n = len(b)
    if n == 0:
        return b, NO_SAMPLE
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return np.full(n, np.nan), NON_FINITE
    with np.errstate(all="ignore"):
        for k in range(n):
            col = np.abs(A[k:, k])
            col[~np.isfinite(col)] = np.inf
            p = k + int(np.argmax(col))  # (the first of equal ones)
            if not col[p - k] > 0.0 or col[p - k] == np.inf:
                return np.full(n, np.nan), SINGULAR
            if pivots is not None:
                pivots.append(p)
            if p != k:
                A[[k, p], k:] = A[[p, k], k:]
                b[[k, p]] = b[[p, k]]
            m = A[k + 1:, k] / A[k, k]
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - m[:, None] * A[k, k + 1:][None, :]
            b[k + 1:] = b[k + 1:] - m * b[k]
        for k in range(n - 1, -1, -1):
            b[k] = b[k] / A[k, k]
            b[:k] = b[:k] - A[:k, k] * b[k]
    return b, 0


def evaluate(uv, w, hw, grid_step=1, mask=None):
    """(image, scale): image[y][x] = sum_i w_i phi(x s - u_i, y s - v_i) added in row order from 0.0, and
    scale[y][x] = sum_i |w_i phi_i|, what a relative error of the phis is multiplied by.  Outside the mask: 0."""
    uv, w = np.asarray(uv, np.float64), np.asarray(w, np.float64)
    ys, xs = np.mgrid[0:hw[0], 0:hw[1]]
    x, y = (xs * grid_step).astype(np.float64), (ys * grid_step).astype(np.float64)
    s, scale = np.zeros(hw), np.zeros(hw)
    with np.errstate(all="ignore"):
        for i in range(len(w)):
            t = w[i] * phi(x - uv[i, 0], y - uv[i, 1])
            s = s + t
            scale = scale + np.abs(t)
    if mask is not None:
        s, scale = np.where(mask != 0, s, 0.0), np.where(mask != 0, scale, 0.0)
    return s, scale


def image(uvz, hw, smooth=0.5, mask=None):
    """the three stages after one another: (image, weights, status)"""
    uvz = np.asarray(uvz, np.float64).reshape(-1, 3)
    w, status = lu_solve(assemble(uvz[:, :2], smooth), uvz[:, 2])
    return evaluate(uvz[:, :2], w, hw, 1, mask)[0], w, status


def ulps(a, b):
    """the largest distance of two float64 arrays in units in the last place (along the ordered bit patterns)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
    if not a.size:
        return 0.0
    ka, kb = key(a), key(b)
    far = ka.astype(np.float64) - kb.astype(np.float64)  # (the int64 difference wraps beyond 2^63: only then the rounded one)
    return float(np.abs(np.where(np.abs(far) < 2.0 ** 62, (ka - kb).astype(np.float64), far)).max())


def exchanging_system(n, seed=0):
    """(A, z) whose elimination exchanges rows at EVERY step k < n - 1: an upper triangle with a heavy diagonal under a small
    dense matrix, its rows rotated down by one"""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.uniform(-1.0, 1.0, (n, n)), 1) + np.diag(rng.uniform(4.0, 5.0, n)) + rng.uniform(-1e-3, 1e-3, (n, n))
    return np.roll(U, 1, axis=0), rng.uniform(-1.0, 1.0, n)


def samples(seed, n, hw, z=None):
    """n (u, v, z) rows at distinct fractional places of an (h, w) frame (quarter pixels: every difference is exact)"""
    rng = np.random.default_rng(seed)
    cells = rng.permutation((4 * hw[0]) * (4 * hw[1]))[:n]
    u, v = (cells % (4 * hw[1])) / 4.0, (cells // (4 * hw[1])) / 4.0
    zz = rng.uniform(1.0, 5.0, n) if z is None else z(u, v)
    return np.stack([u, v, zz], 1)


# ---- the exact reference ---------------------------------------------------------------------------------------------
DIGITS = 60
# the end-to-end fixtures: (seed, rows) of samples(seed, rows, EXACT_HW).  tests/test_spline_cpu.py checks that the restatement's
# own error on them stays below 1e-6 of max|z|
EXACT_CASES = ((21, 12), (22, 40))
EXACT_HW = (16, 16)


def exact_image(uvz, hw, smooth=0.5):
    """the spline of the float64 rows, solved and evaluated in mpmath at DIGITS digits, rounded to float64 at the end"""
    from mpmath import matrix, mp, mpf, log, lu_solve as mp_lu_solve
    old = mp.dps
    mp.dps = DIGITS
    try:
        rows = [[mpf(float(c)) for c in r] for r in np.asarray(uvz, np.float64)]
        n = len(rows)

        def f(dx, dy):
            r2 = dx * dx + dy * dy
            return mpf(0) if r2 == 0 else r2 * log(r2) / 2
        A = matrix(n, n)
        for i in range(n):
            for j in range(n):
                A[i, j] = -mpf(float(smooth)) if i == j else f(rows[i][0] - rows[j][0], rows[i][1] - rows[j][1])
        w = mp_lu_solve(A, matrix([r[2] for r in rows]))
        out = np.empty(hw)
        for y in range(hw[0]):
            for x in range(hw[1]):
                out[y, x] = float(sum((w[i] * f(mpf(x) - rows[i][0], mpf(y) - rows[i][1]) for i in range(n)), mpf(0)))
        return out
    finally:
        mp.dps = old
