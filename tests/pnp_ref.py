"""NumPy float64 restatement of the batched PnP of ``csrc/pnp.hip``, one frame at a time.  Test infrastructure only.

The same parametrisation (``R <- exp([w]x) R``, ``t <- t + d``), the same damping rule (Marquardt: ``lambda diag(J^T J)``,
1e-3 at the start, / 10 after a step that lowers the cost, * 10 otherwise) and the same stopping rule (step below
``eps (|p| + eps)`` with ``|p|^2 = 3 + |t|^2``, lambda outside [1e-12, 1e12], 100 evaluations) as the kernel; the projection is
``points_ref.project_points``.  Only the order of the sums over the points differs (NumPy's pairwise sum here, lane
strides and a butterfly there), which is what tests/golden/pnp_tolerance.json measures.  The start pose (``init_pose``)
follows the kernel's steps with ``numpy.linalg.eigh`` for the null vector.
"""
import numpy as np

import points_ref
from distort_depth_ref import _coefficients

EPS = 2.0 ** -52
MAX_ITERATIONS = 100
SINGULAR_PIVOT = 1e-10
OK, FEW, NONFINITE, SINGULAR = 0, 1, 2, 3


def distort_jacobian(D, x, y):
    """d(xd, yd) / d(x, y) of cv2.projectPoints' polynomial: (n, 2, 2)."""
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coefficients(D)
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6
    icdist2 = 1.0 / (1 + k4 * r2 + k5 * r4 + k6 * r6)
    q = cdist * icdist2
    dq = ((k1 + 2 * k2 * r2 + 3 * k3 * r4) - q * (k4 + 2 * k5 * r2 + 3 * k6 * r4)) * icdist2
    gx, gy = 2 * x * dq, 2 * y * dq
    j = np.empty((len(x), 2, 2))
    j[:, 0, 0] = q + x * gx + 2 * p1 * y + 6 * p2 * x + 2 * s1 * x + 4 * s2 * r2 * x
    j[:, 0, 1] = x * gy + 2 * p1 * x + 2 * p2 * y + 2 * s1 * y + 4 * s2 * r2 * y
    j[:, 1, 0] = y * gx + 2 * p1 * x + 2 * p2 * y + 2 * s3 * x + 4 * s4 * r2 * x
    j[:, 1, 1] = q + y * gy + 6 * p1 * y + 2 * p2 * x + 2 * s3 * y + 4 * s4 * r2 * y
    return j


def residuals(R, t, obj, uv, K, D):
    return points_ref.project_points(obj, R, t, K, D) - uv


def pose_jacobian(R, t, obj, uv, K, D):
    """(r (n, 2) residuals, J (2n, 6) their Jacobian in R <- exp([w]x) R, t <- t + d, and x, y, iz of the projection) at
    the pose R, t.  (``uv`` is among the arguments because the residual needs it.)"""
    K = np.asarray(K, np.float64)
    P = obj @ R.T
    Xc = P + t
    with np.errstate(all="ignore"):
        iz = np.where(Xc[:, 2] != 0, 1.0 / Xc[:, 2], 1.0)
        x, y = Xc[:, 0] * iz, Xc[:, 1] * iz
        r = residuals(R, t, obj, uv, K, D)
        d = distort_jacobian(D, x, y) * np.array([K[0, 0], K[1, 1]])[None, :, None]
        g = np.stack([d[:, :, 0] * iz[:, None], d[:, :, 1] * iz[:, None],
                      -(d[:, :, 0] * x[:, None] + d[:, :, 1] * y[:, None]) * iz[:, None]], 2)  # (n, 2, 3): d pixel / d camera point
        J = np.concatenate([np.cross(P[:, None, :], g), g], 2).reshape(-1, 6)
    return r, J, x, y, iz


def normal_equations(R, t, obj, uv, K, D):
    """(J^T J (6, 6), J^T r (6,), r^T r) at the pose R, t."""
    r, J = pose_jacobian(R, t, obj, uv, K, D)[:2]
    with np.errstate(all="ignore"):
        rr = r.reshape(-1)
        A = (J[:, :, None] * J[:, None, :]).sum(0)
        return A, (J * rr[:, None]).sum(0), (rr * rr).sum()


def rotate_left(w, R):
    th = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    h = 0.5 * th
    A = np.sin(th) / th if th > 0 else 1.0
    sh = np.sin(h) / h if h > 0 else 1.0
    B = 0.5 * sh * sh
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return (np.eye(3) + A * Kx + B * (Kx @ Kx)) @ R


def _cholesky(M):
    with np.errstate(all="ignore"):
        try:
            L = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            return None
    return L if np.isfinite(L).all() else None


def refine(obj, uv, K, D, T0, min_points=4):
    """dict(T, reprojection_error, iterations, status) of one frame from the start pose T0 (4, 4)."""
    obj, uv = np.asarray(obj, np.float64), np.asarray(uv, np.float64)
    nan = dict(T=np.full((4, 4), np.nan), reprojection_error=np.nan, iterations=0)
    if len(obj) < min_points:
        return dict(nan, status=FEW)
    if not (np.isfinite(obj).all() and np.isfinite(uv).all()):
        return dict(nan, status=NONFINITE)
    if not np.isfinite(T0).all():
        return dict(nan, status=SINGULAR)
    R, t = np.array(T0[:3, :3], np.float64), np.array(T0[:3, 3], np.float64)
    A, g, c = normal_equations(R, t, obj, uv, K, D)
    lam, it, stopped = 1e-3, 0, False
    while it < MAX_ITERATIONS and not stopped:
        it += 1
        better = small = False
        L = _cholesky(A + lam * np.diag(np.diag(A)))
        if L is not None:
            d = np.linalg.solve(L.T, np.linalg.solve(L, -g))
            R2, t2 = rotate_left(d[:3], R), t + d[3:]
            A2, g2, c2 = normal_equations(R2, t2, obj, uv, K, D)
            small = np.sqrt((d * d).sum()) < EPS * (np.sqrt(3.0 + (t * t).sum()) + EPS)
            better = bool(c2 < c)
            if better:
                R, t, A, g, c = R2, t2, A2, g2, c2
        lam = lam * 0.1 if better else lam * 10.0
        stopped = bool(small or lam < 1e-12 or lam > 1e12)
    with np.errstate(all="ignore"):
        s = 1.0 / np.sqrt(np.diag(A))
        L = _cholesky(A * s[:, None] * s[None, :])
    if L is None or (np.diag(L) ** 2).min() < SINGULAR_PIVOT or not np.isfinite(c) or not stopped:
        return dict(nan, iterations=it, status=SINGULAR)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return dict(T=T, reprojection_error=float(np.sqrt(c / (2.0 * len(obj)))), iterations=it, status=OK, min_pivot=float((np.diag(L) ** 2).min()))


def plane_of(obj):
    X = np.asarray(obj, np.float64).reshape(-1, 3)
    if np.ptp(X[:, 2]) == 0:
        return True, np.eye(3)
    _, s, Vt = np.linalg.svd(X - X.mean(0), full_matrices=False)
    if np.linalg.det(Vt) < 0:
        Vt = Vt * np.array([[1.0], [1.0], [-1.0]])
    return bool(s[2] < 1e-3 * s[1]), Vt


def null_vector_by_inverse_iteration(M):
    """The kernel's way to the null vector of a normal matrix: six rounds of inverse iteration on M + 1e-13 tr(M) I from
    the start 1, 1.25, 1.5, ... through one Cholesky factor."""
    n = len(M)
    L = np.linalg.cholesky(M + 1e-13 * np.trace(M) * np.eye(n))
    v = 1.0 + 0.25 * np.arange(n)
    for _ in range(6):
        v = np.linalg.solve(L.T, np.linalg.solve(L, v))
        v = v / np.sqrt((v * v).sum())
    return v


def normalised_dlt(X, xy, null="eigh"):
    """G (3, d + 1) with xy ~ G [X 1] from (n, d) object and (n, 2) image coordinates: the direct linear transform on
    Hartley-normalised points, as the kernel forms it; ``null``: the null vector from ``numpy.linalg.eigh`` or, "kernel",
    from the kernel's inverse iteration."""
    Dn = X.shape[1]
    m, mi = X.mean(0), xy.mean(0)
    so = np.sqrt(Dn) / np.sqrt(((X - m) ** 2).sum(1)).mean()
    si = np.sqrt(2.0) / np.sqrt(((xy - mi) ** 2).sum(1)).mean()
    h = np.concatenate([(X - m) * so, np.ones((len(X), 1))], 1)
    x, y = ((xy - mi) * si).T
    z = np.zeros_like(h)
    rows = np.concatenate([np.concatenate([h, z, -x[:, None] * h], 1), np.concatenate([z, h, -y[:, None] * h], 1)])
    M = rows.T @ rows
    v = np.linalg.eigh(M)[1][:, 0] if null == "eigh" else null_vector_by_inverse_iteration(M)
    Gn = v.reshape(3, Dn + 1)
    To = np.eye(Dn + 1)
    To[:Dn, :Dn] *= so
    To[:Dn, Dn] = -so * m
    Ti_inv = np.array([[1 / si, 0, mi[0]], [0, 1 / si, mi[1]], [0, 0, 1]])
    return Ti_inv @ Gn @ To


def init_pose(obj, uv, K, D, planar, plane, null="eigh"):
    """The start pose from ``normalised_dlt`` of the object points (a plane's: turned by ``plane``, x and y) and the
    undistorted image points, as the kernel forms it."""
    obj, uv = np.asarray(obj, np.float64), np.asarray(uv, np.float64)
    xy = points_ref.undistort_trace(uv, K, D, iters=10)[0]
    X = obj @ plane.T if planar else obj
    m = X.mean(0)
    G = normalised_dlt(X[:, :2 if planar else 3], xy, null)
    unit = lambda a: a / np.linalg.norm(a)  # noqa: E731
    T = np.eye(4)
    if planar:
        s = 2.0 / (np.linalg.norm(G[:, 0]) + np.linalg.norm(G[:, 1]))
        if G[2, 0] * m[0] + G[2, 1] * m[1] + G[2, 2] < 0:
            s = -s
        c1 = unit(G[:, 0] * s)
        c2 = G[:, 1] * s
        c2 = unit(c2 - (c1 @ c2) * c1)
        c3 = np.cross(c1, c2)
        T[:3, :3] = np.stack([c1, c2, c3], 1) @ plane
        T[:3, 3] = s * G[:, 2] - c3 * m[2]
    else:
        s = 1.0 / np.linalg.norm(G[2, :3])
        if G[2, :3] @ m + G[2, 3] < 0:
            s = -s
        r3 = unit(G[2, :3] * s)
        r1 = G[0, :3] * s
        r1 = unit(r1 - (r1 @ r3) * r3)
        T[:3, :3] = np.stack([r1, np.cross(r3, r1), r3])
        T[:3, 3] = s * G[:, 3]
    return T


def solve(obj, uv, K, D, T0=None):
    """One frame: the start pose (unless given), then the refinement."""
    planar, plane = plane_of(obj)
    if T0 is None:
        if len(obj) < (4 if planar else 6):
            return refine(obj, uv, K, D, np.eye(4), min_points=4 if planar else 6)
        T0 = init_pose(obj, uv, K, D, planar, plane)
        return refine(obj, uv, K, D, T0, min_points=4 if planar else 6)
    return refine(obj, uv, K, D, np.asarray(T0, np.float64), min_points=4)
