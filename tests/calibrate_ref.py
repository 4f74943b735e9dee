"""NumPy float64 restatement of the calibration of ``csrc/calibrate.hip`` / ``calibrating_amd/calibrate.py``.  Test
infrastructure only.

The same start (a Hartley-normalised homography per frame, cv2's ``initIntrinsicParams2D`` for K0, no lens, start poses
from ``pnp_ref`` under K0), the same Schur-complement Levenberg-Marquardt with the same damping, acceptance (a lower cost, or one
within 64 ulp of the current), stopping and masking as the kernels; NumPy's order of the sums over points and frames, which is what tests/golden/calibrate_tolerance.json
measures.
"""
import numpy as np

import pnp_ref
import points_ref
from distort_depth_ref import _coefficients

EPS = 2.0 ** -52
MAX_EVALUATIONS = 100
SINGULAR_PIVOT = 1e-10
COST_RESOLUTION = 64 * EPS  # a candidate's cost within the rounding of the sums of the current one is no worse
USE_INTRINSIC_GUESS, FIX_PRINCIPAL_POINT, ZERO_TANGENT_DIST, FIX_FOCAL_LENGTH, FIX_K1, FIX_K2, FIX_K3 = 1, 4, 8, 16, 32, 64, 128


def free_mask(flags):
    m = np.ones(9, bool)
    if flags & FIX_FOCAL_LENGTH:
        m[0:2] = False
    if flags & FIX_PRINCIPAL_POINT:
        m[2:4] = False
    if flags & ZERO_TANGENT_DIST:
        m[6:8] = False
    m[4] &= not flags & FIX_K1
    m[5] &= not flags & FIX_K2
    m[8] &= not flags & FIX_K3
    return m


def homography(obj, uv, plane, null="eigh"):
    """plane coordinates (the object points turned by ``plane``, x and y) -> raw pixels, as the kernel forms it"""
    return pnp_ref.normalised_dlt((obj @ plane.T)[:, :2], uv, null)


def initial_camera_matrix(Hs, xy):
    """cv2's initIntrinsicParams2D: the principal point at the centre, 1 / f^2 from the vanishing points by least squares"""
    cx, cy = (xy[0] - 1) * 0.5, (xy[1] - 1) * 0.5
    A, b = [], []
    for G in Hs:
        G = np.array(G)
        G[0] -= G[2] * cx
        G[1] -= G[2] * cy
        h, v = G[:, 0], G[:, 1]
        d1, d2 = (h + v) * 0.5, (h - v) * 0.5
        h, v, d1, d2 = (a / np.sqrt((a * a).sum()) for a in (h, v, d1, d2))
        A += [[h[0] * v[0], h[1] * v[1]], [d1[0] * d2[0], d1[1] * d2[1]]]
        b += [-h[2] * v[2], -d1[2] * d2[2]]
    A, b = np.array(A), np.array(b)
    f = np.linalg.solve(A.T @ A, A.T @ b)
    return np.array([[np.sqrt(abs(1 / f[0])), 0, cx], [0, np.sqrt(abs(1 / f[1])), cy], [0, 0, 1]])


def camera_of(k):
    return np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]]), np.array(k[4:9])


def frame_terms(R, t, obj, uv, k):
    """residuals (2n,), pose Jacobian (2n, 6), intrinsic Jacobian (2n, 9) of one frame at R, t and k = fx fy cx cy k1 k2 p1 p2 k3"""
    K, D = camera_of(k)
    r, Jp, x, y, _ = pnp_ref.pose_jacobian(R, t, obj, uv, K, D)
    with np.errstate(all="ignore"):
        k1, k2, p1, p2, k3 = _coefficients(D)[:5]
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        a1, a2, a3 = 2 * x * y, r2 + 2 * x * x, r2 + 2 * y * y
        cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6
        xd, yd = x * cdist + p1 * a1 + p2 * a2, y * cdist + p1 * a3 + p2 * a1
        o, l = np.zeros_like(x), np.ones_like(x)
        fx, fy = k[0], k[1]
        Ju = np.stack([xd, o, l, o, fx * (x * r2), fx * (x * r4), fx * a1, fx * a2, fx * (x * r6)], 1)
        Jv = np.stack([o, yd, o, l, fy * (y * r2), fy * (y * r4), fy * a3, fy * a1, fy * (y * r6)], 1)
        Jk = np.stack([Ju, Jv], 1).reshape(-1, 9)
    return r.reshape(-1), Jp, Jk


def blocks(r, Jp, Jk):
    """(A, B, C, gp, gk, c): the sums over one frame's residuals and Jacobians"""
    outer = lambda a, b: (a[:, :, None] * b[:, None, :]).sum(0)  # noqa: E731
    return (outer(Jp, Jp), outer(Jp, Jk), outer(Jk, Jk), (Jp * r[:, None]).sum(0), (Jk * r[:, None]).sum(0), (r * r).sum())


def linearise(poses, objs, uvs, k):
    """per frame (A, B, C, gp, gk, c)"""
    return [blocks(*frame_terms(R, t, obj, uv, k)) for (R, t), obj, uv in zip(poses, objs, uvs)]


def cost_of(poses, objs, uvs, k):
    K, D = camera_of(k)
    return [((points_ref.project_points(obj, R, t, K, D) - uv) ** 2).sum() for (R, t), obj, uv in zip(poses, objs, uvs)]


def _chol(M):
    return pnp_ref._cholesky(M)


def _solve(L, b):
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def reduced(lin, lam, free):
    """(S, g, the per-frame factors) of the block for lambda, masked; None where a frame's damped matrix is not definite"""
    S, g, dC, Ls = np.zeros((9, 9)), np.zeros(9), np.zeros(9), []
    for A, B, C, gp, gk, c in lin:
        L = _chol(A + lam * np.diag(np.diag(A)))
        if L is None:
            return None
        Ls.append(L)
        S = S + (C - B.T @ _solve(L, B))
        g = g + (gk - B.T @ _solve(L, gp))
        dC = dC + np.diag(C)
    return S, g, dC, Ls


def mask_system(S, g, free):
    S, g = S.copy(), g.copy()
    fixed = ~free
    S[fixed, :] = 0
    S[:, fixed] = 0
    S[fixed, fixed] = 1
    g[fixed] = 0
    return S, g


def shared_step(lin, lam, free):
    """(dk, the per-frame factors) of one evaluation at lambda, as ``joint`` solves it; None where nothing can be solved"""
    red = reduced(lin, lam, free)
    if red is None:
        return None
    S, g, dC, Ls = red
    S, g = mask_system(S + lam * np.diag(dC), g, free)
    L = _chol(S)
    if L is None:
        return None
    dk = _solve(L, -g)
    return (dk, Ls) if np.isfinite(dk).all() else None


def candidates(lin, Ls, poses, objs, uvs, k, dk):
    """One evaluation's intermediate values after the block's step, as ``joint`` forms them -> dict(k2, poses2, cost2,
    step2, norm2: per frame, cost, accept)."""
    poses2, step2, norm2 = [], [], []
    for (A, B, C, gp, gk, c), Lf, (R, t) in zip(lin, Ls, poses):
        d = _solve(Lf, -(gp + B @ dk))
        poses2.append((pnp_ref.rotate_left(d[:3], R), t + d[3:]))
        step2.append((d * d).sum())
        norm2.append(3.0 + (t * t).sum())
    k2 = k + dk
    cost2 = cost_of(poses2, objs, uvs, k2)
    c2, c = sum(cost2), sum(l[5] for l in lin)
    return dict(k2=k2, poses2=poses2, cost2=cost2, step2=step2, norm2=norm2, cost=c,
                accept=bool(c2 < c or c2 - c <= COST_RESOLUTION * c))


def final_stage(lin, free):
    """(the smallest pivot of the undamped reduced matrix scaled to a unit diagonal, NaN where it does not factor; the cost),
    as ``joint`` ends"""
    S = reduced(lin, 0.0, free)[0]
    with np.errstate(all="ignore"):
        s = 1.0 / np.sqrt(np.diag(S))
        L = _chol(mask_system(S * s[:, None] * s[None, :], np.zeros(9), free)[0])
    return (np.nan if L is None else float((np.diag(L) ** 2).min())), sum(l[5] for l in lin)


def joint(objs, uvs, k0, poses0, flags):
    """The Levenberg-Marquardt over the block and the poses from k0 and the start poses [(R, t)] ->
    dict(k, poses, cost, iterations, evaluations, status, min_pivot)."""
    free = free_mask(flags)
    k, poses = np.array(k0, np.float64), [(np.array(R), np.array(t)) for R, t in poses0]
    lin = linearise(poses, objs, uvs, k)
    lam, evals, its, stopped = 1e-3, 0, 0, False
    while evals < MAX_EVALUATIONS and not stopped:
        evals += 1
        better = small = False
        red = reduced(lin, lam, free)
        dk = None
        if red is not None:
            S, g, dC, Ls = red
            S, g = mask_system(S + lam * np.diag(dC), g, free)
            L = _chol(S)
            if L is not None:
                dk = _solve(L, -g)
                if not np.isfinite(dk).all():
                    dk = None
        if dk is not None:
            poses2, step, norm = [], 0.0, 0.0
            for (A, B, C, gp, gk, c), Lf, (R, t) in zip(lin, Ls, poses):
                d = _solve(Lf, -(gp + B @ dk))
                poses2.append((pnp_ref.rotate_left(d[:3], R), t + d[3:]))
                step += (d * d).sum()
                norm += 3.0 + (t * t).sum()
            k2 = k + dk
            c2 = sum(cost_of(poses2, objs, uvs, k2))
            c = sum(l[5] for l in lin)
            small = np.sqrt(step + (dk * dk).sum()) < EPS * (np.sqrt(norm + (k * k).sum()) + EPS)
            better = bool(c2 < c or c2 - c <= COST_RESOLUTION * c)
            if better:
                k, poses, its = k2, poses2, its + 1
                lin = linearise(poses, objs, uvs, k)
        lam = lam * 0.1 if better else lam * 10.0
        stopped = bool(small or lam < 1e-12 or lam > 1e12)
    cost = sum(l[5] for l in lin)
    status, pivot = 3, np.nan
    red = reduced(lin, 0.0, free)
    if red is not None:
        S = red[0]
        with np.errstate(all="ignore"):
            s = 1.0 / np.sqrt(np.diag(S))
            S, _ = mask_system(S * s[:, None] * s[None, :], np.zeros(9), free)
            L = _chol(S)
        if L is not None:
            pivot = float((np.diag(L) ** 2).min())
            if pivot >= SINGULAR_PIVOT and np.isfinite(cost) and stopped:
                status = 0
    return dict(k=k, poses=poses, cost=cost, frame_cost=[l[5] for l in lin], iterations=its, evaluations=evals, status=status,
                min_pivot=pivot)


def start(objs, uvs, xy, flags=0, K=None, D=None):
    """(k0, frame status words, start poses of the frames whose status is 0, planar) -- the steps of calibrate_camera"""
    k0 = np.zeros(9)
    planar, plane = pnp_ref.plane_of(np.concatenate([o for o in objs if np.isfinite(o).all()]))
    ok = [len(o) >= 4 and bool(np.isfinite(o).all() and np.isfinite(u).all()) for o, u in zip(objs, uvs)]
    if flags & USE_INTRINSIC_GUESS:
        k0[:4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        if D is not None:
            k0[4:4 + np.size(D)] = np.ravel(D)
    else:
        assert planar
        K0 = initial_camera_matrix([homography(o, u, plane) for o, u, good in zip(objs, uvs, ok) if good], xy)
        k0[:4] = K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2]
    if flags & ZERO_TANGENT_DIST:
        k0[6:8] = 0
    K0, D0 = camera_of(k0)
    status, poses = [], []
    for o, u in zip(objs, uvs):
        minimum = 4 if planar else 6
        if len(o) < 4:
            status.append(1)
            continue
        if not (np.isfinite(o).all() and np.isfinite(u).all()):
            status.append(2)
            continue
        r = pnp_ref.refine(o, u, K0, D0, pnp_ref.init_pose(o, u, K0, D0, planar, plane), min_points=minimum) \
            if len(o) >= minimum else dict(status=1)
        status.append(0 if r["status"] == 0 else (1 if r["status"] == 1 else 3))
        if r["status"] == 0:
            poses.append((r["T"][:3, :3], r["T"][:3, 3]))
    return k0, np.array(status), poses, planar


def calibrate(objs, uvs, xy, flags=0, K=None, D=None):
    """what ``calibrate_camera`` returns, with ``K0`` of the start besides; T and reprojection_error are NaN for a frame
    that is not part of the joint problem"""
    objs, uvs = [np.asarray(o, np.float64) for o in objs], [np.asarray(u, np.float64) for u in uvs]
    k0, status, poses0, _ = start(objs, uvs, xy, flags, K, D)
    used = np.flatnonzero(status == 0)
    r = joint([objs[i] for i in used], [uvs[i] for i in used], k0, poses0, flags)
    T = np.full((len(objs), 4, 4), np.nan)
    T[:, 3] = [0, 0, 0, 1]
    err = np.full(len(objs), np.nan)
    for at, (R, t), c in zip(used, r["poses"], r["frame_cost"]):
        T[at, :3, :3], T[at, :3, 3] = R, t
        err[at] = np.sqrt(c / len(objs[at]))
    Kr, Dr = camera_of(r["k"])
    n = sum(len(objs[i]) for i in used)
    return dict(retval=float(np.sqrt(r["cost"] / n)), K=Kr, D=Dr.reshape(1, 5), T=T, reprojection_error=err, iterations=r["iterations"],
                status=status, evaluations=r["evaluations"], camera_status=r["status"], K0=camera_of(k0)[0], min_pivot=r["min_pivot"])
