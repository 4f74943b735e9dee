"""NumPy float64 restatement of the stereo calibration of ``csrc/stereo_calibrate.hip`` /
``calibrating_amd/stereo_calibrate.py``.  Test infrastructure only.

The same start (``pnp_ref`` in each camera, per frame ``T2 inv(T1)`` as a Rodrigues vector and a translation, the
component-wise median), the same Schur-complement Levenberg-Marquardt with the same damping, acceptance (a lower cost,
or one within 64 ulp of the current), stopping, status words and ``retval`` as the kernels; NumPy's order of the sums
over points and frames, which is what tests/golden/stereo_calibrate_tolerance.json measures.

The Jacobian blocks of camera 2 are checked against central differences with the step ``FD_STEP`` = 1e-5.  The residual
is a pixel, fx ~ 1000 times a ratio of coordinates that a unit of rotation or of (translation / depth) moves by O(1);
depths are 0.3 m and more, so its third derivatives stay below about 6 fx / 0.3^3 ~ 2e5 px per unit^3 and the truncation
h^2 / 6 |f'''| below 4e-6; the rounding 2^-52 |f| / h is 3e-8.  ``FD_BOUND`` = 1e-5 px per unit, on entries of 1e2 .. 1e4.
"""
import numpy as np

import pnp_ref
import points_ref

EPS = 2.0 ** -52
MAX_EVALUATIONS = 100
SINGULAR_PIVOT = 1e-10
COST_RESOLUTION = 64 * EPS
FD_STEP, FD_BOUND = 1e-5, 1e-5
FIX_INTRINSIC, USE_EXTRINSIC_GUESS = 0x100, 0x400000


def frame_terms(Ri, ti, R, t, obj, uv1, uv2, cams):
    """(r1 (2n,), J1 (2n, 6), r2 (2n,), Jf (2n, 6), Jr (2n, 6)) of one frame: camera 1's residuals and their Jacobian in the
    frame's pose; camera 2's residuals, their Jacobian in the frame's pose and in the rig"""
    K1, D1, K2, D2 = cams
    r1, J1 = pnp_ref.pose_jacobian(Ri, ti, obj, uv1, K1, D1)[:2]
    rt = R @ ti
    r2, J2 = pnp_ref.pose_jacobian(R @ Ri, rt + t, obj, uv2, K2, D2)[:2]
    Jw, Jd = J2[:, :3], J2[:, 3:]
    Jf = np.concatenate([Jw @ R, Jd @ R], 1)
    Jr = np.concatenate([Jw + np.cross(rt, Jd), Jd], 1)
    return r1.reshape(-1), J1, r2.reshape(-1), Jf, Jr


def residuals(Ri, ti, R, t, obj, uv1, uv2, cams):
    K1, D1, K2, D2 = cams
    return np.concatenate([(points_ref.project_points(obj, Ri, ti, K1, D1) - uv1).reshape(-1),
                           (points_ref.project_points(obj, R @ Ri, R @ ti + t, K2, D2) - uv2).reshape(-1)])


def finite_difference_blocks(Ri, ti, R, t, obj, uv1, uv2, cams, h=FD_STEP):
    """(d r / d frame (4n, 6), d r / d rig (4n, 6)) by central differences in the local perturbations"""
    def moved(x):
        return residuals(pnp_ref.rotate_left(x[:3], Ri), ti + x[3:6], pnp_ref.rotate_left(x[6:9], R), t + x[9:], obj, uv1, uv2, cams)
    cols = []
    for q in range(12):
        e = np.zeros(12)
        e[q] = h
        cols.append((moved(e) - moved(-e)) / (2 * h))
    J = np.stack(cols, 1)
    return J[:, :6], J[:, 6:]


def blocks(r1, J1, r2, Jf, Jr):
    """(A, B, C, gp, gr, c): the sums over one frame's residuals and Jacobians"""
    outer = lambda a, b: (a[:, :, None] * b[:, None, :]).sum(0)  # noqa: E731
    return (outer(J1, J1) + outer(Jf, Jf), outer(Jf, Jr), outer(Jr, Jr), (J1 * r1[:, None]).sum(0) + (Jf * r2[:, None]).sum(0),
            (Jr * r2[:, None]).sum(0), (r1 * r1).sum() + (r2 * r2).sum())


def linearise(poses, R, t, objs, uv1s, uv2s, cams):
    """per frame (A, B, C, gp, gr, c)"""
    return [blocks(*frame_terms(Ri, ti, R, t, obj, u1, u2, cams)) for (Ri, ti), obj, u1, u2 in zip(poses, objs, uv1s, uv2s)]


def _solve(L, b):
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def reduced(lin, lam):
    """(S, g, diag sum C, the per-frame factors); None where a frame's damped matrix is not definite"""
    S, g, dC, Ls = np.zeros((6, 6)), np.zeros(6), np.zeros(6), []
    for A, B, C, gp, gr, c in lin:
        L = pnp_ref._cholesky(A + lam * np.diag(np.diag(A)))
        if L is None:
            return None
        Ls.append(L)
        S = S + (C - B.T @ _solve(L, B))
        g = g + (gr - B.T @ _solve(L, gp))
        dC = dC + np.diag(C)
    return S, g, dC, Ls


def shared_step(lin, lam):
    """(the rig's step, the per-frame factors) of one evaluation at lambda, as ``joint`` solves it; None where nothing can
    be solved"""
    red = reduced(lin, lam)
    if red is None:
        return None
    S, g, dC, Ls = red
    L = pnp_ref._cholesky(S + lam * np.diag(dC))
    if L is None:
        return None
    dr = _solve(L, -g)
    return (dr, Ls) if np.isfinite(dr).all() else None


def candidates(lin, Ls, poses, R, t, objs, uv1s, uv2s, cams, dr):
    """One evaluation's intermediate values after the rig's step, as ``joint`` forms them -> dict(R2, t2, poses2, cost2,
    step2, norm2: per frame, cost, accept)."""
    R2, t2 = pnp_ref.rotate_left(dr[:3], R), t + dr[3:]
    poses2, step2, norm2, cost2 = [], [], [], []
    for (A, B, C, gp, gr, c), Lf, (Ri, ti), obj, u1, u2 in zip(lin, Ls, poses, objs, uv1s, uv2s):
        d = _solve(Lf, -(gp + B @ dr))
        poses2.append((pnp_ref.rotate_left(d[:3], Ri), ti + d[3:]))
        step2.append((d * d).sum())
        norm2.append(3.0 + (ti * ti).sum())
        rr = residuals(poses2[-1][0], poses2[-1][1], R2, t2, obj, u1, u2, cams)
        cost2.append((rr * rr).sum())
    c2, c = sum(cost2), sum(l[5] for l in lin)
    return dict(R2=R2, t2=t2, poses2=poses2, cost2=cost2, step2=step2, norm2=norm2, cost=c,
                accept=bool(c2 < c or c2 - c <= COST_RESOLUTION * c))


def final_stage(lin):
    """(the smallest pivot of the undamped reduced matrix scaled to a unit diagonal, NaN where it does not factor; the cost),
    as ``joint`` ends"""
    S = reduced(lin, 0.0)[0]
    with np.errstate(all="ignore"):
        s = 1.0 / np.sqrt(np.diag(S))
        L = pnp_ref._cholesky(S * s[:, None] * s[None, :])
    return (np.nan if L is None else float((np.diag(L) ** 2).min())), sum(l[5] for l in lin)


def joint(objs, uv1s, uv2s, cams, poses0, R0, t0):
    """The Levenberg-Marquardt over the rig and the frames' poses -> dict(R, t, poses, cost, frame_cost, iterations,
    evaluations, status, min_pivot)."""
    R, t = np.array(R0, np.float64), np.array(t0, np.float64).reshape(3)
    poses = [(np.array(a), np.array(b)) for a, b in poses0]
    lin = linearise(poses, R, t, objs, uv1s, uv2s, cams)
    lam, evals, its, stopped = 1e-3, 0, 0, False
    while evals < MAX_EVALUATIONS and not stopped:
        evals += 1
        better = small = False
        red = reduced(lin, lam)
        dr = None
        if red is not None:
            S, g, dC, Ls = red
            L = pnp_ref._cholesky(S + lam * np.diag(dC))
            if L is not None:
                dr = _solve(L, -g)
                if not np.isfinite(dr).all():
                    dr = None
        if dr is not None:
            R2, t2 = pnp_ref.rotate_left(dr[:3], R), t + dr[3:]
            poses2, step, norm, c2 = [], 0.0, 0.0, 0.0
            for (A, B, C, gp, gr, c), Lf, (Ri, ti), obj, u1, u2 in zip(lin, Ls, poses, objs, uv1s, uv2s):
                d = _solve(Lf, -(gp + B @ dr))
                poses2.append((pnp_ref.rotate_left(d[:3], Ri), ti + d[3:]))
                step += (d * d).sum()
                norm += 3.0 + (ti * ti).sum()
                rr = residuals(poses2[-1][0], poses2[-1][1], R2, t2, obj, u1, u2, cams)
                c2 += (rr * rr).sum()
            c = sum(l[5] for l in lin)
            small = np.sqrt(step + (dr * dr).sum()) < EPS * (np.sqrt(norm + 3.0 + (t * t).sum()) + EPS)
            better = bool(c2 < c or c2 - c <= COST_RESOLUTION * c)
            if better:
                R, t, poses, its = R2, t2, poses2, its + 1
                lin = linearise(poses, R, t, objs, uv1s, uv2s, cams)
        lam = lam * 0.1 if better else lam * 10.0
        stopped = bool(small or lam < 1e-12 or lam > 1e12)
    cost = sum(l[5] for l in lin)
    status, pivot = 3, np.nan
    red = reduced(lin, 0.0)
    if red is not None:
        with np.errstate(all="ignore"):
            s = 1.0 / np.sqrt(np.diag(red[0]))
            L = pnp_ref._cholesky(red[0] * s[:, None] * s[None, :])
        if L is not None:
            pivot = float((np.diag(L) ** 2).min())
            if pivot >= SINGULAR_PIVOT and np.isfinite(cost) and stopped:
                status = 0
    return dict(R=R, t=t, poses=poses, cost=cost, frame_cost=[l[5] for l in lin], iterations=its, evaluations=evals, status=status,
                min_pivot=pivot)


def rig_start(T1s, T2s):
    """the component-wise median of the Rodrigues vectors and translations of T2 inv(T1)"""
    from calibrating_amd import geometry
    rs, ts = [], []
    for A, B in zip(T1s, T2s):
        R = B[:3, :3] @ A[:3, :3].T
        rs.append(geometry.rodrigues(R).reshape(3))
        ts.append(B[:3, 3] - R @ A[:3, 3])
    return geometry.rodrigues(np.median(np.array(rs), axis=0)), np.median(np.array(ts), axis=0)


def start(objs, uv1s, uv2s, cams):
    """(frame status words, the start poses of the frames whose status is 0 in camera 1 and in camera 2)"""
    K1, D1, K2, D2 = cams
    finite = [o for o in objs if np.isfinite(o).all()]
    planar, plane = pnp_ref.plane_of(np.concatenate(finite))
    minimum = 4 if planar else 6
    status, T1s, T2s = [], [], []
    for o, u1, u2 in zip(objs, uv1s, uv2s):
        if len(o) < minimum:
            status.append(1)
            continue
        if not (np.isfinite(o).all() and np.isfinite(u1).all() and np.isfinite(u2).all()):
            status.append(2)
            continue
        a = pnp_ref.refine(o, u1, K1, D1, pnp_ref.init_pose(o, u1, K1, D1, planar, plane), min_points=minimum)
        b = pnp_ref.refine(o, u2, K2, D2, pnp_ref.init_pose(o, u2, K2, D2, planar, plane), min_points=minimum)
        ok = a["status"] == 0 and b["status"] == 0
        status.append(0 if ok else 3)
        if ok:
            T1s.append(a["T"]), T2s.append(b["T"])
    return np.array(status), T1s, T2s


def stereo_calibrate(objs, uv1s, uv2s, K1, D1, K2, D2, R0=None, t0=None):
    """what ``stereo_calibrate`` returns, with the rig's status (``rig_status``), the smallest pivot and the start (``R0``,
    ``t0``) besides; T and reprojection_error are NaN for a frame that is not part of the joint problem"""
    objs = [np.asarray(o, np.float64) for o in objs]
    uv1s, uv2s = [np.asarray(u, np.float64) for u in uv1s], [np.asarray(u, np.float64) for u in uv2s]
    cams = (K1, D1, K2, D2)
    status, T1s, T2s = start(objs, uv1s, uv2s, cams)
    used = np.flatnonzero(status == 0)
    if R0 is None:
        R0, t0 = rig_start(T1s, T2s)
    r = joint([objs[i] for i in used], [uv1s[i] for i in used], [uv2s[i] for i in used], cams, [(T[:3, :3], T[:3, 3]) for T in T1s], R0, t0)
    T = np.full((len(objs), 4, 4), np.nan)
    T[:, 3] = [0, 0, 0, 1]
    err = np.full(len(objs), np.nan)
    for at, (Ri, ti), c in zip(used, r["poses"], r["frame_cost"]):
        T[at, :3, :3], T[at, :3, 3] = Ri, ti
        err[at] = np.sqrt(c / (2.0 * len(objs[at])))
    n = sum(len(objs[i]) for i in used)
    return dict(retval=float(np.sqrt(r["cost"] / (2.0 * n))), R=r["R"], t=r["t"].reshape(3, 1), T=T, reprojection_error=err,
                iterations=r["iterations"], status=status, evaluations=r["evaluations"], rig_status=r["status"],
                min_pivot=r["min_pivot"], R0=np.asarray(R0, np.float64), t0=np.asarray(t0, np.float64).reshape(3))
