"""An exact reference of the start stage -- ``camd_pnp_init`` and ``camd_calib_homography`` as include/calibrating_amd.h
defines them -- in mpmath at ``DIGITS`` digits, from the float64 values of the inputs.  CPU only; no GPU test imports it.

Only the definition is written down: the ten rounds of ``camd_undistort_points``' iteration (they are part of the
definition: a start from the iteration's fixed point would be another start), the turn by ``plane``, the means and the
Hartley scales (mean distance sqrt 2 on the image side, sqrt D on the object side), the 2n x 3C rows and M = A^T A, the
eigenvector of M's smallest eigenvalue (``mpmath.eigsy``), the de-normalisation to G, and then scale, the sign from the
depth of the points' centre, Gram-Schmidt, ``R = R' plane`` and ``t = s h3 - c3 z0``.  No inverse iteration, no shift, no
summation order: what the kernel's six rounds and its butterfly approximate.  Everything is rounded to float64 once, at
the end."""
import numpy as np
from mpmath import mp, mpf

DIGITS = 60
mp.dps = DIGITS
ZERO, ONE = mpf(0), mpf(1)
UNDISTORT_ROUNDS = 10


def exact(a):
    """the float64 / float32 values of an array as mpf, exactly"""
    return [mpf(float(v)) for v in np.asarray(a).reshape(-1)]


def lens12(D):
    """k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 of 0, 4, 5, 8, 12 or 14 coefficients (tauX = tauY = 0)"""
    D = exact(D)
    assert len(D) in (0, 4, 5, 8, 12, 14) and all(v == 0 for v in D[12:])
    return D[:12] + [ZERO] * (12 - len(D[:12]))


def undistort(u, v, cam, D, ndist, rounds=UNDISTORT_ROUNDS):
    """camd_undistort_points' iteration on one pixel, before any hand-over: cam = fx fy cx cy"""
    x0, y0 = (u - cam[2]) / cam[0], (v - cam[3]) / cam[1]
    if ndist == 0:
        return x0, y0
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = D
    x, y = x0, y0
    for _ in range(rounds):
        r2 = x * x + y * y
        icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        if icdist < 0:
            return x0, y0
        dX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 * r2
        dY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r2 * r2
        x, y = (x0 - dX) * icdist, (y0 - dY) * icdist
    return x, y


def norm(v):
    return mp.sqrt(sum(a * a for a in v))


def unit(v):
    n = norm(v)
    return [a / n for a in v]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def dlt(X, xy):
    """X: n points of D coordinates, xy: n image points -> (G 3 x (D + 1) as rows, lambda1, lambda2, trace M)"""
    n, D = len(X), len(X[0])
    C = D + 1
    m = [sum(p[q] for p in X) / n for q in range(D)]
    mi = [sum(p[q] for p in xy) / n for q in range(2)]
    so = mp.sqrt(D) / (sum(norm([p[q] - m[q] for q in range(D)]) for p in X) / n)
    si = mp.sqrt(2) / (sum(norm([p[q] - mi[q] for q in range(2)]) for p in xy) / n)
    M = mp.zeros(3 * C)
    for p, u in zip(X, xy):
        h = [(p[q] - m[q]) * so for q in range(D)] + [ONE]
        x, y = (u[0] - mi[0]) * si, (u[1] - mi[1]) * si
        zero = [ZERO] * C
        for row in (h + zero + [-x * a for a in h], zero + h + [-y * a for a in h]):
            for i in range(3 * C):
                if row[i] != 0:
                    for j in range(3 * C):
                        M[i, j] += row[i] * row[j]
    E, Q = mp.eigsy(M)
    order = sorted(range(3 * C), key=lambda i: E[i])
    v = [Q[i, order[0]] for i in range(3 * C)]
    Gn = [v[C * r:C * r + C] for r in range(3)]
    # G = Ti^-1 Gn To: To = [so I, -so mean; 0 1], Ti^-1 = [1 / si, 0, mx; 0, 1 / si, my; 0, 0, 1]
    G = [[so * row[q] for q in range(D)] + [row[D] - so * sum(m[q] * row[q] for q in range(D))] for row in Gn]
    G = [[G[0][q] / si + mi[0] * G[2][q] for q in range(C)], [G[1][q] / si + mi[1] * G[2][q] for q in range(C)], G[2]]
    return G, E[order[0]], E[order[1]], sum(M[i, i] for i in range(3 * C))


def normalised(G):
    """unit Frobenius norm, the entry of largest magnitude positive"""
    flat = [a for row in G for a in row]
    s = norm(flat)
    if max(flat, key=abs) < 0:
        s = -s
    return [a / s for a in flat]


def frame(obj, uv, K, D, plane, kind):
    """One frame -> dict(G (9 or 12, normalised), pose (12: R row-major, t; NaN for a homography case), lambda1, lambda2,
    trace) as mpf.  kind: "planar", "cloud" or "homography" (a planar frame under an identity camera without a lens)."""
    ndist = 0 if kind == "homography" else len(np.ravel(D))
    Kx = exact(K)
    cam = [ONE, ONE, ZERO, ZERO] if kind == "homography" else [Kx[0], Kx[4], Kx[2], Kx[5]]
    lens = lens12(D if ndist else [])
    P = exact(plane)
    X = [exact(p) for p in obj]
    if kind != "cloud":
        X = [[sum(P[3 * i + q] * p[q] for q in range(3)) for i in range(3)] for p in X]
    xy = [undistort(mpf(float(u)), mpf(float(v)), cam, lens, ndist) for u, v in uv]
    n = len(X)
    centre = [sum(p[q] for p in X) / n for q in range(3)]
    if kind == "cloud":
        G, l1, l2, tr = dlt(X, xy)
        s = 1 / norm(G[2][:3])
        if sum(G[2][q] * centre[q] for q in range(3)) + G[2][3] < 0:
            s = -s
        r3 = unit([a * s for a in G[2][:3]])
        r1 = [a * s for a in G[0][:3]]
        d = sum(a * b for a, b in zip(r1, r3))
        r1 = unit([a - d * b for a, b in zip(r1, r3)])
        pose = r1 + cross(r3, r1) + r3 + [s * G[q][3] for q in range(3)]
    else:
        G, l1, l2, tr = dlt([p[:2] for p in X], xy)
        col = lambda q: [G[0][q], G[1][q], G[2][q]]  # noqa: E731
        s = 2 / (norm(col(0)) + norm(col(1)))
        if G[2][0] * centre[0] + G[2][1] * centre[1] + G[2][2] < 0:
            s = -s
        c1 = unit([a * s for a in col(0)])
        c2 = [a * s for a in col(1)]
        d = sum(a * b for a, b in zip(c1, c2))
        c2 = unit([a - d * b for a, b in zip(c2, c1)])
        c3 = cross(c1, c2)
        R = [c1[i] * P[j] + c2[i] * P[3 + j] + c3[i] * P[6 + j] for i in range(3) for j in range(3)]
        pose = R + [s * G[i][2] - c3[i] * centre[2] for i in range(3)]
    if kind == "homography":
        pose = [mpf("nan")] * 12
    return dict(G=normalised(G), pose=pose, lambda1=l1, lambda2=l2, trace=tr)


def f64(v):
    return np.array([float(x) for x in v], np.float64)


def _job(job):
    mp.dps = DIGITS
    return frame(*job)


def evaluate(c, pool=None):
    """One case of tests/pnp_start_cases.py -> dict of float64 arrays, a row per frame: G (9 or 12), pose (12),
    eigen (lambda1, lambda2, trace M)"""
    run = map if pool is None else pool.map
    out = list(run(_job, [(c["obj"], uv, c["K"], c["D"], c["plane"], c["kind"]) for uv in c["uv"]]))
    return dict(G=np.stack([f64(r["G"]) for r in out]), pose=np.stack([f64(r["pose"]) for r in out]),
                eigen=np.stack([f64([r["lambda1"], r["lambda2"], r["trace"]]) for r in out]))
