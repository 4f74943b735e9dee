"""An exact reference of one evaluation of the two joint solvers (csrc/calibrate.hip, csrc/stereo_calibrate.hip), in
mpmath at ``DIGITS`` digits, INDEPENDENT of the kernels' derivation.  CPU only; no GPU test imports it.

Only the model is written down here: the projection as include/calibrating_amd.h documents it for
``camd_project_points`` (``iz = Z ? 1 / Z : 1``, the rational / tangential / thin-prism polynomial, ``u = xd fx + cx``), the
local parameters (``R <- exp([w]x) R, t <- t + d`` for a frame, the same for the rig with ``x2 = R x1 + t``, and ``fx fy cx
cy k1 k2 p1 p2 k3``) and the Levenberg-Marquardt step through the Schur complement.  No Jacobian is written down: every
derivative is a central difference of that projection with ``h = 1e-20``, whose truncation (h^2 f''' / 6 ~ 1e-35) and
rounding (10^-DIGITS |f| / h ~ 1e-37) are both far below float64.  The inputs are float64 values, or float32 values
widened, taken as exact.

Per used frame the sums come in the kernels' packing --
    calibrate: A 21 | B 6 x 9 | C 45 | gp 6 | gk 9 | c          stereo: A 21 | B 6 x 6 | C 21 | gp 6 | gr 6 | c
(triangles packed row by row, ``p (p + 1) / 2 + q``) -- each with its scale ``sum_i |a_i| |b_i|``, the sum of absolute
products, against which every error of a float64 sum is measured.  From the unrounded sums: the damped reduced system at
the case's lambda, the shared step, every frame's step and candidate, each candidate's cost, the accept decision, and the
final stage's numbers (the smallest pivot of the undamped reduced matrix scaled to a unit diagonal, the cost, the
per-frame error).  Everything is rounded to float64 once, at the end."""
import numpy as np
from mpmath import mp, mpf

DIGITS = 60
mp.dps = DIGITS
H = mpf(10) ** -20
ZERO, ONE = mpf(0), mpf(1)
CALIB_WS, STEREO_WS = 136, 91


def exact(a):
    """the float64 / float32 values of an array as mpf, exactly"""
    return [mpf(float(v)) for v in np.asarray(a).reshape(-1)]


def lens12(D):
    """k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 of 0, 4, 5, 8 or 12 coefficients"""
    assert len(D) in (0, 4, 5, 8, 12)
    return list(D) + [ZERO] * (12 - len(D))


def project(X, R, t, cam, D):
    """camd_project_points' model: one point X under R (9, row-major), t, cam = fx fy cx cy and the twelve lens coefficients"""
    Xc = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0]
    Yc = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1]
    Zc = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]
    iz = ONE / Zc if Zc != 0 else ONE
    x, y = Xc * iz, Yc * iz
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = D
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    radial = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r4
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r4
    return xd * cam[0] + cam[2], yd * cam[1] + cam[3]


def rotate_left(w, R):
    """exp([w]x) R: Rodrigues' formula, I + sin(th) / th [w]x + (1 - cos th) / th^2 [w]x^2 with 1 - cos th = 2 sin^2(th / 2)"""
    th = mp.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th == 0:
        return list(R)
    a, s = mp.sin(th) / th, mp.sin(th / 2) / (th / 2)
    b = s * s / 2
    W = [[ZERO, -w[2], w[1]], [w[2], ZERO, -w[0]], [-w[1], w[0], ZERO]]
    W2 = [[sum(W[i][m] * W[m][j] for m in range(3)) for j in range(3)] for i in range(3)]
    E = [[(ONE if i == j else ZERO) + a * W[i][j] + b * W2[i][j] for j in range(3)] for i in range(3)]
    return [sum(E[i][m] * R[3 * m + j] for m in range(3)) for i in range(3) for j in range(3)]


def compose(R, t, Ri, ti):
    """the frame's pose in camera 2: x2 = R (Ri X + ti) + t"""
    Rc = [sum(R[3 * i + m] * Ri[3 * m + j] for m in range(3)) for i in range(3) for j in range(3)]
    tc = [sum(R[3 * i + m] * ti[m] for m in range(3)) + t[i] for i in range(3)]
    return Rc, tc


# ---- residuals of one frame over its local parameters ------------------------------------------------------------
def calib_residuals(fr, p):
    """fr: dict(obj, uv, R, t, k); p: 15 offsets (w 3, d 3, fx fy cx cy k1 k2 p1 p2 k3) -> 2n residuals"""
    R, t = rotate_left(p[0:3], fr["R"]), [fr["t"][q] + p[3 + q] for q in range(3)]
    k = [fr["k"][q] + p[6 + q] for q in range(9)]
    D = lens12(k[4:9])
    out = []
    for X, uv in zip(fr["obj"], fr["uv"]):
        u, v = project(X, R, t, k[:4], D)
        out += [u - uv[0], v - uv[1]]
    return out


def stereo_residuals(fr, p):
    """fr: dict(obj, uv1, uv2, R, t (the board in camera 1), rigR, rigt, cam1, D1, cam2, D2); p: 12 offsets (the frame's
    w 3, d 3; the rig's w 3, d 3) -> (camera 1's 2n residuals, camera 2's)"""
    Ri, ti = rotate_left(p[0:3], fr["R"]), [fr["t"][q] + p[3 + q] for q in range(3)]
    R, t = rotate_left(p[6:9], fr["rigR"]), [fr["rigt"][q] + p[9 + q] for q in range(3)]
    Rc, tc = compose(R, t, Ri, ti)
    r1, r2 = [], []
    for X, a, b in zip(fr["obj"], fr["uv1"], fr["uv2"]):
        u, v = project(X, Ri, ti, fr["cam1"], fr["D1"])
        r1 += [u - a[0], v - a[1]]
        u, v = project(X, Rc, tc, fr["cam2"], fr["D2"])
        r2 += [u - b[0], v - b[1]]
    return r1, r2


def central_differences(f, params, which):
    """columns d f / d p_q for q in ``which``: (f(+h e_q) - f(-h e_q)) / 2h -> rows x len(which)"""
    cols = []
    for q in which:
        e = [ZERO] * params
        e[q] = H
        plus = f(e)
        e[q] = -H
        minus = f(e)
        cols.append([(a - b) / (2 * H) for a, b in zip(plus, minus)])
    return [list(row) for row in zip(*cols)]


def products(Ja, Jb):
    """(sum_i Ja[i]^T Jb[i], the same of absolute values): len(Ja[0]) x len(Jb[0])"""
    na, nb = len(Ja[0]), len(Jb[0])
    val = [[ZERO] * nb for _ in range(na)]
    mag = [[ZERO] * nb for _ in range(na)]
    for a, b in zip(Ja, Jb):
        for p in range(na):
            for q in range(nb):
                v = a[p] * b[q]
                val[p][q] += v
                mag[p][q] += abs(v)
    return val, mag


def add(a, b):
    return [[x + y for x, y in zip(r, s)] for r, s in zip(a, b)]


def column(r):
    return [[v] for v in r]


def blocks_of(terms):
    """terms: [(J of the frame, J of the shared block, r)] summed (stereo: camera 1 with no shared part, then camera 2) ->
    dict(A, B, C, gp, gs, c) as (values, scales); gp, gs are lists, c a number"""
    out = None
    for Jf, Js, r in terms:
        A, B, C = products(Jf, Jf), products(Jf, Js), products(Js, Js)
        gp, gs, c = products(Jf, column(r)), products(Js, column(r)), products(column(r), column(r))
        new = dict(A=A, B=B, C=C, gp=gp, gs=gs, c=c)
        out = new if out is None else {k: (add(out[k][0], new[k][0]), add(out[k][1], new[k][1])) for k in new}
    return out


def calib_frame(fr):
    fr = {k: v for k, v in fr.items()}
    r = calib_residuals(fr, [ZERO] * 15)
    J = central_differences(lambda p: calib_residuals(fr, p), 15, range(15))
    return blocks_of([([row[:6] for row in J], [row[6:] for row in J], r)])


def stereo_frame(fr):
    r1, r2 = stereo_residuals(fr, [ZERO] * 12)
    J1 = central_differences(lambda p: stereo_residuals(fr, p)[0], 12, range(6))
    J2 = central_differences(lambda p: stereo_residuals(fr, p)[1], 12, range(12))
    none = [[ZERO] * 6 for _ in r1]  # camera 1 does not see the rig
    return blocks_of([(J1, none, r1), ([row[:6] for row in J2], [row[6:] for row in J2], r2)])


def pack(b, which):
    """the workspace row of one frame, values (which = 0) or scales (1)"""
    A, B, C, gp, gs, c = (b[k][which] for k in ("A", "B", "C", "gp", "gs", "c"))
    tri = lambda M: [M[p][q] for p in range(len(M)) for q in range(p + 1)]  # noqa: E731
    return tri(A) + [v for row in B for v in row] + tri(C) + [v[0] for v in gp] + [v[0] for v in gs] + [c[0][0]]


# ---- a symmetric positive definite system -------------------------------------------------------------------------
def cholesky(M):
    """(L, the pivots d_j = L_jj^2) or (None, pivots so far) where one is not positive"""
    n = len(M)
    L = [[ZERO] * n for _ in range(n)]
    pivots = []
    for j in range(n):
        d = M[j][j] - sum(L[j][q] * L[j][q] for q in range(j))
        pivots.append(d)
        if not d > 0:
            return None, pivots
        L[j][j] = mp.sqrt(d)
        for i in range(j + 1, n):
            L[i][j] = (M[i][j] - sum(L[i][q] * L[j][q] for q in range(j))) / L[j][j]
    return L, pivots


def solve(L, b):
    n = len(L)
    x = list(b)
    for i in range(n):
        x[i] = (x[i] - sum(L[i][q] * x[q] for q in range(i))) / L[i][i]
    for i in reversed(range(n)):
        x[i] = (x[i] - sum(L[q][i] * x[q] for q in range(i + 1, n))) / L[i][i]
    return x


def damped(M, lam, diag=None):
    diag = [M[q][q] for q in range(len(M))] if diag is None else diag
    return [[M[p][q] + (lam * diag[p] if p == q else 0) for q in range(len(M))] for p in range(len(M))]


def reduced(blocks, lam):
    """(S, g, diag sum C, the frames' factors) of the shared block; a factor is None where a frame's damped A is not
    positive definite"""
    m = len(blocks[0]["C"][0])
    S, g, dC, Ls = [[ZERO] * m for _ in range(m)], [ZERO] * m, [ZERO] * m, []
    for b in blocks:
        A, B, C, gp, gs = (b[k][0] for k in ("A", "B", "C", "gp", "gs"))
        L, _ = cholesky(damped(A, lam))
        Ls.append(L)
        if L is None:
            continue
        Y = [solve(L, [B[p][q] for p in range(6)]) for q in range(m)]  # column q of A^-1 B
        y = solve(L, [v[0] for v in gp])
        for p in range(m):
            for q in range(m):
                S[p][q] += C[p][q] - sum(B[e][p] * Y[q][e] for e in range(6))
            g[p] += gs[p][0] - sum(B[e][p] * y[e] for e in range(6))
            dC[p] += C[p][p]
    return S, g, dC, Ls


def masked(S, g, mask):
    """a fixed entry: a unit row and column, a zero right-hand side"""
    m = len(S)
    fixed = [mask is not None and mask[q] == 0 for q in range(m)]
    S = [[(ONE if p == q else ZERO) if fixed[p] or fixed[q] else S[p][q] for q in range(m)] for p in range(m)]
    return S, [ZERO if fixed[q] else g[q] for q in range(m)]


def unit_diagonal_pivot(S, mask):
    """the smallest Cholesky pivot of S scaled to a unit diagonal (the scale from the unmasked diagonal, then the mask)"""
    m = len(S)
    s = [ONE / mp.sqrt(S[q][q]) for q in range(m)]
    T, _ = masked([[S[p][q] * s[p] * s[q] for q in range(m)] for p in range(m)], [ZERO] * m, mask)
    L, pivots = cholesky(T)
    return min(pivots), L is not None


def f64(v):
    return np.array([float(x) for x in v], np.float64)


def _frame_job(job):
    kind, fr = job
    mp.dps = DIGITS
    return calib_frame(fr) if kind == "calib" else stereo_frame(fr)


def _cost_job(job):
    kind, fr = job
    mp.dps = DIGITS
    if kind == "calib":
        return sum(v * v for v in calib_residuals(fr, [ZERO] * 15))
    r1, r2 = stereo_residuals(fr, [ZERO] * 12)
    return sum(v * v for v in r1) + sum(v * v for v in r2)


def frame_inputs(c):
    """every frame of a case (tests/solver_stage_cases.py) as exact numbers"""
    start = np.concatenate([[0], np.cumsum(c["counts"])])
    kind = str(c["kind"])
    out = []
    for f, n in enumerate(c["counts"]):
        s, n = int(start[f]), int(n)
        obj = np.asarray(c["obj"])[:n] if bool(c["shared"]) else np.asarray(c["obj"])[s:s + n]
        fr = dict(obj=[exact(X) for X in obj], R=exact(c["poses"][f, :9]), t=exact(c["poses"][f, 9:]))
        if kind == "calib":
            fr.update(uv=[exact(u) for u in c["uv"][s:s + n]], k=exact(c["k"]))
        else:
            fr.update(uv1=[exact(u) for u in c["uv1"][s:s + n]], uv2=[exact(u) for u in c["uv2"][s:s + n]],
                      rigR=exact(c["rig"][:9]), rigt=exact(c["rig"][9:]),
                      cam1=[exact(c["K1"])[q] for q in (0, 4, 2, 5)], cam2=[exact(c["K2"])[q] for q in (0, 4, 2, 5)],
                      D1=lens12(exact(c["D1"])), D2=lens12(exact(c["D2"])))
        out.append(fr)
    return out


def evaluate(c, pool=None, workspace=True):
    """One case -> dict of float64 arrays: ws, scale (frames x 136 or 91; left out with workspace=False), step (9 or 6),
    shared (the candidate K, 9, or rig, 12), cand (frames x 16: R 9, t 3, cost, |step|^2, |pose|^2, 0), cost, cand_cost,
    accept, frames_definite, reduced_definite, pivot, pivot_definite, frame_error."""
    run = map if pool is None else (lambda f, jobs: pool.map(f, jobs, chunksize=max(1, len(jobs) // 256)))
    kind = str(c["kind"])
    frames = frame_inputs(c)
    blocks = list(run(_frame_job, [(kind, fr) for fr in frames]))
    lam = mpf(float(c["lam"]))
    mask = exact(c["mask"]) if kind == "calib" else None
    m = 9 if kind == "calib" else 6
    S, g, dC, Ls = reduced(blocks, lam)
    frames_definite = all(L is not None for L in Ls)
    Sd, gd = masked(damped(S, lam, dC), g, mask)
    L, _ = cholesky(Sd)
    assert frames_definite and L is not None, "%s: the damped system is not positive definite" % c["name"]
    step = solve(L, [-v for v in gd])
    if kind == "calib":
        shared = [a + b for a, b in zip(frames[0]["k"], step)]
    else:
        shared = rotate_left(step[:3], frames[0]["rigR"]) + [frames[0]["rigt"][q] + step[3 + q] for q in range(3)]
    cand, moved = [], []
    for fr, b, Lf in zip(frames, blocks, Ls):
        B, gp = b["B"][0], b["gp"][0]
        d = solve(Lf, [-(gp[p][0] + sum(B[p][q] * step[q] for q in range(m))) for p in range(6)])
        R2, t2 = rotate_left(d[:3], fr["R"]), [fr["t"][q] + d[3 + q] for q in range(3)]
        moved.append(dict(fr, R=R2, t=t2, **(dict(k=shared) if kind == "calib" else dict(rigR=shared[:9], rigt=shared[9:]))))
        cand.append(R2 + t2 + [ZERO, sum(v * v for v in d), 3 + sum(v * v for v in fr["t"]), ZERO])
    for row, c2 in zip(cand, run(_cost_job, [(kind, fr) for fr in moved])):
        row[12] = c2
    cost = sum(b["c"][0][0][0] for b in blocks)
    cand_cost = sum(row[12] for row in cand)
    S0, _, _, L0 = reduced(blocks, ZERO)
    pivot, pivot_definite = unit_diagonal_pivot(S0, mask)
    per_point = 1 if kind == "calib" else 2
    out = dict(step=f64(step), shared=f64(shared), cand=np.stack([f64(row) for row in cand]), cost=np.float64(float(cost)),
               cand_cost=np.float64(float(cand_cost)), accept=np.array(bool(cand_cost < cost)),
               frames_definite=np.array(frames_definite and all(l is not None for l in L0)), reduced_definite=np.array(L is not None),
               pivot=np.float64(float(pivot)), pivot_definite=np.array(pivot_definite),
               frame_error=f64([mp.sqrt(b["c"][0][0][0] / (per_point * int(n))) for b, n in zip(blocks, c["counts"])]))
    if workspace:
        out["ws"] = np.stack([f64(pack(b, 0)) for b in blocks])
        out["scale"] = np.stack([f64(pack(b, 1)) for b in blocks]).astype(np.float32)
    return out
