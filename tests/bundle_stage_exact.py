"""An exact reference of one evaluation of the bundle adjustment (csrc/bundle.hip), in mpmath at ``DIGITS`` digits,
INDEPENDENT of the kernels' derivation and of tests/bundle_ref.py's.  CPU only; no GPU test imports it.

Only the model is written down here: the pinhole projection (``iz = z ? 1 / z : 1``, ``u = x fx + cx``), a view's local
parameters (``R <- exp([w]x) R, t <- t + d``), a point's (``X <- X + dX``), and the gauge: view ``fixed`` is held, the anchor
is moved by ``(w, e)`` with ``R' = exp([w]x) R, c' = c + e, t' = -R' c'`` (``c = -R^T t``) and coordinate ``axis`` of ``e`` is
held.  No Jacobian is written down, and neither is the anchor's matrix M: every derivative -- of a projection in a view's
``(w, d)``, in the anchor's ``(w, e)``, in the point, and of the map ``(w, e) -> (w, t' - t)`` itself -- is a central difference
with ``h = 1e-20``, whose truncation (h^2 f''' / 6 ~ 1e-35) and rounding (10^-DIGITS |f| / h ~ 1e-37) are far below float64.
The inputs are float64 values, or float32 values widened, taken as exact.

The damped normal system over (points, views) has the diagonal of every point's 3 x 3 block V and of every view's 6 x 6
block U in ``(w, d)`` scaled by ``1 + lambda``, the anchor's damping carried into ``(w, e)`` with its block (the header of
csrc/bundle.hip: ``M^T (S + lambda diag U) M``).  It is formed point by point, every point eliminated exactly
(``V*^-1`` from the cofactors of ``V* = V + lambda diag V``), the reduced system of the kept view parameters solved by
Cholesky, and every point's own step taken from its row of the full system: ``dX = -V*^-1 (G^T r + W_a^T y_a + W_b^T y_b)``.

Per chunk (``bundle._chunks``: the product's split) and per pair the 103 sums come in the kernels' packing --
    S_aa 21 | S_bb 21 | S_ba 6 x 6 (row: view b) | g_a 6 | g_b 6 | diag U_a 6 | diag U_b 6 | cost
in every view's ``(w, d)``, fixed view and anchor included, as k_bundle_linearise forms them -- each with its scale, the same
sum with every product replaced by its absolute value (for a Schur entry ``sum |J| |J| + sum |W| |V*^-1| |W|^T``), against
which every error of a float64 sum is measured.  Everything is rounded to float64 once, at the end."""
import numpy as np
from mpmath import mp, mpf

from solver_stage_exact import DIGITS, H, ONE, ZERO, cholesky, f64, rotate_left, solve

mp.dps = DIGITS
CHUNK = 256  # calibrating_amd._native.BUNDLE_CHUNK (asserted by tests/test_bundle_stage_cpu.py)
COST_RESOLUTION = mpf(64) * mpf(2) ** -52
BLOCKS = dict(aa=slice(0, 21), bb=slice(21, 42), ba=slice(42, 78), ga=slice(78, 84), gb=slice(84, 90), da=slice(90, 96),
              db=slice(96, 102), cost=slice(102, 103))
NORMAL, ANCHOR, FIXED = 0, 1, 2


def project(X, R, t, k):
    """(u, v, z) of the world point X in the view R (9, row-major), t, k = fx fy cx cy"""
    x = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0]
    y = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1]
    z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]
    iz = ONE / z if z != 0 else ONE
    return x * iz * k[0] + k[2], y * iz * k[1] + k[3], z


def centre(R, t):
    return [-(R[j] * t[0] + R[3 + j] * t[1] + R[6 + j] * t[2]) for j in range(3)]


def moved(R, t, p, anchored):
    """a view after its six local parameters: (w, d), or the anchor's (w, e)"""
    R2 = rotate_left(p[:3], R)
    if not anchored:
        return R2, [t[q] + p[3 + q] for q in range(3)]
    c = centre(R, t)
    c2 = [c[q] + p[3 + q] for q in range(3)]
    return R2, [-(R2[3 * i] * c2[0] + R2[3 * i + 1] * c2[1] + R2[3 * i + 2] * c2[2]) for i in range(3)]


def offsets(R, t, anchored):
    """the view at +h and -h of each of its six parameters: [(plus, minus)] x 6"""
    out = []
    for q in range(6):
        e = [ZERO] * 6
        e[q] = H
        plus = moved(R, t, e, anchored)
        e[q] = -H
        out.append((plus, moved(R, t, e, anchored)))
    return out


def anchor_map(R, t):
    """d (w, t' - t) / d (w, e) at 0 by central differences: 6 x 6, x = M y to first order"""
    cols = []
    for (Rp, tp), (Rm, tm) in offsets(R, t, True):
        cols.append([(a - b) / (2 * H) for a, b in zip(tp, tm)])
    M = [[ZERO] * 6 for _ in range(6)]
    for q in range(6):
        if q < 3:
            M[q][q] = ONE  # w is w
        for i in range(3):
            M[3 + i][q] = cols[q][i]
    return M


def jacobian(X, pairs_of_poses, k):
    """2 x len: the central differences of (u, v) of X over the given (plus, minus) views"""
    J = [[], []]
    for (Rp, tp), (Rm, tm) in pairs_of_poses:
        up, vp, _ = project(X, Rp, tp, k)
        um, vm, _ = project(X, Rm, tm, k)
        J[0].append((up - um) / (2 * H))
        J[1].append((vp - vm) / (2 * H))
    return J


def point_jacobian(X, R, t, k):
    J = [[], []]
    for j in range(3):
        Xp, Xm = list(X), list(X)
        Xp[j] += H
        Xm[j] -= H
        up, vp, _ = project(Xp, R, t, k)
        um, vm, _ = project(Xm, R, t, k)
        J[0].append((up - um) / (2 * H))
        J[1].append((vp - vm) / (2 * H))
    return J


def tmul(A, B):
    """A^T B of two 2-row matrices (or a 2-row matrix and a 2-vector given as a 2 x 1): cols(A) x cols(B)"""
    return [[A[0][p] * B[0][q] + A[1][p] * B[1][q] for q in range(len(B[0]))] for p in range(len(A[0]))]


def tmul_abs(A, B):
    return [[abs(A[0][p] * B[0][q]) + abs(A[1][p] * B[1][q]) for q in range(len(B[0]))] for p in range(len(A[0]))]


def inverse3(V):
    """(V^-1 from the cofactors, V is positive definite: its leading minors are positive)"""
    (a, b, c), (d, e, f), (g, h, i) = V
    C = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f],
         [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * C[0][0] + b * C[1][0] + c * C[2][0]
    return [[C[p][q] / det for q in range(3)] for p in range(3)], bool(a > 0 and a * e - b * d > 0 and det > 0)


def schur(Wl, Vi, Wr, absolute=False):
    """Wl V^-1 Wr^T: rows(Wl) x rows(Wr); ``absolute``: of the absolute values"""
    f = abs if absolute else (lambda v: v)
    T = [[sum(f(Wl[p][m]) * f(Vi[m][n]) for m in range(3)) for n in range(3)] for p in range(len(Wl))]
    return [[sum(T[p][n] * f(Wr[q][n]) for n in range(3)) for q in range(len(Wr))] for p in range(len(Wl))]


def sub(A, B):
    return [[x - y for x, y in zip(r, s)] for r, s in zip(A, B)]


def add(A, B):
    return [[x + y for x, y in zip(r, s)] for r, s in zip(A, B)]


def neg(A):
    return [[-x for x in r] for r in A]


def tri(M):
    return [M[p][q] for p in range(len(M)) for q in range(p + 1)]


def flat(M):
    return [v for row in M for v in row]


def zeros(n, m):
    return [[ZERO] * m for _ in range(n)]


def vadd(a, b):
    return [x + y for x, y in zip(a, b)]


def view_of(job, which):
    v = job[which]
    R, t, k = [mpf(x) for x in v["R"]], [mpf(x) for x in v["t"]], [mpf(x) for x in v["k"]]
    own = offsets(R, t, False)
    held = v["kind"] == FIXED
    gauge = None if held else (offsets(R, t, True) if v["kind"] == ANCHOR else own)
    return dict(R=R, t=t, k=k, own=own, gauge=gauge)


def linearise_job(job):
    """One chunk of one pair: job = dict(lam, a, b (R, t, k, kind), X, ua, ub) in floats -> the chunk's packed sums and their
    scales, its part of the reduced system in the gauge's parameters (damped and undamped), and per point what its own step
    needs: V*^-1, G^T r, W_a, W_b in the gauge's parameters, its depths, whether V* and V are definite"""
    mp.dps = DIGITS
    lam = mpf(job["lam"])
    a, b = view_of(job, "a"), view_of(job, "b")
    values, scales = [ZERO] * 103, [ZERO] * 103
    red = {lm: dict(aa=zeros(6, 6), bb=zeros(6, 6), ba=zeros(6, 6), ga=[ZERO] * 6, gb=[ZERO] * 6) for lm in ("damped", "undamped")}
    points = []
    for X, ua, ub in zip(job["X"], job["ua"], job["ub"]):
        X, ua, ub = [mpf(float(v)) for v in X], [mpf(float(v)) for v in ua], [mpf(float(v)) for v in ub]
        pa, pb = project(X, a["R"], a["t"], a["k"]), project(X, b["R"], b["t"], b["k"])
        ra, rb = [[pa[0] - ua[0]], [pa[1] - ua[1]]], [[pb[0] - ub[0]], [pb[1] - ub[1]]]
        Ja, Jb = jacobian(X, a["own"], a["k"]), jacobian(X, b["own"], b["k"])
        Ga, Gb = point_jacobian(X, a["R"], a["t"], a["k"]), point_jacobian(X, b["R"], b["t"], b["k"])
        V = add(tmul(Ga, Ga), tmul(Gb, Gb))
        Vd = [[V[p][q] * (1 + lam) if p == q else V[p][q] for q in range(3)] for p in range(3)]
        Vi, definite = inverse3(Vd)
        Vi0, definite0 = inverse3(V)
        gp = [x[0] for x in add(tmul(Ga, ra), tmul(Gb, rb))]
        Wa, Wb = tmul(Ja, Ga), tmul(Jb, Gb)
        # the packed sums, in every view's (w, d)
        val = tri(sub(tmul(Ja, Ja), schur(Wa, Vi, Wa))) + tri(sub(tmul(Jb, Jb), schur(Wb, Vi, Wb))) + flat(neg(schur(Wb, Vi, Wa)))
        mag = tri(add(tmul_abs(Ja, Ja), schur(Wa, Vi, Wa, True))) + tri(add(tmul_abs(Jb, Jb), schur(Wb, Vi, Wb, True))) + \
            flat(schur(Wb, Vi, Wa, True))
        for J, W, r in ((Ja, Wa, ra), (Jb, Wb, rb)):
            val += flat(sub(tmul(J, r), schur(W, Vi, [gp])))
            mag += flat(add(tmul_abs(J, r), schur(W, Vi, [gp], True)))
        for J in (Ja, Jb):
            d = [J[0][q] * J[0][q] + J[1][q] * J[1][q] for q in range(6)]
            val += d
            mag += d
        c = ra[0][0] * ra[0][0] + ra[1][0] * ra[1][0] + rb[0][0] * rb[0][0] + rb[1][0] * rb[1][0]
        values, scales = vadd(values, val + [c]), vadd(scales, mag + [c])
        # the gauge's parameters: nothing for the fixed view, (w, e) by differences for the anchor
        Jga = [[ZERO] * 6, [ZERO] * 6] if a["gauge"] is None else (Ja if a["gauge"] is a["own"] else jacobian(X, a["gauge"], a["k"]))
        Jgb = [[ZERO] * 6, [ZERO] * 6] if b["gauge"] is None else (Jb if b["gauge"] is b["own"] else jacobian(X, b["gauge"], b["k"]))
        Wga, Wgb = tmul(Jga, Ga), tmul(Jgb, Gb)
        for lm, inv in (("damped", Vi), ("undamped", Vi0)):
            s = red[lm]
            s["aa"] = add(s["aa"], sub(tmul(Jga, Jga), schur(Wga, inv, Wga)))
            s["bb"] = add(s["bb"], sub(tmul(Jgb, Jgb), schur(Wgb, inv, Wgb)))
            s["ba"] = add(s["ba"], neg(schur(Wgb, inv, Wga)))
            s["ga"] = vadd(s["ga"], flat(sub(tmul(Jga, ra), schur(Wga, inv, [gp]))))
            s["gb"] = vadd(s["gb"], flat(sub(tmul(Jgb, rb), schur(Wgb, inv, [gp]))))
        points.append(dict(Vi=Vi, gp=gp, Wa=Wga, Wb=Wgb, za=pa[2], zb=pb[2], definite=definite and definite0))
    return dict(values=values, scales=scales, reduced=red, points=points)


def candidate_job(job):
    """One chunk: job = dict(points (linearise_job's), ya, yb (the views' steps in the gauge's parameters), a2, b2 (the
    candidate views: R, t, k), X, ua, ub) -> per point dX, the chunk's candidate cost, |dX|^2, |X|^2, points behind a view"""
    mp.dps = DIGITS
    out = dict(dX=[], cost=ZERO, step2=ZERO, norm2=ZERO, behind=0)
    for p, X, ua, ub in zip(job["points"], job["X"], job["ua"], job["ub"]):
        X, ua, ub = [mpf(float(v)) for v in X], [mpf(float(v)) for v in ua], [mpf(float(v)) for v in ub]
        rhs = [p["gp"][n] + sum(p["Wa"][q][n] * job["ya"][q] + p["Wb"][q][n] * job["yb"][q] for q in range(6)) for n in range(3)]
        d = [-sum(p["Vi"][m][n] * rhs[n] for n in range(3)) for m in range(3)]
        Y = [X[q] + d[q] for q in range(3)]
        cost = ZERO
        for (R, t, k), uv in ((job["a2"], ua), (job["b2"], ub)):
            u, v, z = project(Y, R, t, k)
            cost += (u - uv[0]) ** 2 + (v - uv[1]) ** 2
            out["behind"] += int(not z > 0)
        out["dX"].append(d)
        out["cost"] += cost
        out["step2"] += sum(v * v for v in d)
        out["norm2"] += sum(v * v for v in X)
    return out


def evaluate(c, pool=None):
    """One case of tests/bundle_stage_cases.py -> dict of float64 arrays (the scales float32): partials, partials_scale
    (chunks x 103), pair_blocks, pair_scale (pairs x 103), step (views x 6, BS_STEP: (w, d), M y for the anchor), cand
    (views x 12: R, t), dX (used x 3), eval_partials (chunks x 3: cost, |dX|^2, |X|^2), eval_blocks (pairs x 3), cost,
    cand_cost, accept, pivot, pair_error (pairs), depth_a, depth_b (used), points_definite, reduced_definite, pivot_definite,
    behind (candidate points at z <= 0)."""
    from calibrating_amd import bundle
    run = map if pool is None else (lambda f, jobs: pool.map(f, jobs, chunksize=1))
    N, fixed = len(c["K"]), int(c["fixed_view"])
    anchor, axis = bundle.gauge(c["T0"], fixed)
    R64, t64 = bundle.poses_from_T(c["T0"])
    kind = lambda v: FIXED if v == fixed else (ANCHOR if v == anchor else NORMAL)  # noqa: E731
    views = [dict(R=[float(x) for x in R64[v].reshape(-1)], t=[float(x) for x in t64[v]],
                  k=[float(c["K"][v][0, 0]), float(c["K"][v][1, 1]), float(c["K"][v][0, 2]), float(c["K"][v][1, 2])], kind=kind(v))
             for v in range(N)]
    used = c["status"] == 0
    ua, ub, X = c["uvs_a"][used], c["uvs_b"][used], c["X"]
    bounds = np.concatenate([[0], np.cumsum(c["counts"])])
    used_counts = [int(used[bounds[p]:bounds[p + 1]].sum()) for p in range(len(c["pairs"]))]
    table, ranges = bundle._chunks(used_counts)
    pairs = [tuple(int(v) for v in p) for p in c["pairs"]]
    lam = float(c["lam"])
    rows = [slice(int(s), int(s) + int(n)) for _, s, n, _ in table]
    jobs = [dict(lam=lam, a=views[pairs[p][0]], b=views[pairs[p][1]], X=X[r], ua=ua[r], ub=ub[r]) for (p, _, _, _), r in zip(table, rows)]
    lin = list(run(linearise_job, jobs))
    P, n6 = len(pairs), 6 * N
    chunks_of = [range(int(ranges[p]), int(ranges[p + 1])) for p in range(P)]
    pair_values = [[sum(lin[ch]["values"][q] for ch in chunks_of[p]) for q in range(103)] for p in range(P)]
    pair_scales = [[sum(lin[ch]["scales"][q] for ch in chunks_of[p]) for q in range(103)] for p in range(P)]
    # the reduced system over all 6 N gauge parameters (the fixed view's rows stay empty), then its kept rows
    lam_m = mpf(lam)
    Ma = anchor_map(*[[mpf(x) for x in views[anchor][k]] for k in ("R", "t")])
    keep = [e for e in range(n6) if e // 6 != fixed and e != 6 * anchor + 3 + axis]

    def reduced(which, damping):
        S, g = zeros(n6, n6), [ZERO] * n6
        for p, (a, b) in enumerate(pairs):
            for ch in chunks_of[p]:
                s = lin[ch]["reduced"][which]
                for i in range(6):
                    g[6 * a + i] += s["ga"][i]
                    g[6 * b + i] += s["gb"][i]
                    for j in range(6):
                        S[6 * a + i][6 * a + j] += s["aa"][i][j]
                        S[6 * b + i][6 * b + j] += s["bb"][i][j]
                        S[6 * b + i][6 * a + j] += s["ba"][i][j]
                        S[6 * a + j][6 * b + i] += s["ba"][i][j]
        if damping:
            U = [ZERO] * n6
            for p, (a, b) in enumerate(pairs):
                for q in range(6):
                    U[6 * a + q] += pair_values[p][BLOCKS["da"].start + q]
                    U[6 * b + q] += pair_values[p][BLOCKS["db"].start + q]
            for v in range(N):
                if v == fixed:
                    continue
                for i in range(6):
                    for j in range(6):
                        if v == anchor:  # M^T diag(U) M
                            S[6 * v + i][6 * v + j] += lam_m * sum(Ma[m][i] * U[6 * v + m] * Ma[m][j] for m in range(6))
                        elif i == j:
                            S[6 * v + i][6 * v + i] += lam_m * U[6 * v + i]
        return [[S[i][j] for j in keep] for i in keep], [g[i] for i in keep]

    Sd, gd = reduced("damped", True)
    L, _ = cholesky(Sd)
    assert L is not None, "%s: the damped reduced matrix is not positive definite" % c["name"]
    yk = solve(L, [-v for v in gd])
    y = [ZERO] * n6
    for e, v in zip(keep, yk):
        y[e] = v
    step, cand = [], []
    for v in range(N):
        yv = y[6 * v:6 * v + 6]
        R, t = [mpf(x) for x in views[v]["R"]], [mpf(x) for x in views[v]["t"]]
        step.append([sum(Ma[i][m] * yv[m] for m in range(6)) for i in range(6)] if v == anchor else list(yv))
        R2, t2 = (R, t) if v == fixed else moved(R, t, yv, v == anchor)
        cand.append((list(R2), list(t2), [mpf(x) for x in views[v]["k"]]))
    jobs2 = [dict(points=lin[ch]["points"], ya=y[6 * pairs[p][0]:6 * pairs[p][0] + 6], yb=y[6 * pairs[p][1]:6 * pairs[p][1] + 6],
                  a2=cand[pairs[p][0]], b2=cand[pairs[p][1]], X=X[r], ua=ua[r], ub=ub[r]) for ch, ((p, _, _, _), r) in enumerate(zip(table, rows))]
    ev = list(run(candidate_job, jobs2))
    eval_partials = [[e["cost"], e["step2"], e["norm2"]] for e in ev]
    eval_blocks = [[sum(eval_partials[ch][q] for ch in chunks_of[p]) for q in range(3)] for p in range(P)]
    cost = sum(pv[102] for pv in pair_values)
    cand_cost = sum(e[0] for e in eval_blocks)
    behind = sum(e["behind"] for e in ev)
    accept = behind == 0 and (cand_cost < cost or cand_cost - cost <= COST_RESOLUTION * cost)
    # the final stage: undamped, scaled to a unit diagonal
    S0, _ = reduced("undamped", False)
    s = [ONE / mp.sqrt(S0[q][q]) for q in range(len(keep))]
    L0, pivots = cholesky([[S0[p][q] * s[p] * s[q] for q in range(len(keep))] for p in range(len(keep))])
    pts = [pt for l in lin for pt in l["points"]]
    return dict(
        partials=np.stack([f64(l["values"]) for l in lin]), partials_scale=np.stack([f64(l["scales"]) for l in lin]).astype(np.float32),
        pair_blocks=np.stack([f64(v) for v in pair_values]), pair_scale=np.stack([f64(v) for v in pair_scales]).astype(np.float32),
        step=np.stack([f64(v) for v in step]), cand=np.stack([f64(R2 + t2) for R2, t2, _ in cand]),
        dX=np.stack([f64(d) for e in ev for d in e["dX"]]), dX_rms=np.float64(float(mp.sqrt(sum(e["step2"] for e in ev) / len(pts)))),
        eval_partials=np.stack([f64(v) for v in eval_partials]),
        eval_blocks=np.stack([f64(v) for v in eval_blocks]), cost=np.float64(float(cost)), cand_cost=np.float64(float(cand_cost)),
        accept=np.array(bool(accept)), pivot=np.float64(float(min(pivots))),
        pair_error=f64([mp.sqrt(pv[102] / (2 * n)) for pv, n in zip(pair_values, used_counts)]),
        depth_a=f64([pt["za"] for pt in pts]), depth_b=f64([pt["zb"] for pt in pts]),
        points_definite=np.array(all(pt["definite"] for pt in pts)), reduced_definite=np.array(L is not None),
        pivot_definite=np.array(L0 is not None), behind=np.array(behind, np.int64))
