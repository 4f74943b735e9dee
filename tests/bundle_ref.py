"""NumPy float64 restatement of the joint refinement of ``csrc/bundle.hip`` / ``calibrating_amd/bundle.py``.  Test
infrastructure only.

The same problem (one world point per match, two observations; the world-to-camera pose of every view with pnp.hip's local
perturbation), the same gauge (the pose of ``fixed_view``; one coordinate of the anchor's centre, through the anchor's
``(w, e)`` step and ``M = [I 0; -[t]x -R]``), the same Levenberg-Marquardt rule (damping ``lambda diag``, acceptance within
64 ulp of the cost, a candidate with a point at ``z <= 0`` rejected, the stop, the cap) and the same status words as the
kernels.  The start point and the status of a match are restated operation by operation, every sum left to right, so the
kernels must give the same BITS; the solver uses dense arithmetic and NumPy's order of the sums over points and pairs,
which is what tests/golden/bundle_tolerance.json measures.

Central differences with ``FD_STEP`` = 1e-6 check the Jacobians.  A residual is a pixel: f ~ 70 times a ratio of
coordinates that a unit of rotation, or of (translation / depth) with depths of 2.5 and more, moves by O(1); its third
derivatives stay below about 6 f ~ 4e2 px per unit^3, the truncation h^2 / 6 |f'''| below 1e-10 and the rounding 2^-52 |f|
/ h below 1e-8 px per unit.  ``FD_BOUND`` = 1e-6 px per unit, on entries of 1 .. 1e2.
"""
import numpy as np

EPS = 2.0 ** -52
MAX_EVALUATIONS = 100
SINGULAR_PIVOT = 1e-10
COST_RESOLUTION = 64 * EPS
MIN_SINE = 0.03  # |d_a x d_b| of the unit rays below which a match has no start (status 2)
MAX_VIEWS = 16
MIN_OBSERVATIONS = 6
FD_STEP, FD_BOUND = 1e-6, 1e-6


def rotate_left(w, R):
    """exp([w]x) R as csrc/pnp_common.hpp's rotate_left forms it"""
    w = np.asarray(w, np.float64)
    th = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    h = 0.5 * th
    A = np.sin(th) / th if th > 0 else 1.0
    sh = np.sin(h) / h if h > 0 else 1.0
    B = 0.5 * sh * sh
    E = np.array([[1 - B * (w[1] * w[1] + w[2] * w[2]), B * w[0] * w[1] - A * w[2], B * w[0] * w[2] + A * w[1]],
                  [B * w[0] * w[1] + A * w[2], 1 - B * (w[0] * w[0] + w[2] * w[2]), B * w[1] * w[2] - A * w[0]],
                  [B * w[0] * w[2] - A * w[1], B * w[1] * w[2] + A * w[0], 1 - B * (w[0] * w[0] + w[1] * w[1])]])
    return E @ R


def poses_from_T(T):
    """camera to world (N, 4, 4) -> world to camera R (N, 3, 3), t (N, 3), as ``bundle.py`` hands them to the device"""
    T = np.asarray(T, np.float64)
    R = np.ascontiguousarray(np.swapaxes(T[:, :3, :3], 1, 2))
    c = T[:, :3, 3]
    t = -np.stack([R[:, i, 0] * c[:, 0] + R[:, i, 1] * c[:, 1] + R[:, i, 2] * c[:, 2] for i in range(3)], 1)
    return R, t


def T_from_poses(R, t):
    T = np.zeros((len(R), 4, 4))
    T[:, 3, 3] = 1
    T[:, :3, :3] = np.swapaxes(R, 1, 2)
    T[:, :3, 3] = -np.stack([R[:, 0, j] * t[:, 0] + R[:, 1, j] * t[:, 1] + R[:, 2, j] * t[:, 2] for j in range(3)], 1)
    return T


def gauge(T, fixed_view):
    """(anchor view, axis): the view whose start centre is farthest from the fixed view's, and the coordinate of largest
    magnitude of the difference of the centres; ties to the lower view and the lower axis"""
    c = np.asarray(T, np.float64)[:, :3, 3]
    d2 = ((c - c[fixed_view]) ** 2).sum(1)
    d2[fixed_view] = -1.0
    anchor = int(np.argmax(d2))
    return anchor, int(np.argmax(np.abs(c[anchor] - c[fixed_view])))


def k4(K):
    K = np.asarray(K, np.float64)
    return np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1)


def observe(R, t, k, X, uv, terms=True):
    """z (n,), r (n, 2) and with ``terms`` J (n, 2, 6), G (n, 2, 3) of the points X (n, 3) in one view"""
    P = [R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1] + R[i, 2] * X[:, 2] for i in range(3)]
    z = P[2] + t[2]
    with np.errstate(all="ignore"):
        iz = np.where(z != 0, 1.0 / np.where(z != 0, z, 1.0), 1.0)
    x, y = (P[0] + t[0]) * iz, (P[1] + t[1]) * iz
    r = np.stack([x * k[0] + k[2] - uv[:, 0], y * k[1] + k[3] - uv[:, 1]], 1)
    if not terms:
        return z, r
    zero = np.zeros_like(z)
    g = [[k[0] * iz, zero, -(k[0] * x) * iz], [zero, k[1] * iz, -(k[1] * y) * iz]]
    J = np.empty((len(z), 2, 6))
    G = np.empty((len(z), 2, 3))
    for e in range(2):
        J[:, e, 0] = P[1] * g[e][2] - P[2] * g[e][1]
        J[:, e, 1] = P[2] * g[e][0] - P[0] * g[e][2]
        J[:, e, 2] = P[0] * g[e][1] - P[1] * g[e][0]
        for j in range(3):
            J[:, e, 3 + j] = g[e][j]
            G[:, e, j] = g[e][0] * R[0, j] + g[e][1] * R[1, j] + g[e][2] * R[2, j]
    return z, r, J, G


def start(K, R, t, pairs, uvs_a, uvs_b, counts, threshold=None):
    """(points (M, 3), status (M,) int32) of every match, operation by operation as k_bundle_start"""
    k = k4(K)
    uvs_a, uvs_b = np.asarray(uvs_a).astype(np.float64), np.asarray(uvs_b).astype(np.float64)
    M = len(uvs_a)
    points, status = np.full((M, 3), np.nan), np.ones(M, np.int32)
    at = 0
    for (a, b), n in zip(pairs, counts):
        ua, ub = uvs_a[at:at + n], uvs_b[at:at + n]
        with np.errstate(all="ignore"):
            d, c = [], []
            for v, uv in ((a, ua), (b, ub)):
                x, y = (uv[:, 0] - k[v, 2]) * (1.0 / k[v, 0]), (uv[:, 1] - k[v, 3]) * (1.0 / k[v, 1])
                dv = [R[v, 0, j] * x + R[v, 1, j] * y + R[v, 2, j] for j in range(3)]
                c.append([-(R[v, 0, j] * t[v, 0] + R[v, 1, j] * t[v, 1] + R[v, 2, j] * t[v, 2]) for j in range(3)])
                n2 = (0.0 + dv[0] * dv[0]) + dv[1] * dv[1] + dv[2] * dv[2]
                inv = 1.0 / np.sqrt(n2)
                d.append([q * inv for q in dv])
            da, db = d
            cr = [da[1] * db[2] - da[2] * db[1], da[2] * db[0] - da[0] * db[2], da[0] * db[1] - da[1] * db[0]]
            s2 = cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]
            w = [c[0][j] - c[1][j] for j in range(3)]
            bb = da[0] * db[0] + da[1] * db[1] + da[2] * db[2]
            dd = da[0] * w[0] + da[1] * w[1] + da[2] * w[2]
            ee = db[0] * w[0] + db[1] * w[1] + db[2] * w[2]
            inv = 1.0 / s2
            sa, sb = (bb * ee - dd) * inv, (ee - bb * dd) * inv
            Y = np.stack([0.5 * ((c[0][j] + sa * da[j]) + (c[1][j] + sb * db[j])) for j in range(3)], 1)
            za, ra = observe(R[a], t[a], k[a], Y, ua, terms=False)
            zb, rb = observe(R[b], t[b], k[b], Y, ub, terms=False)
            ea, eb = ra[:, 0] * ra[:, 0] + ra[:, 1] * ra[:, 1], rb[:, 0] * rb[:, 0] + rb[:, 1] * rb[:, 1]
            finite = np.isfinite(ua).all(1) & np.isfinite(ub).all(1)
            front = (s2 >= MIN_SINE * MIN_SINE) & (za > 0) & (zb > 0) & np.isfinite(Y).all(1)
            far = np.zeros(n, bool) if threshold is None else ((ea > threshold * threshold) | (eb > threshold * threshold))
        st = np.where(~finite, 1, np.where(~front, 2, np.where(far, 3, 0))).astype(np.int32)
        status[at:at + n] = st
        points[at:at + n] = np.where((st == 0)[:, None], Y, np.nan)
        at += n
    return points, status


def point_terms(qa, qb, X, ua, ub, lam):
    """what csrc/bundle.hip's point_terms forms for the points of one pair; q = (R, t, k4) of a view"""
    za, ra, Ja, Ga = observe(*qa, X, ua)
    zb, rb, Jb, Gb = observe(*qb, X, ub)
    n = len(X)
    V = {}
    for p in range(3):
        for q in range(p + 1):
            V[p, q] = (Ga[:, 0, p] * Ga[:, 0, q] + Ga[:, 1, p] * Ga[:, 1, q]) + (Gb[:, 0, p] * Gb[:, 0, q] + Gb[:, 1, p] * Gb[:, 1, q])
    gp = [(Ga[:, 0, p] * ra[:, 0] + Ga[:, 1, p] * ra[:, 1]) + (Gb[:, 0, p] * rb[:, 0] + Gb[:, 1, p] * rb[:, 1]) for p in range(3)]
    with np.errstate(all="ignore"):
        d0 = V[0, 0] + lam * V[0, 0]
        l00 = np.sqrt(d0)
        i0 = 1.0 / l00
        l10, l20 = V[1, 0] * i0, V[2, 0] * i0
        d1 = (V[1, 1] + lam * V[1, 1]) - l10 * l10
        l11 = np.sqrt(d1)
        i1 = 1.0 / l11
        l21 = (V[2, 1] - l20 * l10) * i1
        d2 = (V[2, 2] + lam * V[2, 2]) - l20 * l20 - l21 * l21
        l22 = np.sqrt(d2)
        i2 = 1.0 / l22
        ok = (d0 > 0) & (d1 > 0) & (d2 > 0) & np.isfinite(d0) & np.isfinite(d1) & np.isfinite(d2)

        def forward(w0, w1, w2):
            z0 = w0 * i0
            z1 = (w1 - l10 * z0) * i1
            return z0, z1, (w2 - l20 * z0 - l21 * z1) * i2

        Za, Zb = np.empty((n, 3, 6)), np.empty((n, 3, 6))
        for i in range(6):
            Za[:, 0, i], Za[:, 1, i], Za[:, 2, i] = forward(*[Ja[:, 0, i] * Ga[:, 0, q] + Ja[:, 1, i] * Ga[:, 1, q] for q in range(3)])
            Zb[:, 0, i], Zb[:, 1, i], Zb[:, 2, i] = forward(*[Jb[:, 0, i] * Gb[:, 0, q] + Jb[:, 1, i] * Gb[:, 1, q] for q in range(3)])
        y = np.stack(forward(*gp), 1)
    return dict(ra=ra, rb=rb, Ja=Ja, Jb=Jb, Za=Za, Zb=Zb, y=y, ok=ok, L=(l10, l20, l21), il=(i0, i1, i2), za=za, zb=zb)


def _outer(A, B):
    s = A[:, 0, :, None] * B[:, 0, None, :]
    for e in range(1, A.shape[1]):
        s = s + A[:, e, :, None] * B[:, e, None, :]
    return s


def pair_block(o):
    """the sums of one pair: S_aa, S_bb, S_ba, g_a, g_b, diag U_a, diag U_b, cost, points that did not factor"""
    Ja, Jb, Za, Zb, ra, rb, y = o["Ja"], o["Jb"], o["Za"], o["Zb"], o["ra"], o["rb"], o["y"]
    ga = (Ja[:, 0] * ra[:, :1] + Ja[:, 1] * ra[:, 1:]) - (Za[:, 0] * y[:, :1] + Za[:, 1] * y[:, 1:2] + Za[:, 2] * y[:, 2:])
    gb = (Jb[:, 0] * rb[:, :1] + Jb[:, 1] * rb[:, 1:]) - (Zb[:, 0] * y[:, :1] + Zb[:, 1] * y[:, 1:2] + Zb[:, 2] * y[:, 2:])
    cost = (ra[:, 0] * ra[:, 0] + ra[:, 1] * ra[:, 1]) + (rb[:, 0] * rb[:, 0] + rb[:, 1] * rb[:, 1])
    return dict(aa=(_outer(Ja, Ja) - _outer(Za, Za)).sum(0), bb=(_outer(Jb, Jb) - _outer(Zb, Zb)).sum(0),
                ba=(-_outer(Zb, Za)).sum(0), ga=ga.sum(0), gb=gb.sum(0),
                da=(Ja[:, 0] * Ja[:, 0] + Ja[:, 1] * Ja[:, 1]).sum(0), db=(Jb[:, 0] * Jb[:, 0] + Jb[:, 1] * Jb[:, 1]).sum(0),
                cost=cost.sum(), bad=int((~o["ok"]).sum()))


def anchor_matrix(R, t):
    """x = M y: the anchor's (w, d) from its (w, e), e a shift of its world centre"""
    M = np.zeros((6, 6))
    M[:3, :3] = np.eye(3)
    M[3:, :3] = [[0, t[2], -t[1]], [-t[2], 0, t[0]], [t[1], -t[0], 0]]
    M[3:, 3:] = -R
    return M


def _cholesky(A):
    """lower L with A = L L^T (right-looking, as k_bundle_solve), the smallest pivot; L is None where a pivot is not > 0"""
    L = np.array(A, np.float64)
    n = len(L)
    pivot, ok = np.inf, True
    with np.errstate(all="ignore"):
        for j in range(n):
            d = L[j, j]
            pivot = min(pivot, d) if np.isfinite(d) else d
            ok = ok and d > 0 and np.isfinite(d)
            r = np.sqrt(d)
            L[j, j] = r
            L[j + 1:, j] *= 1.0 / r
            L[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return (np.tril(L) if ok else None), float(pivot)


def _solve(L, b):
    x = np.array(b, np.float64)
    n = len(x)
    for j in range(n):
        x[j] = x[j] / L[j, j]
        x[j + 1:] -= L[j + 1:, j] * x[j]
    for j in range(n - 1, -1, -1):
        x[j] = x[j] / L[j, j]
        x[:j] -= L[j, :j] * x[j]
    return x


class Problem:
    def __init__(self, K, R, t, pairs, uvs_a, uvs_b, offsets, fixed, anchor, axis):
        self.k, self.pairs, self.offsets = k4(K), pairs, offsets
        self.ua, self.ub = uvs_a, uvs_b
        self.N, self.fixed, self.anchor, self.axis = len(R), fixed, anchor, axis
        self.keep = [e for e in range(6 * self.N) if e // 6 != fixed and e != 6 * anchor + 3 + axis]

    def terms(self, R, t, X, lam):
        out = []
        for (a, b), (s, e) in zip(self.pairs, self.offsets):
            out.append(point_terms((R[a], t[a], self.k[a]), (R[b], t[b], self.k[b]), X[s:e], self.ua[s:e], self.ub[s:e], lam))
        return out

    def system(self, terms, blocks=None):
        """S, g, diag U over all views, the cost, the points that did not factor, the pairs' costs; ``blocks``: the pairs'
        sums where they are not ``pair_block`` of the terms"""
        n6 = 6 * self.N
        S, g, dU, cost, bad, pair_cost = np.zeros((n6, n6)), np.zeros(n6), np.zeros(n6), 0.0, 0, []
        for p, ((a, b), o) in enumerate(zip(self.pairs, terms)):
            blk = pair_block(o) if blocks is None else blocks[p]
            sa, sb = slice(6 * a, 6 * a + 6), slice(6 * b, 6 * b + 6)
            S[sa, sa] += blk["aa"]
            S[sb, sb] += blk["bb"]
            S[sb, sa] += blk["ba"]
            S[sa, sb] += blk["ba"].T
            g[sa] += blk["ga"]
            g[sb] += blk["gb"]
            dU[sa] += blk["da"]
            dU[sb] += blk["db"]
            cost += blk["cost"]
            bad += blk["bad"]
            pair_cost.append(blk["cost"])
        return S, g, dU, cost, bad, pair_cost

    def reduced(self, S, g, dU, lam, R, t):
        """the kept rows of M^T (S + lam diag U) M and of M^T g, and M"""
        A = S + lam * np.diag(dU)
        M = np.eye(6 * self.N)
        s = slice(6 * self.anchor, 6 * self.anchor + 6)
        M[s, s] = anchor_matrix(R[self.anchor], t[self.anchor])
        A, g = M.T @ A @ M, M.T @ g
        return A[np.ix_(self.keep, self.keep)], g[self.keep], M


def shared_step(prob, S, g, dU, lam, R, t):
    """(y, x): the step of every view in its gauge parameters (6 N; zero where held) and x = M y, every view's (w, d); None
    where the damped reduced matrix does not factor or the step is not finite"""
    A, gk, M = prob.reduced(S, g, dU, lam, R, t)
    L, _ = _cholesky(A)
    if L is None:
        return None
    y = _solve(L, -gk)
    if not np.isfinite(y).all():
        return None
    yy = np.zeros(6 * prob.N)
    yy[prob.keep] = y
    return yy, M @ yy


def candidate_poses(prob, R, t, yy):
    """every view's candidate: R' = exp([w]x) R, t' = t + d; the anchor's c' = c + e, t' = -R' c'"""
    R2, t2 = R.copy(), t.copy()
    for v in range(prob.N):
        w = yy[6 * v:6 * v + 6]
        R2[v] = rotate_left(w[:3], R[v])
        if v == prob.anchor:
            c2v = -(R[v].T @ t[v]) + w[3:]
            t2[v] = -(R2[v] @ c2v)
        else:
            t2[v] = t[v] + w[3:]
    return R2, t2


def point_steps(o, da, db):
    """dX (n, 3) of one pair's points from its terms and the (w, d) steps of its two views"""
    n = len(o["y"])
    sa, sb = np.zeros((n, 3)), np.zeros((n, 3))
    for p in range(6):
        sa, sb = sa + o["Za"][:, :, p] * da[p], sb + o["Zb"][:, :, p] * db[p]
    r = -(o["y"] + (sa + sb))
    l10, l20, l21 = o["L"]
    i0, i1, i2 = o["il"]
    d2 = r[:, 2] * i2
    d1 = (r[:, 1] - l21 * d2) * i1
    d0 = (r[:, 0] - l10 * d1 - l20 * d2) * i0
    return np.stack([d0, d1, d2], 1)


def candidate(prob, R, t, X, terms, yy, x, steps=point_steps):
    """the candidate of one evaluation: dict(R2, t2, X2, c2 (infinite where a point lies behind a view), step, norm (the
    squared sizes lm_small compares), pairs: per pair (cost, |dX|^2, |X|^2, bad) with bad the points behind a view)"""
    R2, t2 = candidate_poses(prob, R, t, yy)
    X2 = X.copy()
    c2, step, norm, behind, pairs = 0.0, (x * x).sum(), sum(3.0 + (t[v] * t[v]).sum() for v in range(prob.N)), False, []
    for (a, b), (s, e), o in zip(prob.pairs, prob.offsets, terms):
        d = steps(o, x[6 * a:6 * a + 6], x[6 * b:6 * b + 6])
        X2[s:e] = X[s:e] + d
        za, ra = observe(R2[a], t2[a], prob.k[a], X2[s:e], prob.ua[s:e], terms=False)
        zb, rb = observe(R2[b], t2[b], prob.k[b], X2[s:e], prob.ub[s:e], terms=False)
        cc = (ra[:, 0] * ra[:, 0] + ra[:, 1] * ra[:, 1]) + (rb[:, 0] * rb[:, 0] + rb[:, 1] * rb[:, 1])
        bad = (za <= 0) | (zb <= 0) | ~np.isfinite(cc)
        behind = behind or bool(bad.any())
        pairs.append((cc.sum(), (d * d).sum(), (X[s:e] * X[s:e]).sum(), int(bad.sum())))
        c2 += pairs[-1][0]
        step += pairs[-1][1]
        norm += pairs[-1][2]
    if behind:
        c2 = np.inf
    return dict(R2=R2, t2=t2, X2=X2, c2=c2, step=step, norm=norm, pairs=pairs)


def better(c2, c):
    """lm_better: a lower cost, or one within the rounding of the sums"""
    return bool(c2 < c or c2 - c <= COST_RESOLUTION * c)


def final_stage(prob, R, t, X):
    """the undamped stage: (cost, points that did not factor, the pairs' costs, the smallest pivot of the kept reduced
    matrix scaled to a unit diagonal, its factor or None)"""
    terms = prob.terms(R, t, X, 0.0)
    S, g, dU, cost, bad, pair_cost = prob.system(terms)
    A, _, _ = prob.reduced(S, g, dU, 0.0, R, t)
    with np.errstate(all="ignore"):
        s = 1.0 / np.sqrt(np.diag(A))
        L, pivot = _cholesky(A * s[:, None] * s[None, :])
    return cost, bad, pair_cost, pivot, L


def depths(prob, R, t, X):
    out = []
    for (a, b), (s0, e0) in zip(prob.pairs, prob.offsets):
        out.append((observe(R[a], t[a], prob.k[a], X[s0:e0], prob.ua[s0:e0], terms=False)[0],
                    observe(R[b], t[b], prob.k[b], X[s0:e0], prob.ub[s0:e0], terms=False)[0]))
    return out


def pair_errors(pair_cost, used_counts):
    with np.errstate(all="ignore"):
        return np.array([np.sqrt(c / (2.0 * n)) if n else np.nan for c, n in zip(pair_cost, used_counts)])


def solve(K, T, pairs, uvs_a, uvs_b, counts, fixed_view=0, threshold=None):
    """what ``bundle_adjust_pairs`` returns, with ``start`` (M, 3), ``rig_status`` (0 / 3) and ``min_pivot`` besides; nothing is
    raised for a singular problem (``rig_status`` says it), a view with too few observations raises as the product does"""
    K, T = np.asarray(K, np.float64), np.asarray(T, np.float64)
    pairs = [tuple(int(v) for v in p) for p in pairs]
    counts = [int(c) for c in counts]
    uvs_a, uvs_b = np.asarray(uvs_a).astype(np.float64), np.asarray(uvs_b).astype(np.float64)
    N = len(K)
    R, t = poses_from_T(T)
    anchor, axis = gauge(T, fixed_view)
    X0, status = start(K, R, t, pairs, uvs_a, uvs_b, counts, threshold)
    used = status == 0
    bounds = np.concatenate([[0], np.cumsum(counts)])
    used_counts = [int(used[bounds[p]:bounds[p + 1]].sum()) for p in range(len(pairs))]
    obs = np.zeros(N, int)
    for (a, b), n in zip(pairs, used_counts):
        obs[a] += n
        obs[b] += n
    for v in range(N):
        if obs[v] < MIN_OBSERVATIONS:
            raise ValueError("view %d is left with %d used observations (at least %d are needed)" % (v, obs[v], MIN_OBSERVATIONS))
    ub = np.concatenate([[0], np.cumsum(used_counts)])
    prob = Problem(K, R, t, pairs, uvs_a[used], uvs_b[used], [(ub[p], ub[p + 1]) for p in range(len(pairs))], fixed_view, anchor, axis)
    X = X0[used].copy()
    lam, evals, its, stopped, cost0 = 1e-3, 0, 0, False, None
    while evals < MAX_EVALUATIONS and not stopped:
        evals += 1
        terms = prob.terms(R, t, X, lam)
        S, g, dU, c, bad, _ = prob.system(terms)
        cost0 = c if cost0 is None else cost0
        taken = small = False
        step = shared_step(prob, S, g, dU, lam, R, t) if bad == 0 else None
        if step is not None:
            cand = candidate(prob, R, t, X, terms, *step)
            small = np.sqrt(cand["step"]) < EPS * (np.sqrt(cand["norm"]) + EPS)
            taken = better(cand["c2"], c)
            if taken:
                R, t, X, its = cand["R2"], cand["t2"], cand["X2"], its + 1
        lam = lam * 0.1 if taken else lam * 10.0
        stopped = bool(small or lam < 1e-12 or lam > 1e12)
    cost, bad, pair_cost, pivot, L = final_stage(prob, R, t, X)
    good = L is not None and bad == 0 and pivot >= SINGULAR_PIVOT and np.isfinite(cost) and stopped
    points = np.full((len(status), 3), np.nan)
    points[used] = X
    Tout = T_from_poses(R, t)
    Tout[fixed_view] = T[fixed_view]
    n_used = int(used.sum())
    return dict(T=Tout, points=points, status=status, retval=float(np.sqrt(cost / (2.0 * n_used))), cost0=float(cost0), cost=float(cost),
                pair_error=pair_errors(pair_cost, used_counts), iterations=its, evaluations=evals, anchor=(anchor, axis), start=X0,
                rig_status=0 if good else 3, min_pivot=pivot, depths=depths(prob, R, t, X), used_counts=used_counts)


def _aligned(T, T_true):
    """the poses ``T`` after the similarity that lays view 0 on view 0 of ``T_true`` and makes the mean distance of the
    centres from view 0's equal"""
    T, T_true = np.asarray(T, np.float64), np.asarray(T_true, np.float64)
    A = T_true[0] @ np.linalg.inv(T[0])
    moved = np.array([A @ Tk for Tk in T])
    c, ct = moved[:, :3, 3], T_true[:, :3, 3]
    scale = np.linalg.norm(ct - ct[0], axis=1).sum() / np.linalg.norm(c - c[0], axis=1).sum()
    moved[:, :3, 3] = c[0] + (c - c[0]) * scale
    return moved, T_true


def pose_distance(T, T_true):
    """largest |T_k - T_true_k|_F over the views after that alignment: rotation (as a chord) and centre in one number"""
    moved, T_true = _aligned(T, T_true)
    return float(np.linalg.norm(moved - T_true, axis=(1, 2)).max())


def pose_errors(T, T_true):
    """(largest rotation angle, largest centre distance) between two sets of camera-to-world poses after that alignment"""
    moved, T_true = _aligned(T, T_true)
    c, ct = moved[:, :3, 3], T_true[:, :3, 3]
    # the angle from the chord |R - R_true|_F = 2 sqrt(2) sin(angle / 2): linear in a small error, also where a rotation is
    # orthonormal to float32 only (arccos of the trace would turn 1e-8 of that into 1e-4 rad)
    chord = np.linalg.norm(moved[:, :3, :3] - T_true[:, :3, :3], axis=(1, 2)).max()
    return float(2 * np.arcsin(min(1.0, chord / (2 * np.sqrt(2))))), float(np.linalg.norm(c - ct, axis=1).max())
