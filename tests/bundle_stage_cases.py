"""Seeded cases of the stage tests of the bundle adjustment (tests/test_bundle_stage_cpu.py,
tests/test_gpu_bundle_stages.py): one evaluation point per case, OFF the minimum, at which ``camd_bundle_start / emit /
step / finish`` are driven stage by stage.  Only DATA lives here, built on ``reconstruction_cases.scene`` as
tests/bundle_cases.py is.

A pair's used matches are pixel centres of view a with where the flow takes them in view b, a seeded choice (in row order)
among those that the restatement's ``start()`` uses under the START poses (status 0: a triangulation sine of at least
``MIN_SINE``, in front of both views).  The start poses are the truth perturbed by ``bundle_cases.perturbed``.  The evaluation
point ``X`` of a used match is the TRUE surface point plus a seeded shift of up to ``shift`` per coordinate, so residuals are
pixels and nothing cancels in the gradients.  Into the pairs ``bad`` names, three more rows are laid -- at the start, in the
middle and at the end -- alternately with a NaN coordinate (status 1) and with the pixel in view b of the point at infinity
of view a's ray (status 2), so that neither the compaction nor ``src`` is the identity.

The used counts lie on the edges of every path: 7 / 64 / 65 around the wavefront, 63 / 255 / 256 / 257 around the chunk of
256, 66 pairs for k_bundle_update's stride of 64, 120 pairs of 16 views for k_bundle_solve at 96 rows, and 64 x 256 + 1
used matches in one pair for k_bundle_pair_sum's stride.  A case that names its gauge takes the first scene seed that
gives it (``scene_seed`` finds it again at once whenever the case is built); the 12 and 16 views are the ones farthest apart
out of a scene of 36 and 64 (``spread_views``), since two views of a random scene that lie close together share no match
that ``start()`` uses.

A case is a dict: name, K (N, 3, 3), T0 (N, 4, 4), pairs (P, 2) int32, counts (P,) int64 rows, uvs_a, uvs_b (M, 2) float64 or
float32, fixed_view, lam, X (U, 3) float64 (float32 values in ``MANY``), and what the restatement's start makes of the rows:
status (M,) int32 and src (U,) int64, the rows of the used matches."""
import numpy as np

import bundle_cases as bc
import bundle_ref as ref
import reconstruction_cases as rc

SEED = 21
LAMBDA = 1e-3
SHIFT = 0.02
BORDERS = [6, 63, 255, 256, 257, 20, 20, 20, 20, 20]
BIG_HW = (160, 208)  # the 48 x 64 image has too few pixels for one pair of 16385 matches


def _spec(views, used, seed, bad=(0,), dtype="f64", fixed=0, lam=LAMBDA, shift=SHIFT, hw=rc.HW, anchor=None, axis=None, pool=0):
    return dict(views=views, used=list(used), seed=seed, bad=tuple(bad), dtype=dtype, fixed=fixed, lam=lam, shift=shift, hw=tuple(hw),
                anchor=anchor, axis=axis, pool=pool)


CASES = {
    "v3-n7-64-65": _spec(3, [7, 64, 65], 1, bad=(0, 1, 2)),
    "v5-borders": _spec(5, BORDERS, 2, bad=(0, 3, 9)),
    "v5-borders-f32-fixed3": _spec(5, BORDERS, 4, bad=(1, 4, 8), dtype="f32", fixed=3, anchor=0),
    "v3-axis0": _spec(3, [8, 9, 10], 1, bad=(1,), axis=0),
    "v3-axis1": _spec(3, [8, 9, 10], 6, bad=(2,), axis=1),
    "v3-axis2": _spec(3, [8, 9, 10], 22, bad=(0,), axis=2),
    "v12-p66": _spec(12, [6] * 66, 1, bad=(0, 33, 65), pool=36),
    "v16-p120": _spec(16, [6] * 120, 1, bad=(0, 64, 119), pool=64),
    # next to no damping and an evaluation point up to 2.46 off the surface, some of it 0.6 before a view: the
    # near-Gauss-Newton step overshoots (cost 1.08e6 -> 1.36e6, the nearest candidate 0.22 before its view; at 2.44 the step
    # is still taken, from 2.50 on a candidate lies behind a view).  With 12 matches a pair the first rejected step, at 2.60,
    # put a candidate 0.013 before a view, where its cost is too ill conditioned for any float64 evaluation: the restatement
    # itself was 1.6e-10 off, above the cap
    "v3-rejected": _spec(3, [40, 40, 40], 1, bad=(1,), lam=1e-9, shift=2.46),
}
MANY = "v3-many-f32"
MANY_CASE = {MANY: _spec(3, [64 * 256 + 1, 8, 8], 1, bad=(0, 2), dtype="f32", hw=BIG_HW)}
MANY_NAMED = [0, 1, 63, 64, 255, 256, 257, 511, 512, 4095, 4096, 8191, 8192, 16127, 16128, 16383, 16384,  # of the big pair
              16385, 16386, 16392, 16393, 16400, 1000, 2000, 3000, 5000, 7000, 9000, 11000, 13000, 15000, 16000]
SMALL = list(CASES)
NAMES = SMALL + [MANY]
REJECTED = "v3-rejected"
AXES = ("v3-axis0", "v3-axis1", "v3-axis2")
SUBSET = ("v5-borders", (0, 4, 9))  # the case of the subset test and the pairs it takes alone
INPUT_KEYS = ("K", "T0", "pairs", "counts", "uvs_a", "uvs_b", "fixed_view", "lam", "X", "status", "src")
SEARCH = 1000
_BUILT = {}


def _start_poses(Ts, seed):
    return bc.perturbed(Ts, np.random.default_rng([SEED, seed, 1]))


def spread_views(Ts, n):
    """n of the scene's views whose centres lie far apart across the optical axis: view 0, then again and again the view
    farthest from those taken (two views closer than about 0.1 share no point at the scene's depth of 3 whose rays meet
    at a sine of MIN_SINE); in rising order"""
    c = np.array([T[:2, 3] for T in Ts])
    taken = [0]
    while len(taken) < n:
        d = np.linalg.norm(c[:, None] - c[None, taken], axis=2).min(1)
        d[taken] = -1.0
        taken.append(int(np.argmax(d)))
    return sorted(taken)


def scene_seed(s):
    """the first scene seed from the case's own whose start poses give the gauge the case names (any, where it names none)"""
    for seed in range(s["seed"], s["seed"] + SEARCH):
        if s["anchor"] is None and s["axis"] is None:
            return seed
        Ts = np.array(rc.poses(s["views"], np.random.default_rng(seed)))
        anchor, axis = ref.gauge(_start_poses(Ts, seed), s["fixed"])
        if (s["anchor"] is None or anchor == s["anchor"]) and (s["axis"] is None or axis == s["axis"]):
            return seed
    raise AssertionError("no scene seed meets the case")


def scene_of(s, seed):
    """(K, true poses, flows keyed by the case's pairs) of the case's views: the scene's, or ``views`` spread ones out of
    a scene of ``pool``"""
    viewds, flowds, Ts = rc.scene(s["pool"] or s["views"], seed, hw=s["hw"])
    views = spread_views(Ts, s["views"]) if s["pool"] else list(range(s["views"]))
    flows = {(i, j): flowds[(a, b)] for i, a in enumerate(views) for j, b in enumerate(views) if i < j}
    return np.array([viewds[v]["K"] for v in views]), np.array([Ts[v] for v in views]), flows


def _far_pixel(K, R, t, a, b, ua):
    """the pixel in view b of the point at infinity of view a's ray through ua, under the start poses"""
    d = R[a].T @ np.array([(ua[0] - K[a][0, 2]) / K[a][0, 0], (ua[1] - K[a][1, 2]) / K[a][1, 1], 1.0])
    p = K[b] @ (R[b] @ d)
    return p[:2] / p[2]


def case(name):
    if name in _BUILT:
        return _BUILT[name]
    s = (MANY_CASE if name == MANY else CASES)[name]
    index = NAMES.index(name)
    seed = scene_seed(s)
    K, Ts, flowds = scene_of(s, seed)
    N = s["views"]
    T0 = _start_poses(Ts, seed)
    R, t = ref.poses_from_T(T0)
    dtype = np.float32 if s["dtype"] == "f32" else np.float64
    rng = np.random.default_rng([SEED, index, 2])
    pairs = bc.all_pairs(N)
    surface = {}
    uas, ubs, truths = [], [], []
    for p, ((a, b), n) in enumerate(zip(pairs, s["used"])):
        if a not in surface:
            surface[a] = rc.surface_points(K[a], Ts[a], s["hw"])
        f = flowds[(a, b)]
        ys, xs = np.nonzero(f["common_fov_mask"])
        ua = np.stack([xs + 0.5, ys + 0.5], 1).astype(np.float64)
        ub = ua + f["flow_abs"][ys, xs].astype(np.float64)
        ua, ub = ua.astype(dtype), ub.astype(dtype)
        _, st = ref.start(K, R, t, [(a, b)], ua, ub, [len(ua)])
        ok = np.flatnonzero(st == 0)
        assert len(ok) >= n, "%s: pair %d has %d matches with a start point, %d are wanted" % (name, p, len(ok), n)
        pick = np.sort(rng.choice(ok, size=n, replace=False))
        ua, ub, truth = ua[pick], ub[pick], surface[a][ys[pick], xs[pick]]
        if p in s["bad"]:  # three rows more: at the start, in the middle, at the end
            kinds = (1, 2, 1) if s["bad"].index(p) % 2 == 0 else (2, 1, 2)
            for at, kind in zip((0, n // 2 + 1, n + 2), kinds):
                row_a = ua[min(at, len(ua) - 1)].astype(np.float64)
                row_b = _far_pixel(K, R, t, a, b, row_a) if kind == 2 else np.array([np.nan, row_a[1]])
                ua, ub = np.insert(ua, at, row_a.astype(dtype), 0), np.insert(ub, at, row_b.astype(dtype), 0)
                truth = np.insert(truth, at, np.nan, 0)
        uas.append(ua), ubs.append(ub), truths.append(truth)
    uvs_a, uvs_b, truth = np.concatenate(uas), np.concatenate(ubs), np.concatenate(truths)
    counts = np.array([len(u) for u in uas], np.int64)
    _, status = ref.start(K, R, t, pairs, uvs_a, uvs_b, counts)
    src = np.flatnonzero(status == 0).astype(np.int64)
    X = truth[src] + rng.uniform(-s["shift"], s["shift"], (len(src), 3))
    if name == MANY:
        X = X.astype(np.float32).astype(np.float64)  # (stored as float32)
    assert np.isfinite(X).all() and len(src) == sum(s["used"])
    _BUILT[name] = dict(name=name, K=K, T0=T0, pairs=np.array(pairs, np.int32), counts=counts, uvs_a=uvs_a, uvs_b=uvs_b,
                        fixed_view=np.array(s["fixed"], np.int64), lam=np.array(s["lam"]), X=X, status=status, src=src)
    return _BUILT[name]


def used_counts(c):
    bounds = np.concatenate([[0], np.cumsum(c["counts"])])
    return [int((c["status"][bounds[p]:bounds[p + 1]] == 0).sum()) for p in range(len(c["counts"]))]


def offsets(c):
    """[(first, end)] of every pair among the used points"""
    ub = np.concatenate([[0], np.cumsum(used_counts(c))])
    return [(int(ub[p]), int(ub[p + 1])) for p in range(len(c["counts"]))]


def reverse(c):
    """the same case with its pairs, and the rows of every pair, in reversed order -> (case, the used points' permutation,
    the pairs' permutation) with reversed[i] = original[perm[i]]"""
    r, perm, order = bc.reverse(c)
    used = c["status"] == 0
    rank = np.cumsum(used) - 1  # row -> its place among the used points
    uperm = rank[perm[used[perm]]]
    return dict(r, X=c["X"][uperm], status=c["status"][perm], src=np.flatnonzero(c["status"][perm] == 0).astype(np.int64)), uperm, order


def subproblem(c, p):
    """a 3-view problem of its own around pair p of the case: the pair's two views and a third, their three pairs with
    their rows and evaluation points, the same start poses and lambda -> (case, the pair's index in it)"""
    a, b = (int(v) for v in c["pairs"][p])
    third = next(v for v in range(len(c["K"])) if v not in (a, b))
    views = sorted((a, b, third))
    at = {v: i for i, v in enumerate(views)}
    order = [q for q, (x, y) in enumerate(c["pairs"]) if int(x) in at and int(y) in at]
    bounds = np.concatenate([[0], np.cumsum(c["counts"])])
    rows = np.concatenate([np.arange(bounds[q], bounds[q + 1]) for q in order])
    off = offsets(c)
    used = np.concatenate([np.arange(*off[q]) for q in order])
    status = c["status"][rows]
    fixed = int(c["fixed_view"])
    sub = dict(c, K=c["K"][views], T0=c["T0"][views], pairs=np.array([(at[int(c["pairs"][q][0])], at[int(c["pairs"][q][1])]) for q in order], np.int32),
               counts=c["counts"][order], uvs_a=c["uvs_a"][rows], uvs_b=c["uvs_b"][rows], X=c["X"][used], status=status,
               src=np.flatnonzero(status == 0).astype(np.int64), fixed_view=np.array(at.get(fixed, 0), np.int64))
    return sub, order.index(p)
