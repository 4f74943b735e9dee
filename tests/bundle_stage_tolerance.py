"""How one evaluation of the bundle adjustment is compared with the exact fixture, and how far the float64 NumPy
restatement (tests/bundle_ref.py) lies from it.  No mpmath here: the exact numbers are read from
tests/golden/bundle_stage_exact.npz (tests/golden/make_bundle_stage_golden.py writes it).

``errors(got, want)`` is the one comparison -- of the restatement for the measurement, of its mutations for the sensitivity
test, of the GPU's stages in tests/test_gpu_bundle_stages.py.  Its yardsticks:
    sum/aa bb ba ga gb da db cost   |value - exact| / s per entry of a chunk's or a pair's 103 sums, s the same sum over the
                       absolute values of its products (the fixture's scales); an entry whose s is 0 has to be 0
    step               every view's (w, d): relative to |step| over all views
    pose               every view's candidate R, t: to 1
    dX                 Xc - X: relative to the case's RMS |dX|, so that the size of X does not hide an error in a small step
    cost, cand_cost, eval/cost, eval/step2, eval/norm2 (a chunk's and a pair's candidate cost, |dX|^2, |X|^2), pair_error,
    depth              relative to themselves
    pivot              absolute: it is a pivot of a matrix with a unit diagonal
``measure()`` takes the restatement's errors over every case with the points of every pair, and the pairs, in forward and
in reversed order.  A GPU stage differs from the restatement only in the order of the same float64 arithmetic (a lane per
point, butterflies, the two-level sum, contraction, its own Cholesky), so it is allowed ``FACTOR`` = 8 times the largest error
found, as in tests/solver_stage_tolerance.py; a quantity the restatement happens to get exactly is allowed 8 roundings of
2^-52.  Every bound has to stay below ``CAP`` = 1e-10: a structural error is of order 1 on these scales.  Nothing here comes
from the kernels."""
import json
import os

import numpy as np

import bundle_ref as ref
import bundle_stage_cases as cases
from calibrating_amd import bundle

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "bundle_stage_exact.npz")
PATH = os.path.join(HERE, "golden", "bundle_stage_tolerance.json")
FACTOR, CAP, ULP = 8, 1e-10, 2.0 ** -52
BLOCKS = dict(aa=slice(0, 21), bb=slice(21, 42), ba=slice(42, 78), ga=slice(78, 84), gb=slice(84, 90), da=slice(90, 96),
              db=slice(96, 102), cost=slice(102, 103))
SUMS = tuple("sum/" + k for k in BLOCKS)
EVALUATION = ("step", "pose", "dX", "cand_cost", "eval/cost", "eval/step2", "eval/norm2")
FINAL = ("cost", "pivot", "pair_error", "depth")
KINDS = SUMS + EVALUATION + FINAL
MANY_WHICH = EVALUATION + ("cost", "pivot", "pair_error")  # (the 16385-match case keeps no depths)
SAME_AS_PAIRS = dict(partials="pair_blocks", partials_scale="pair_scale", eval_partials="eval_blocks")
MANY_KEYS = ("pair_blocks", "pair_scale", "step", "cand", "dX", "dX_rows", "dX_rms", "eval_blocks", "cost", "cand_cost", "accept", "pivot",
             "pair_error", "points_definite", "reduced_definite", "pivot_definite", "behind")


def block_errors(values, exact, scale):
    """per block the largest |value - exact| / scale over rows of 103 sums; infinite where a sum of zeros is not 0"""
    values, exact, scale = (np.asarray(a, np.float64)[..., :103].reshape(-1, 103) for a in (values, exact, scale))
    with np.errstate(all="ignore"):
        e = np.where(scale > 0, np.abs(values - exact) / scale, np.where(values == exact, 0.0, np.inf))
    e = np.where(np.isfinite(values), e, np.inf)
    return {"sum/" + k: float(e[:, s].max()) for k, s in BLOCKS.items()}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        e = np.max(np.abs(a - b) / np.abs(b))
    return float(e) if np.isfinite(e) else np.inf


def errors(got, want, which=EVALUATION + FINAL, sums=True):
    """name -> error of ``got`` against the exact ``want`` (the docstring's yardsticks): the sums that both hold (chunks and
    pairs together), then the quantities ``which`` names.  ``got["dX"]`` holds the rows ``want["dX_rows"]`` names."""
    out = {}
    if sums:
        for k, s in (("partials", "partials_scale"), ("pair_blocks", "pair_scale")):
            if k in got and k in want:
                out = {n: max(v, out.get(n, 0.0)) for n, v in block_errors(got[k], want[k], want[s]).items()}
    for k in which:
        if k == "step":
            e = float(np.abs(got["step"] - want["step"]).max() / np.sqrt((want["step"] ** 2).sum()))
        elif k == "pose":
            e = float(np.abs(got["cand"] - want["cand"]).max())
        elif k == "dX":
            e = float(np.abs(got["dX"] - want["dX"]).max() / float(want["dX_rms"]))
        elif k.startswith("eval/"):
            at = ("eval/cost", "eval/step2", "eval/norm2").index(k)
            e = max(_rel(got[n][:, at], want[n][:, at]) for n in ("eval_partials", "eval_blocks") if n in got and n in want)
        elif k == "pivot":
            e = abs(float(got["pivot"]) - float(want["pivot"]))
        elif k == "depth":
            e = max(_rel(got[n], want[n]) for n in ("depth_a", "depth_b"))
        else:
            e = _rel(got[k], want[k])
        out[k] = e if np.isfinite(e) else np.inf
    return out


# ---- the restatement, stage by stage ------------------------------------------------------------------------------
def problem(c):
    """(bundle_ref.Problem, R, t) of a case at its start poses"""
    R, t = ref.poses_from_T(c["T0"])
    fixed = int(c["fixed_view"])
    anchor, axis = ref.gauge(c["T0"], fixed)
    used = c["status"] == 0
    pairs = [tuple(int(v) for v in p) for p in c["pairs"]]
    prob = ref.Problem(c["K"], R, t, pairs, c["uvs_a"][used].astype(np.float64), c["uvs_b"][used].astype(np.float64), cases.offsets(c),
                       fixed, anchor, axis)
    return prob, R, t


def pack(blk):
    """a pair_block of the restatement in the kernels' packing (103 sums)"""
    lower = np.tril_indices(6)
    return np.concatenate([blk["aa"][lower], blk["bb"][lower], blk["ba"].reshape(-1), blk["ga"], blk["gb"], blk["da"], blk["db"], [blk["cost"]]])


def chunk_rows(c):
    """(the product's chunk table, the pairs' chunk ranges) of a case"""
    return bundle._chunks(cases.used_counts(c))


def _slice_terms(o, s):
    return {k: (tuple(x[s] for x in v) if isinstance(v, tuple) else v[s]) for k, v in o.items()}


def stages(c, partials=True, mutate=None):
    """The restatement's float64 evaluation of a case, in the layout of the exact fixture.  ``mutate`` (the sensitivity
    test's planted mistakes): point_lam / view_lam (the lambda of the points' V / of the views' diag U), problem(prob),
    blocks(terms, blocks, chunk_blocks) -> the pairs' sums, candidate_terms(terms, undamped terms) -> the terms the points'
    steps are taken from, after(out, prob, R, t, x)."""
    m = mutate or {}
    prob, R, t = problem(c)
    if "problem" in m:
        m["problem"](prob)
    X, lam, N = c["X"], float(c["lam"]), prob.N
    terms = prob.terms(R, t, X, m.get("point_lam", lam))
    blocks = [ref.pair_block(o) for o in terms]
    table, ranges = chunk_rows(c)
    out = {}
    if partials or "blocks" in m:
        chunk_blocks = [ref.pair_block(_slice_terms(terms[p], slice(s - prob.offsets[p][0], s - prob.offsets[p][0] + n))) for p, s, n, _ in table]
        out["partials"] = np.stack([pack(b) for b in chunk_blocks])
        if "blocks" in m:
            blocks = m["blocks"](terms, blocks, [chunk_blocks[int(ranges[p]):int(ranges[p + 1])] for p in range(len(blocks))])
    out["pair_blocks"] = np.stack([pack(b) for b in blocks])
    S, g, dU, cost, bad, pair_cost = prob.system(terms, blocks)
    assert bad == 0
    step = ref.shared_step(prob, S, g, dU, m.get("view_lam", lam), R, t)
    if step is None:  # mutated sums without a definite system: the sums alone are left to compare
        assert m
        return out
    yy, x = step
    cterms = m["candidate_terms"](terms, prob.terms(R, t, X, 0.0)) if "candidate_terms" in m else terms
    cand = ref.candidate(prob, R, t, X, cterms, yy, x)
    R2, t2, X2 = cand["R2"], cand["t2"], cand["X2"]
    per_point = []
    for (a, b), (s, e) in zip(prob.pairs, prob.offsets):
        _, ra = ref.observe(R2[a], t2[a], prob.k[a], X2[s:e], prob.ua[s:e], terms=False)
        _, rb = ref.observe(R2[b], t2[b], prob.k[b], X2[s:e], prob.ub[s:e], terms=False)
        d = X2[s:e] - X[s:e]
        per_point.append(np.stack([(ra[:, 0] * ra[:, 0] + ra[:, 1] * ra[:, 1]) + (rb[:, 0] * rb[:, 0] + rb[:, 1] * rb[:, 1]),
                                   (d * d).sum(1), (X[s:e] * X[s:e]).sum(1)], 1))
    per_point = np.concatenate(per_point)
    cost0, bad0, pair_cost0, pivot, L0 = ref.final_stage(prob, R, t, X)
    z = ref.depths(prob, R, t, X)
    out.update(step=x.reshape(N, 6), cand=np.concatenate([R2.reshape(N, 9), t2], 1), dX=X2 - X,
               eval_partials=np.stack([per_point[s:s + n].sum(0) for _, s, n, _ in table]), eval_blocks=np.array([p[:3] for p in cand["pairs"]]),
               cost=np.float64(cost), cand_cost=np.float64(cand["c2"]), accept=ref.better(cand["c2"], cost), pivot=np.float64(pivot),
               pair_error=ref.pair_errors(pair_cost0, cases.used_counts(c)), depth_a=np.concatenate([a for a, _ in z]),
               depth_b=np.concatenate([b for _, b in z]), final_cost=np.float64(cost0))
    if "after" in m:
        m["after"](out, prob, R, t, x)
    return out


def restated(c, reverse=False, mutate=None):
    """``stages`` of the case, or of the case with its pairs and the rows of every pair reversed, laid back in the case's
    order (the chunks of a reversed pair are other chunks: their sums are left out)"""
    if not reverse:
        return stages(c, mutate=mutate)
    r, uperm, order = cases.reverse(c)
    out = stages(r, partials=False, mutate=mutate)
    uback, pback = np.argsort(uperm), np.argsort(order)
    out.pop("eval_partials")
    for k in ("dX", "depth_a", "depth_b"):
        out[k] = out[k][uback]
    for k in ("pair_blocks", "eval_blocks", "pair_error"):
        out[k] = out[k][pback]
    return out


def named(got, want):
    """``got`` with its dX at the rows the fixture names (the 16385-match case keeps 32 of them)"""
    return dict(got, dX=got["dX"][want["dX_rows"]]) if "dX_rows" in want else got


# ---- the fixture and the measurement --------------------------------------------------------------------------------
_LOADED = {}


def fixture():
    """name -> (case, exact): read once, shared by every test, never changed"""
    if not _LOADED:
        with np.load(FIXTURE) as z:
            for name in cases.NAMES:
                c = {k: z["%s/in/%s" % (name, k)] for k in cases.INPUT_KEYS}
                c.update(name=name, X=c["X"].astype(np.float64))
                head = name + "/exact/"
                want = {k[len(head):]: z[k] for k in z.files if k.startswith(head)}
                if name != cases.MANY:  # (a case whose pairs are one chunk each holds the chunks' sums once, as the pairs')
                    want.update({k: want[v] for k, v in SAME_AS_PAIRS.items() if k not in want})
                for v in list(c.values()) + list(want.values()):
                    if isinstance(v, np.ndarray):
                        v.setflags(write=False)
                _LOADED[name] = (c, want)
    return _LOADED


def conditions(c, want):
    """what the issue asks of a case, from the exact numbers alone"""
    obs = np.zeros(len(c["K"]), np.int64)
    for (a, b), n in zip(c["pairs"], cases.used_counts(c)):
        obs[a] += n
        obs[b] += n
    return dict(cost_change=float((want["cand_cost"] - want["cost"]) / want["cost"]), pivot=float(want["pivot"]),
                definite=bool(want["points_definite"] and want["reduced_definite"] and want["pivot_definite"]), behind=int(want["behind"]),
                observations=int(obs.min()), accept=bool(want["accept"]))


def measure(names=None):
    """the restatement against the exact fixture over every case, forward and reversed -> the tolerance record"""
    worst = {}
    for name, (c, want) in fixture().items():
        if names is not None and name not in names:
            continue
        for reverse in (False, True):
            e = errors(named(restated(c, reverse), want), want, EVALUATION + FINAL if "depth_a" in want else MANY_WHICH)
            worst.update({k: max(worst.get(k, 0.0), v) for k, v in e.items()})
    return dict(measured=worst, factor=FACTOR, cap=CAP, ulp=ULP, bound={k: FACTOR * max(v, ULP) for k, v in worst.items()})


def load():
    with open(PATH) as f:
        return json.load(f)
