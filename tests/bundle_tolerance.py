"""How far the bundle-adjustment restatement (tests/bundle_ref.py) disagrees with ITSELF when only the order of its sums
changes: every noisy case solved with its pairs, and the rows of every pair, in forward and in reversed order.  The GPU
differs from the restatement in nothing but summation order (a lane per point, butterflies, the two-level sum over a
pair's chunks and the pairs in rising order instead of NumPy's chains), so it is allowed ``FACTOR`` = 8 times the largest
disagreement, as in tests/stereo_calibrate_tolerance.py.  Also recorded: the evaluations every case takes (the cap of
csrc/bundle.hip is more than twice the largest), the restatement's distance from the truth on the noise-free cases, and for
every noisy case the pose error of the start and of the restatement's result against the truth.
``python tests/bundle_tolerance.py`` writes tests/golden/bundle_tolerance.json; tests/test_bundle_cpu.py checks the file
against a fresh measurement.  Nothing here comes from the kernels."""
import json
import os

import numpy as np

import bundle_cases as bc
import bundle_ref as ref

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bundle_tolerance.json")
FACTOR = 8
KEYS = ("T", "points", "retval", "pair_error")


def solve(c, reverse=False, **kw):
    if not reverse:
        return ref.solve(c["K"], c["T0"], c["pairs"], c["uvs_a"], c["uvs_b"], c["counts"], **kw)
    r, perm, order = bc.reverse(c)
    out = ref.solve(r["K"], r["T0"], r["pairs"], r["uvs_a"], r["uvs_b"], r["counts"], **kw)
    back, pback = np.argsort(perm), np.argsort(order)
    return dict(out, points=out["points"][back], status=out["status"][back], start=out["start"][back], pair_error=out["pair_error"][pback])


_SOLVED = {}


def solved(name, noisy):
    """(case, the restatement's result): computed once, shared by every test, never changed"""
    key = (name, bool(noisy))
    if key not in _SOLVED:
        c = bc.case(name, bc.NOISE_SIGMA, bc.NOISY_SEED) if noisy else bc.case(name, 0.0, bc.SEED)
        _SOLVED[key] = (c, solve(c))
    return _SOLVED[key]


def difference(a, b):
    """largest |a - b| of T, the used points, retval and the errors of the pairs with used points"""
    used = a["status"] == 0
    live = np.isfinite(a["pair_error"])
    return dict(T=float(np.abs(a["T"] - b["T"]).max()), points=float(np.abs(a["points"][used] - b["points"][used]).max()),
                retval=float(abs(a["retval"] - b["retval"])), pair_error=float(np.abs(a["pair_error"][live] - b["pair_error"][live]).max()))


def measure():
    worst, evaluations, truth, poses = dict.fromkeys(KEYS, 0.0), {}, dict(rotation=0.0, centre=0.0, retval=0.0), {}
    for name in bc.NAMES:
        c, a = solved(name, True)
        b = solve(c, reverse=True)
        assert a["rig_status"] == 0 and b["rig_status"] == 0 and np.array_equal(a["status"], b["status"]), name
        d = difference(a, b)
        worst = {k: max(worst[k], d[k]) for k in KEYS}
        c0, r0 = solved(name, False)
        assert r0["rig_status"] == 0, name
        rot, centre = ref.pose_errors(r0["T"], c0["T_true"])
        truth = dict(rotation=max(truth["rotation"], rot), centre=max(truth["centre"], centre), retval=max(truth["retval"], r0["retval"]))
        evaluations[name] = max(a["evaluations"], b["evaluations"], r0["evaluations"])
        assert evaluations[name] < ref.MAX_EVALUATIONS / 2, (name, evaluations[name])
        poses[name] = dict(start=list(ref.pose_errors(c["T0"], c["T_true"])), result=list(ref.pose_errors(a["T"], c["T_true"])))
    return dict(disagreement=worst, factor=FACTOR, bound={k: FACTOR * v for k, v in worst.items()}, truth_distance=truth,
                evaluations=evaluations, evaluation_cap=ref.MAX_EVALUATIONS, pose_error=poses, noise_sigma=bc.NOISE_SIGMA)


def load():
    with open(PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    m = measure()
    with open(PATH, "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)
        f.write("\n")
    print(m)
