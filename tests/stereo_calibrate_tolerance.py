"""How far the stereo-calibration restatement (tests/stereo_calibrate_ref.py) disagrees with ITSELF when only the order of
its sums changes: every noisy case solved with its points and frames in forward and in reversed order.  The GPU differs
from the restatement in nothing but summation order (lane strides, butterflies and the two-level sum over frames instead
of NumPy's chains), so it is allowed 8 times the largest disagreement, as in tests/calibrate_tolerance.py.  Also recorded:
the evaluations every case takes (the cap of csrc/stereo_calibrate.hip is more than twice the largest) and the
restatement's distance from the truth on the noise-free cases.  ``python tests/stereo_calibrate_tolerance.py`` writes
tests/golden/stereo_calibrate_tolerance.json; tests/test_stereo_calibrate_cpu.py checks the file against a fresh
measurement.  Nothing here comes from the kernels."""
import json
import os

import numpy as np

import stereo_calibrate_cases as sc
import stereo_calibrate_ref as ref

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_calibrate_tolerance.json")
FACTOR = 8
KEYS = ("R", "t", "T", "retval", "reprojection_error")
PER_FRAME = ("T", "reprojection_error")


def solve(c, reverse=False, **kw):
    objs, uv1s, uv2s = c["obj"], c["uv1"], c["uv2"]
    if reverse:
        objs, uv1s, uv2s = ([a[::-1] for a in rows[::-1]] for rows in (objs, uv1s, uv2s))
    r = ref.stereo_calibrate(objs, uv1s, uv2s, c["K1"], c["D1"], c["K2"], c["D2"], **kw)
    if reverse:
        r = dict(r, T=r["T"][::-1], reprojection_error=r["reprojection_error"][::-1], status=r["status"][::-1])
    return r


_SOLVED = {}


def solved(name, noisy):
    """(case, the restatement's result): computed once, shared by every test, never changed"""
    key = (name, bool(noisy))
    if key not in _SOLVED:
        c = sc.case(name, sigma=sc.NOISE_SIGMA, seed=sc.NOISY_SEED) if noisy else sc.case(name, seed=sc.SEED)
        _SOLVED[key] = (c, solve(c))
    return _SOLVED[key]


def difference(a, b):
    """largest |a - b| of R, t, T, retval and the per-frame errors over the frames both solved"""
    used = a["status"] == 0
    return {k: float(np.abs(np.asarray(a[k], np.float64)[used if k in PER_FRAME else ...] -
                            np.asarray(b[k], np.float64)[used if k in PER_FRAME else ...]).max()) for k in KEYS}


def truth_distance(c, r):
    used = r["status"] == 0
    return dict(R=float(np.abs(r["R"] - c["R"]).max()), t=float(np.abs(np.ravel(r["t"]) - c["t"]).max()),
                T=float(np.abs(r["T"][used] - c["T"][used]).max()), retval=float(r["retval"]),
                reprojection_error=float(np.asarray(r["reprojection_error"])[used].max()))


def measure():
    worst, truth, evaluations = dict.fromkeys(KEYS, 0.0), dict.fromkeys(KEYS, 0.0), {}
    for name in sc.NAMES:
        c, a = solved(name, True)
        b = solve(c, reverse=True)
        assert a["rig_status"] == 0 and b["rig_status"] == 0 and np.array_equal(a["status"], b["status"]), name
        d = difference(a, b)
        worst = {k: max(worst[k], d[k]) for k in KEYS}
        c0, r0 = solved(name, False)
        assert r0["rig_status"] == 0, name
        t = truth_distance(c0, r0)
        truth = {k: max(truth[k], t[k]) for k in KEYS}
        evaluations[name] = max(a["evaluations"], b["evaluations"], r0["evaluations"])
        assert evaluations[name] < ref.MAX_EVALUATIONS / 2, (name, evaluations[name])
    return dict(disagreement=worst, factor=FACTOR, bound={k: FACTOR * v for k, v in worst.items()}, truth_distance=truth,
                evaluations=evaluations, evaluation_cap=ref.MAX_EVALUATIONS)


def load():
    with open(PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    m = measure()
    with open(PATH, "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)
        f.write("\n")
    print(m)
