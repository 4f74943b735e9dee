"""How far the calibration restatement (tests/calibrate_ref.py) disagrees with ITSELF when only the order of its sums
changes: every noisy case solved with its points and frames in forward and in reversed order.  The GPU differs from the
restatement in nothing but summation order (lane strides and a butterfly instead of NumPy's chains), a different class of
order, so it is allowed 8 times the largest disagreement, as in tests/pnp_tolerance.py.  Also recorded: the evaluations
every case takes (the cap of csrc/calibrate.hip is more than twice the largest) and the restatement's distance from the
truth on the noise-free cases.  ``python tests/calibrate_tolerance.py`` writes tests/golden/calibrate_tolerance.json;
tests/test_calibrate_cpu.py checks the file against a fresh measurement.  Nothing here comes from the kernels."""
import json
import os

import numpy as np

import calibrate_cases as cc
import calibrate_ref as ref

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calibrate_tolerance.json")
FACTOR = 8
PARAMETER_CONDITION = 1e-6  # px: a case whose own forward / reversed fx fy cx cy differ by more is no parity case
KEYS = ("K", "D", "T", "retval", "reprojection_error")


def solve(c, reverse=False):
    objs, uvs = c["obj"], c["uv"]
    if reverse:
        objs, uvs = [o[::-1] for o in objs[::-1]], [u[::-1] for u in uvs[::-1]]
    r = ref.calibrate(objs, uvs, c["xy"], c["flags"], c["K_guess"])
    if reverse:
        r = dict(r, T=r["T"][::-1], reprojection_error=r["reprojection_error"][::-1], status=r["status"][::-1])
    return r


_SOLVED = {}


def solved(name, noisy):
    """(case, the restatement's result): computed once, shared by every test, never changed"""
    key = (name, bool(noisy))
    if key not in _SOLVED:
        c = cc.case(name, sigma=cc.NOISE_SIGMA, seed=cc.NOISY_SEED) if noisy else cc.case(name, seed=cc.SEED)
        _SOLVED[key] = (c, solve(c))
    return _SOLVED[key]


def difference(a, b):
    """largest |a - b| of K, D, T, retval and the per-frame errors over the frames both solved"""
    used = a["status"] == 0
    return {k: float(np.abs(np.asarray(a[k], np.float64)[used if k in ("T", "reprojection_error") else ...] -
                            np.asarray(b[k], np.float64)[used if k in ("T", "reprojection_error") else ...]).max()) for k in KEYS}


def truth_distance(c, r):
    used = r["status"] == 0
    return dict(K=float(np.abs(r["K"] - c["K"]).max()), D=float(np.abs(r["D"].ravel() - c["D"]).max()),
                T=float(np.abs(r["T"][used] - c["T"][used]).max()), retval=float(r["retval"]),
                reprojection_error=float(r["reprojection_error"][used].max()))


def measure():
    worst, truth, evaluations = dict.fromkeys(KEYS, 0.0), dict.fromkeys(KEYS, 0.0), {}
    for name in cc.NAMES:
        c, a = solved(name, True)
        b = solve(c, reverse=True)
        assert a["camera_status"] == 0 and b["camera_status"] == 0 and np.array_equal(a["status"], b["status"]), name
        d = difference(a, b)
        assert np.abs((a["K"] - b["K"])[[0, 1, 0, 1], [0, 1, 2, 2]]).max() < PARAMETER_CONDITION, (name, d)
        worst = {k: max(worst[k], d[k]) for k in KEYS}
        c0, r0 = solved(name, False)
        assert r0["camera_status"] == 0, name
        t = truth_distance(c0, r0)
        truth = {k: max(truth[k], t[k]) for k in KEYS}
        evaluations[name] = max(a["evaluations"], b["evaluations"], r0["evaluations"])
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
