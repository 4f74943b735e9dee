"""How far the PnP restatement (tests/pnp_ref.py) disagrees with ITSELF when only the order of its sums changes: the noisy
cases solved with the points in forward and in reversed order, from the same start.  The GPU differs from the restatement
in nothing but summation order (lane strides and a butterfly instead of NumPy's pairwise chain), a different class of
order, so it is allowed 8 times the largest disagreement.  ``python tests/pnp_tolerance.py`` writes
tests/golden/pnp_tolerance.json; tests/test_pnp_cpu.py checks the file against a fresh measurement."""
import json
import os

import numpy as np

import pnp_cases as pc
import pnp_ref as ref

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_tolerance.json")
FACTOR = 8
FRAMES = 2


def noisy_cases():
    """[(name, case dict, start poses (frames, 4, 4))]: every case of the grid with sigma = 0.3 px, started from the
    restatement's own direct linear transform"""
    out = []
    for kind, n, ndist in pc.GRID:
        c = pc.case(kind, n, FRAMES, ndist, sigma=pc.NOISE_SIGMA, seed=5)
        planar, plane = ref.plane_of(c["obj"])
        T0 = np.stack([ref.init_pose(c["obj"], uv, c["K"], c["D"], planar, plane) for uv in c["uv"]])
        out.append(("%s-n%d-d%d" % (kind, n, ndist), c, T0))
    return out


def measure():
    dT = dR = 0.0
    for _, c, T0 in noisy_cases():
        for uv, start in zip(c["uv"], T0):
            a = ref.refine(c["obj"], uv, c["K"], c["D"], start)
            b = ref.refine(c["obj"][::-1], uv[::-1], c["K"], c["D"], start)
            assert a["status"] == 0 and b["status"] == 0
            dT = max(dT, float(np.abs(a["T"] - b["T"]).max()))
            dR = max(dR, abs(a["reprojection_error"] - b["reprojection_error"]))
    return dict(T_disagreement=dT, rms_disagreement=dR, factor=FACTOR, T_bound=FACTOR * dT, rms_bound=FACTOR * dR)


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
