#!/usr/bin/env python3
"""Writes tests/golden/pnp_start_exact.npz and tests/golden/pnp_start_tolerance.json: the exact reference of the start
stage (``camd_pnp_init``, ``camd_calib_homography``) and the bounds measured against it.

DEVELOPMENT MACHINE ONLY (it needs mpmath; the GPU tests read the two files and nothing else).
    python tests/golden/make_pnp_start_golden.py [--only-tolerance]

The fixture holds five arrays, the cases of tests/pnp_start_cases.py one after the other in the order of its ``NAMES``
(their sizes are its ``SPEC``): ``obj`` -- every case's object rows, float32 values; ``uv_noisy`` (float32 values, a
detector's) and ``uv_exact`` (float64, every bit of the projection) -- the image rows of every frame; ``camera`` -- per case
K (9), the plane's rotation (9) and D padded to 14: everything a call of the two entry points is rebuilt from; and
``exact`` -- per frame what tests/pnp_start_exact.py computes from those inputs in mpmath and rounds to float64 once: G (H
or P, unit Frobenius norm, its largest entry positive; 12 places, NaN behind H's 9), the pose (12 doubles; NaN for a
homography case) and lambda1, lambda2, trace M.  The file is written without a time stamp, so that the same inputs give
the same bytes.  The tolerance file is the restatement's error against this fixture (tests/pnp_start_tolerance.py), never
anything a kernel gave."""
import io
import json
import multiprocessing
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import pnp_start_cases as cases  # noqa: E402
import pnp_start_tolerance as tolerance  # noqa: E402


def write_fixture():
    import pnp_start_exact as exact
    rows = {k: [] for k in tolerance.ARRAYS}
    with multiprocessing.Pool() as pool:
        for name in cases.NAMES:
            c = cases.case(name)
            want = exact.evaluate(c, pool)
            noisy = cases.SPEC[name][4] != 0
            assert np.array_equal(c["obj"].astype(np.float32), c["obj"]) and (not noisy or np.array_equal(c["uv"].astype(np.float32), c["uv"]))
            rows["obj"].append(c["obj"].astype(np.float32))
            rows["uv_noisy" if noisy else "uv_exact"].append(c["uv"].reshape(-1, 2).astype(np.float32 if noisy else np.float64))
            rows["camera"].append(np.concatenate([c["K"].reshape(-1), c["plane"].reshape(-1), c["D"], np.zeros(14 - len(c["D"]))])[None])
            G = np.full((len(c["uv"]), 12), np.nan)
            G[:, :want["G"].shape[1]] = want["G"]
            rows["exact"].append(np.concatenate([G, want["pose"], want["eigen"]], 1))
            kappa = want["eigen"][:, 2] / (want["eigen"][:, 1] - want["eigen"][:, 0])
            print("%-34s %d x %3d points  kappa %.3g .. %.3g" % (name, len(c["uv"]), len(c["obj"]), kappa.min(), kappa.max()))
    out = {k: np.concatenate(v) for k, v in rows.items()}
    with zipfile.ZipFile(tolerance.FIXTURE, "w") as z:  # numpy.savez stamps the time into every member
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, out[k], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print("wrote %s (%d bytes, %d arrays)" % (os.path.relpath(tolerance.FIXTURE, ROOT), os.path.getsize(tolerance.FIXTURE), len(out)))


def write_tolerance():
    m = tolerance.measure()
    with open(tolerance.PATH, "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in sorted(m["bound"]):
        print("%-14s measured %8.3f  bound %8.3f  (x 2^-52 kappa; at the cap %.3g)" % (k, m["measured"][k], m["bound"][k],
                                                                                       m["bound"][k] * m["ulp"] * m["kappa_cap"]))


if __name__ == "__main__":
    if "--only-tolerance" not in sys.argv:
        write_fixture()
    write_tolerance()
