#!/usr/bin/env python3
"""Writes tests/golden/bundle_stage_exact.npz and tests/golden/bundle_stage_tolerance.json: the exact stage-by-stage
reference of the bundle adjustment and the bounds measured against it.

DEVELOPMENT MACHINE ONLY (it needs mpmath; the GPU tests read the two files and nothing else).
    python tests/golden/make_bundle_stage_golden.py [--only-tolerance]

Per case of tests/bundle_stage_cases.py the fixture holds ``<case>/in/*`` -- K, the start poses, the pairs, the rows and
their counts, the fixed view, lambda, the evaluation point of every used match, and the status and source rows the
restatement's start gives: everything a call of the stage entry points is rebuilt from -- and ``<case>/exact/*``, what
tests/bundle_stage_exact.py computes from those inputs in mpmath and rounds to float64 once (the scales of the sums, which
are yardsticks only, as float32).  The 16385-match case keeps float32 rows and a float32 evaluation point, and of the exact
numbers the pairs' blocks, the state's numbers and ``dX`` of the 32 points ``MANY_NAMED``; its generation takes a few
minutes on one core and runs on all of them.  A case whose pairs are one chunk each holds the chunks' sums once, as the
pairs'.  The archive is written with fixed time stamps, so the same inputs give the same bytes.  The tolerance file is the restatement's error against this fixture (tests/bundle_stage_tolerance.py), never
anything a kernel gave."""
import io
import json
import multiprocessing
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import bundle_stage_cases as cases  # noqa: E402
import bundle_stage_tolerance as tolerance  # noqa: E402


def save(path, arrays):
    """np.savez_compressed with the members in the given order and a fixed time stamp: the same arrays, the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)


def write_fixture():
    import bundle_stage_exact as exact
    out = {}
    with multiprocessing.Pool() as pool:
        for name in cases.NAMES:
            began = time.time()
            c = cases.case(name)
            many = name == cases.MANY
            want = exact.evaluate(c, pool)
            if many:
                want["dX_rows"] = np.array(cases.MANY_NAMED, np.int64)
                want["dX"] = want["dX"][want["dX_rows"]]
            for k in cases.INPUT_KEYS:
                out["%s/in/%s" % (name, k)] = c[k].astype(np.float32) if many and k == "X" else c[k]
            if max(cases.used_counts(c)) <= exact.CHUNK:  # every pair is one chunk: the chunks' sums are the pairs'
                assert all(np.array_equal(want.pop(k), want[v]) for k, v in tolerance.SAME_AS_PAIRS.items())
            for k, v in want.items():
                if not many or k in tolerance.MANY_KEYS:
                    out["%s/exact/%s" % (name, k)] = v
            print("%-24s %6.1f s  cost %.6g -> %.6g (%s), pivot %.3g" % (name, time.time() - began, want["cost"], want["cand_cost"],
                                                                         "taken" if want["accept"] else "rejected", want["pivot"]), flush=True)
    save(tolerance.FIXTURE, out)
    print("wrote %s (%d bytes, %d arrays)" % (os.path.relpath(tolerance.FIXTURE, ROOT), os.path.getsize(tolerance.FIXTURE), len(out)))


def write_tolerance():
    m = tolerance.measure()
    m["cases"] = {name: tolerance.conditions(c, want) for name, (c, want) in tolerance.fixture().items()}
    with open(tolerance.PATH, "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in sorted(m["bound"]):
        print("%-12s measured %.3g  bound %.3g%s" % (k, m["measured"][k], m["bound"][k], "" if m["bound"][k] < m["cap"] else "   ABOVE THE CAP"))
    assert all(b < m["cap"] for b in m["bound"].values()), "a bound above the cap: the case is ill chosen"


if __name__ == "__main__":
    if "--only-tolerance" not in sys.argv:
        write_fixture()
    write_tolerance()
