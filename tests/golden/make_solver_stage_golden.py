#!/usr/bin/env python3
"""Writes tests/golden/solver_stage_exact.npz and tests/golden/solver_stage_tolerance.json: the exact stage-by-stage
reference of the two joint solvers and the bounds measured against it.

DEVELOPMENT MACHINE ONLY (it needs mpmath; the GPU tests read the two files and nothing else).
    python tests/golden/make_solver_stage_golden.py [--only-tolerance]

Per case of tests/solver_stage_cases.py the fixture holds ``<case>/in/*`` -- the rows, counts, start poses, lambda and the
start K and mask or the start rig and cameras: everything a call of the stage entry points is rebuilt from -- and
``<case>/exact/*``, what tests/solver_stage_exact.py computes from those inputs in mpmath and rounds to float64 once (the
scales of the sums, which are yardsticks only, as float32).  The 4097-frame case keeps float32 rows and start poses, and
of the exact numbers only those of the state: step, candidate rig, costs, pivot; its generation takes a few minutes on
one core and runs on all of them.  The tolerance file is the restatements' error against this fixture
(tests/solver_stage_tolerance.py), never anything a kernel gave."""
import json
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import solver_stage_cases as cases  # noqa: E402
import solver_stage_tolerance as tolerance  # noqa: E402

STATE_ONLY = ("step", "shared", "cost", "cand_cost", "accept", "frames_definite", "reduced_definite", "pivot", "pivot_definite")


def write_fixture():
    import solver_stage_exact as exact
    out = {}
    with multiprocessing.Pool() as pool:
        for name in cases.NAMES:
            began = time.time()
            c = cases.case(name)
            many = name == cases.MANY
            want = exact.evaluate(c, pool, workspace=not many)
            for k in cases.INPUT_KEYS[c["kind"]]:
                out["%s/in/%s" % (name, k)] = c[k].astype(np.float32) if many and k == "poses" else c[k]
            for k, v in want.items():
                if not many or k in STATE_ONLY:
                    out["%s/exact/%s" % (name, k)] = v
            print("%-32s %6.1f s  cost %.6g -> %.6g, pivot %.3g" % (name, time.time() - began, want["cost"], want["cand_cost"], want["pivot"]))
    np.savez_compressed(tolerance.FIXTURE, **out)
    print("wrote %s (%d bytes, %d arrays)" % (os.path.relpath(tolerance.FIXTURE, ROOT), os.path.getsize(tolerance.FIXTURE), len(out)))


def write_tolerance():
    m = tolerance.measure()
    m["cases"] = {name: tolerance.conditions(want) for name, (c, want) in tolerance.fixture().items()}
    with open(tolerance.PATH, "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in sorted(m["bound"]):
        print("%-22s measured %.3g  bound %.3g%s" % (k, m["measured"][k], m["bound"][k], "" if m["bound"][k] < m["cap"] else "   ABOVE THE CAP"))
    assert all(b < m["cap"] for b in m["bound"].values()), "a bound above the cap: the case is ill chosen"


if __name__ == "__main__":
    if "--only-tolerance" not in sys.argv:
        write_fixture()
    write_tolerance()
