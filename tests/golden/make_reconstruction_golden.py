#!/usr/bin/env python3
"""Runs the REFERENCE's own ReconstructionExtrinsics on tests/reconstruction_cases.py and writes
tests/golden/reference_reconstruction.npz.

BUILD CONTAINER ONLY (it needs the reference checkout, which does not travel to the GPU box; only the .npz does).
    python tests/golden/make_reconstruction_golden.py

What is executed.  The reference package is imported from where it lies, unmodified, through
``make_reference_golden.import_reference()`` (``boxx.mg`` a no-op, as in make_epipolar_golden.py), and its own class runs on
the flows of every case.  This path is NumPy only.  Nothing of the reference's text goes into the repository.

Per case the script stores the seed it took, ``seed3`` / ``propagate_path`` / every triple's ``idx_sorted``, match counts and
index vectors (SHA-256 + thinned copy), which triples the reference re-rooted, and per view ``T_re`` and ``uvzis`` (row count,
SHA-256 of the [u, v, view] columns, every Z_STEP-th depth).  Where the reference raises, what it raises.

Generator conditions, asserted here; a seed that violates one is passed over and the next is tried:
    the reference succeeds / raises what the case is there for; ``rerooted`` does re-root
    no triple's match count (all planned triples, counted by the restatement tests/epipolar_ref.py) lies within 10 of
    MIN_MATCHED_PIXELS, and no two triples of a case tie in it: no order rests on a tie
Allowances: ``sens_T_re`` / ``sens_z`` = the largest change of the reference's own T_re / depth column over SENS_RUNS reruns with
every coordinate of set2ds moved by one ulp; ``ref_rot_error`` = its rotation error against the generator's true poses."""
import os
import sys
from itertools import combinations

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_reference_golden as mrg  # noqa: E402
import reference_cases as rc  # noqa: E402
import epipolar_cases as ec  # noqa: E402
import epipolar_ref as er  # noqa: E402
import reconstruction_cases as rcc  # noqa: E402
from make_epipolar_golden import put  # noqa: E402

MIN_MATCHED_PIXELS = 10
Z_STEP = 8


def planned_counts(viewds, set2ds):
    """{set3: (first idx_sorted, not_include_uvsn, shared cells)} of every triple with at most one empty pair."""
    out = {}
    for set3 in map(frozenset, combinations(viewds, 3)):
        ijk = tuple(sorted(set3))
        n = {idx: len(set2ds.get(set3.difference({idx}), {"uvs_i": ""})["uvs_i"]) for idx in ijk}
        if list(n.values()).count(0) >= 2:
            continue
        ii, jj, kk = idx_sorted = sorted(ijk, key=lambda x: n[x])
        mains = [set2ds[frozenset((o, ii))]["uvs_" + "ij"[tuple(sorted((o, ii))).index(ii)]] for o in (jj, kk)]
        got = er.matching(mains[0], mains[1], 1, 0)
        out[set3] = (idx_sorted, n, len(got["uv_match_idx1"]))
    return out


def conditions(planned):
    counts = [c for _, _, c in planned.values()]
    return len(set(counts)) == len(counts) and all(abs(c - MIN_MATCHED_PIXELS) > 10 for c in counts)


def run(reg, viewds, set2ds):
    return reg.ReconstructionExtrinsics(rcc.fresh(viewds), set2ds={k: dict(v) for k, v in set2ds.items()})


def nudged_set2ds(set2ds, rng):
    return {k: {kk: ec.nudged(vv, rng) for kk, vv in v.items()} for k, v in set2ds.items()}


def main():
    mrg.import_reference()
    sys.modules["boxx"].mg = lambda *a, **k: None
    from calibrating import reconstruction_epipolar_geometry as reg
    out = {}
    for name, c in rcc.CASES.items():
        for seed in range(c["seed"], c["seed"] + rcc.SEED_SEARCH):
            viewds, flowds, Ts = rcc.case(name, seed)
            set2ds = reg.ReconstructionExtrinsics.build_set2ds_by_flowds(viewds, flowds)
            planned = planned_counts(viewds, set2ds)
            if not conditions(planned):
                continue
            try:
                re, raised = run(reg, viewds, set2ds), None
            except Exception as e:  # what the reference does with this input is part of the record
                re, raised = None, "%s: %s" % (type(e).__name__, e)
            if name in rcc.REFERENCE_SUCCEEDS:
                if re is None:
                    continue
                rerooted = sorted(rcc.triple_name(s) for s, d in re.set3ds.items() if d["idx_sorted"] != planned[s][0])
                if bool(rerooted) != bool(c.get("rerooted")):
                    continue
            elif name == "deferred_seed":
                if raised != "KeyError: 'T_re'":
                    continue
            elif re is not None:
                continue
            break
        else:
            raise SystemExit("%s: no seed from %d on meets the case's conditions" % (name, c["seed"]))
        p = name + "/"
        out[p + "seed"] = np.int64(seed)
        out[p + "in_sha"] = np.array("".join(rc.sha(flowds[k]["flow_abs"]) + rc.sha(flowds[k]["common_fov_mask"]) for k in sorted(flowds)))
        out[p + "planned"] = np.array([rcc.triple_name(s) for s in planned])
        out[p + "planned_idx_sorted"] = np.array([v[0] for v in planned.values()], np.int64)
        out[p + "planned_not_include"] = np.array([[v[1][k] for k in sorted(s)] for s, v in planned.items()], np.int64)
        out[p + "planned_counts"] = np.array([v[2] for v in planned.values()], np.int64)
        out[p + "raises"] = np.array(raised or "")
        if re is None:
            print("%-14s seed %3d: the reference raises %s" % (name, seed, raised))
            continue
        out[p + "seed3"] = np.array(sorted(re.seed), np.int64)
        out[p + "propagate_path"] = np.array([[i] + sorted(s) for i, s in re.propagate_path], np.int64)
        out[p + "rerooted"] = np.array(rerooted, dtype="U16")
        out[p + "triples"] = np.array([rcc.triple_name(s) for s in re.set3ds])
        out[p + "idx_sorted"] = np.array([d["idx_sorted"] for d in re.set3ds.values()], np.int64)
        out[p + "counts"] = np.array([len(d["uv_match_idx1"]) for d in re.set3ds.values()], np.int64)
        for s, d in re.set3ds.items():
            assert d["idx_sorted"] != planned[s][0] or len(d["uv_match_idx1"]) == planned[s][2], "the restatement counts differently"
            for key in ("uv_match_idx1", "uv_match_idx2"):
                put(out, "%s%s/%s" % (p, rcc.triple_name(s), key), d[key])
        out[p + "stereos"] = np.array(list(re.stereods), np.int64)
        for k, d in re.viewds.items():
            uvzis = d["uvzis"]
            assert uvzis.dtype == np.float64 and d["T_re"].dtype == np.float64
            out["%sview%d/T_re" % (p, k)] = d["T_re"]
            out["%sview%d/rows" % (p, k)] = np.int64(len(uvzis))
            out["%sview%d/uvi_sha" % (p, k)] = np.array(rc.sha(np.ascontiguousarray(uvzis[:, [0, 1, 3]])))
            out["%sview%d/z" % (p, k)] = np.ascontiguousarray(uvzis[::Z_STEP, 2])
        out[p + "ref_rot_error"] = np.float64(rcc.rotation_error({k: d["T_re"] for k, d in re.viewds.items()}, Ts))
        rng = np.random.default_rng(9200 + len(name))
        sens_T, sens_z = 0.0, 0.0
        for _ in range(ec.SENS_RUNS):
            r2 = run(reg, viewds, nudged_set2ds(set2ds, rng))
            assert r2.seed == re.seed and r2.propagate_path == re.propagate_path
            for k, d in re.viewds.items():
                sens_T = max(sens_T, float(np.abs(r2.viewds[k]["T_re"] - d["T_re"]).max()))
                sens_z = max(sens_z, float(np.abs(r2.viewds[k]["uvzis"][:, 2] - d["uvzis"][:, 2]).max()))
        out[p + "sens_T_re"], out[p + "sens_z"] = np.float64(sens_T), np.float64(sens_z)
        print("%-14s seed %3d: seed3 %s path %s rerooted %s counts %s..%s rot err %.3g sens T %.3g z %.3g" % (
            name, seed, sorted(re.seed), [i for i, _ in re.propagate_path], rerooted, out[p + "counts"].min(), out[p + "counts"].max(),
            out[p + "ref_rot_error"], sens_T, sens_z))
    np.savez_compressed(rcc.FIXTURE, **out)
    print("wrote %s (%d KB, %d arrays)" % (os.path.relpath(rcc.FIXTURE, ROOT), os.path.getsize(rcc.FIXTURE) // 1024, len(out)))


if __name__ == "__main__":
    main()
