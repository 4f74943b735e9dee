"""Measures, without a GPU, what the robust reconstruction can be held to (tests/essential_batch_cases.py, CPU_ERRORS).

BUILD CONTAINER ONLY (it needs the reference checkout, imported unmodified as tests/golden/make_reconstruction_golden.py does).
Nothing is written: the numbers are printed and copied into tests/essential_batch_cases.py by hand.

For ``one_triple`` and ``ten_triples``: the reference's own ``build_set2ds_by_flowds``, the contamination of
``essential_batch_cases.contaminated``, every pair filtered with the NumPy restatement ``essential_ref.find(**ROBUST)``, then the
reference's own class on the filtered matches -- the CPU composition of ``ReconstructionExtrinsics(cfg=dict(robust=...))``.
As there, a rig takes its pair's matrix from the estimator (its transpose for the rig j -> i): while the class runs, the
reference module's ``compute_essential_matrix`` is replaced, at run time and in this process only, by a look-up of the
restatement's answer for the rays it is handed.
Printed: ``bundle_ref.pose_errors`` of that, of the clean scene, and what the class does with the contaminated matches
unfiltered; the leak (wrong pairs among the inliers); the conditions the scene has to meet.

    python tests/golden/make_essential_batch_bound.py [threshold [wrong [seed]]]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_reference_golden as mrg  # noqa: E402
import bundle_ref  # noqa: E402
import essential_batch_cases as ebc  # noqa: E402
import essential_ref as er  # noqa: E402
import reconstruction_cases as rcc  # noqa: E402

MAX_ROTATION, MAX_CENTRE_SHARE = 0.05, 0.05  # rad; of the mean distance of the true centres from view 0's


def errors(re, Ts):
    keys = sorted(re.viewds)
    return bundle_ref.pose_errors(np.array([re.viewds[k]["T_re"] for k in keys]), np.array([Ts[k] for k in keys]))


def main():
    threshold = float(sys.argv[1]) if len(sys.argv) > 1 else ebc.ROBUST["threshold"]
    wrong = float(sys.argv[2]) if len(sys.argv) > 2 else ebc.WRONG
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else ebc.WRONG_SEED
    mrg.import_reference()
    sys.modules["boxx"].mg = lambda *a, **k: None
    from calibrating import epipolar_geometry as ege, reconstruction_epipolar_geometry as reg
    fx = rcc.load_fixture()
    for name in ("one_triple", "ten_triples"):
        viewds, flowds, Ts = rcc.case(name, int(fx[name + "/seed"]))
        set2ds = reg.ReconstructionExtrinsics.build_set2ds_by_flowds(viewds, flowds)
        c = np.array([T[:3, 3] for T in Ts])
        baseline = float(np.linalg.norm(c[1:] - c[0], axis=1).mean())
        clean = errors(reg.ReconstructionExtrinsics(rcc.fresh(viewds), set2ds={k: dict(v) for k, v in set2ds.items()}), Ts)
        bad = ebc.contaminated(set2ds, wrong, seed)
        filtered, leak, total, known = {}, 0, 0, {}
        for set2, d in bad.items():
            i, j = sorted(set2)
            info = er.find(d["uvs_i"], d["uvs_j"], viewds[i]["K"], viewds[j]["K"], threshold, ebc.ROBUST["hypotheses"], ebc.ROBUST["seed"])
            on = info["inliers"] if info["status"] == "ok" else np.zeros(len(d["uvs_i"]), bool)
            moved = (d["uvs_j"] != np.asarray(set2ds[set2]["uvs_j"])).any(1)
            leak, total = leak + int((on & moved).sum()), total + int(on.sum())
            filtered[set2] = dict(uvs_i=d["uvs_i"][on], uvs_j=d["uvs_j"][on])
            if on.any():
                for uv, view, E in ((d["uvs_i"][on], i, info["E"]), (d["uvs_j"][on], j, info["E"].T)):
                    ray = np.append(uv[0], 1) @ np.linalg.inv(viewds[view]["K"]).T
                    known[(int(on.sum()), round(float(ray[0]), 9), round(float(ray[1]), 9))] = np.array(E)
        plain_fit = ege.compute_essential_matrix
        ege.compute_essential_matrix = lambda x1, x2: known[(len(x1), round(float(x1[0, 0]), 9), round(float(x1[0, 1]), 9))]
        try:
            got = errors(reg.ReconstructionExtrinsics(rcc.fresh(viewds), set2ds=filtered), Ts)
        finally:
            ege.compute_essential_matrix = plain_fit
        try:
            plain = errors(reg.ReconstructionExtrinsics(rcc.fresh(viewds), set2ds={k: dict(v) for k, v in bad.items()}), Ts)
        except Exception as e:  # what the class does with wrong pairs is part of the record
            plain = "%s: %s" % (type(e).__name__, e)
        ok = got[0] <= MAX_ROTATION and got[1] <= MAX_CENTRE_SHARE * baseline
        print("%-12s threshold %g wrong %g seed %d: baseline %.4f; clean %r; filtered on the CPU %r (%d of %d inliers are wrong pairs); "
              "unfiltered %r; conditions %s" % (name, threshold, wrong, seed, baseline, clean, got, leak, total, plain, "met" if ok else "MISSED"))


if __name__ == "__main__":
    main()
