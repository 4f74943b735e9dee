#!/usr/bin/env python3
"""Runs the REFERENCE's own epipolar functions on tests/epipolar_cases.py and writes tests/golden/reference_epipolar.npz.

BUILD CONTAINER ONLY (it needs the reference checkout, which does not travel to the GPU box; only the .npz does).
    python tests/golden/make_epipolar_golden.py

What is executed.  The reference package is imported from where it lies, unmodified, through
``make_reference_golden.import_reference()`` (``boxx.mg`` a no-op, as in make_sparse_golden.py), and its own code runs:
    epipolar_geometry.EssentialMatrixStereo (+ from_stereo, align_scale_with, set_scale), compute_essential_matrix,
    decompose_essential_matrix, matched_xyz_normals_to_zs, filter_overlap_uvs, matching_uvs_in_one_img
    flow_utils.flow_abs_to_normal / flow_normal_to_abs
    reconstruction_epipolar_geometry.ReconstructionExtrinsics.build_set2ds_by_flowds
This path is NumPy only (np.linalg.svd, np.unique): nothing of cv2 is behind these numbers.

Per pose case the script also stores
    <case>/cand_means    the mean zs1 / zs2 of all four candidates (and asserts the generator condition: none within
                         MEAN_FLOOR of zero relative to the largest, so no reduction order can change the winner)
    <case>/sens_*        the largest change of R, t, E (up to sign), z1, z2 over SENS_RUNS reruns of the reference's
                         constructor with every input coordinate moved by one ulp in a seeded direction
    <case>/ref_zs_relerr the reference's own distance from the exact zs (fractions.Fraction) on ZS_SAMPLE matches
    <case>/ref_row_error how far apart (px) the reference's own rig puts the rows of the case's scene points when camera 2
                         stands where it truly stood: the estimation error of its 8-point pose, in rectified rows
Long arrays go in as SHA-256 plus a thinned copy.  Nothing of the reference's text goes into the repository.
"""
import json
import os
import sys

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


def thin(a):
    """About 512 entries of an array, evenly spaced in its flattened form."""
    return np.ascontiguousarray(a.reshape(-1)[:: max(1, a.size // 512)])


def put(out, key, a):
    """An array whole when small, else its SHA-256 and a thinned copy; dtype and shape always."""
    a = np.asarray(a)
    out[key + "_sha"] = np.array(rc.sha(a))
    out[key + "_dtype_shape"] = np.array([a.dtype.str] + [str(s) for s in a.shape])
    out[key] = a if a.size <= 4096 else thin(a)


def construct(eg, cal, c):
    if "record" in c:
        return eg.EssentialMatrixStereo.from_stereo(c["uvs1"], c["uvs2"], cal.Stereo().load(c["record"]))
    return eg.EssentialMatrixStereo(c["uvs1"], c["uvs2"], c["K1"], c["K2"], baseline=c["baseline"], xy1=list(c["xy1"]),
                                    xy2=list(c["xy2"]))


def pose(out, eg, cal, name, c):
    st = construct(eg, cal, c)
    ep = st.epipolar
    R, t = np.array(st.R, np.float64), np.array(st.t, np.float64).reshape(3)
    K2 = c["K1"] if c["K2"] is None else c["K2"]
    x1, x2 = eg.uvs_to_xyz_noramls(c["uvs1"], c["K1"]), eg.uvs_to_xyz_noramls(c["uvs2"], K2)
    cands = eg.decompose_essential_matrix(ep["E"])
    means = []
    for T in cands:
        T[:3, 3] *= st.baseline / np.linalg.norm(T[:3, 3])
        zs = eg.matched_xyz_normals_to_zs(x1, x2, T)
        means.append([zs["zs1"].mean(), zs["zs2"].mean()])
    means = np.array(means)
    out[name + "/candidates"] = np.array(cands, np.float64)  # all four T_1to2, t scaled to the baseline, in order
    small = np.abs(means).min(1)
    assert small.min() >= ec.MEAN_FLOOR * small.max(), (name, means)
    winner = next((i for i in range(4) if means[i, 0] > 0 and means[i, 1] > 0), 3)
    assert np.array_equal(cands[winner][:3, :3], R) and np.allclose(cands[winner][:3, 3], t, rtol=1e-12, atol=0), name
    rows = ec.zs_sample(len(c["uvs1"]))
    out.update({name + "/R": R, name + "/t": t, name + "/E": ep["E"], name + "/z1": np.float64(ep["z1"]),
                name + "/z2": np.float64(ep["z2"]), name + "/cand_means": means, name + "/winner": np.int64(winner),
                name + "/baseline": np.float64(st.baseline),
                name + "/ref_zs_relerr": np.float64(er.zs_relerr(ep["zs1"], ep["zs2"], c["uvs1"], c["uvs2"], c["K1"], K2, R, t, rows)),
                name + "/uvs1_sha": np.array(rc.sha(c["uvs1"])), name + "/uvs2_sha": np.array(rc.sha(c["uvs2"]))})
    for k in ("R1", "R2", "K"):
        out["%s/%s" % (name, k)] = np.array(getattr(st, k), np.float64)
    v1, v2 = er.rectified_v(st, c["X1"], c["R"], c["t"])  # the reference's own rig on the true observations
    out[name + "/ref_row_error"] = np.float64(np.abs(v1 - v2).max())
    if "record" in c:
        out[name + "/dump_json"] = np.array(json.dumps(st.dump(return_dict=True), sort_keys=True))
    rng = np.random.default_rng(9000 + len(name))
    sens = dict(R=0.0, t=0.0, E=0.0, z1=0.0, z2=0.0)
    for _ in range(ec.SENS_RUNS):
        s2 = construct(eg, cal, dict(c, uvs1=ec.nudged(c["uvs1"], rng), uvs2=ec.nudged(c["uvs2"], rng)))
        sens["R"] = max(sens["R"], np.abs(np.array(s2.R) - R).max())
        sens["t"] = max(sens["t"], np.abs(np.array(s2.t).reshape(3) - t).max())
        sens["E"] = max(sens["E"], er.E_distance(s2.epipolar["E"], ep["E"]))
        sens["z1"] = max(sens["z1"], abs(s2.epipolar["z1"] - ep["z1"]))
        sens["z2"] = max(sens["z2"], abs(s2.epipolar["z2"] - ep["z2"]))
    for k, v in sens.items():
        out["%s/sens_%s" % (name, k)] = np.float64(v)
    print("%-24s n=%6d winner=%d  |R-R_true|=%.3g  sens R %.3g t %.3g E %.3g z1 %.3g z2 %.3g  ref zs relerr %.3g" % (
        name, len(c["uvs1"]), winner, np.abs(R - c["R"]).max(), sens["R"], sens["t"], sens["E"], sens["z1"], sens["z2"],
        out[name + "/ref_zs_relerr"]))


def trio(out, eg):
    tc = ec.trio_case()

    def run(A, B):
        a, b = eg.EssentialMatrixStereo(**A), eg.EssentialMatrixStereo(**B)
        b.align_scale_with(a)
        first = b.baseline
        b.align_scale_with(a)
        return first / a.baseline, b.baseline / a.baseline

    ratio, again = run(tc["A"], tc["B"])
    rng = np.random.default_rng(9100)
    sens = 0.0
    for _ in range(ec.SENS_RUNS):
        A, B = dict(tc["A"]), dict(tc["B"])
        for d in (A, B):
            d["uvs1"], d["uvs2"] = ec.nudged(d["uvs1"], rng), ec.nudged(d["uvs2"], rng)
        sens = max(sens, abs(run(A, B)[0] - ratio))
    out["trio/ratio"], out["trio/ratio_again"], out["trio/sens_ratio"] = np.float64(ratio), np.float64(again), np.float64(sens)
    print("trio: ratio %.12g (true %.12g), second align %.3g relative, sens %.3g" % (ratio, tc["true_ratio"], abs(again / ratio - 1), sens))


def main():
    cal = mrg.import_reference()
    sys.modules["boxx"].mg = lambda *a, **k: None
    from calibrating import epipolar_geometry as eg, flow_utils as fu, reconstruction_epipolar_geometry as reg
    out = {}

    for name in ec.ALL_POSE_CASES:
        if name == "later_winner":
            for seed in ec.LATER_WINNER_SEEDS:
                c = ec.pose_case(name, seed)
                st = construct(eg, cal, c)
                first = eg.decompose_essential_matrix(st.epipolar["E"])[0]
                if not np.array_equal(first[:3, :3], np.array(st.R)) or np.dot(first[:3, 3], np.array(st.t).reshape(3)) < 0:
                    break
            else:
                raise SystemExit("no seed gives a winner other than the first candidate")
            out[name + "/seed"] = np.int64(seed)
        else:
            c = ec.pose_case(name)
        pose(out, eg, cal, name, c)
    assert int(out["later_winner/winner"]) != 0
    trio(out, eg)

    for name in ec.MATCH_CASES:
        uvs1, uvs2, d, k = ec.match_case(name)
        got = eg.matching_uvs_in_one_img(uvs1.copy(), uvs2.copy(), d, k)
        out["match/%s/keys" % name] = np.array(sorted(got))
        out["match/%s/in_sha" % name] = np.array(rc.sha(uvs1) + rc.sha(uvs2))
        for key, v in got.items():
            put(out, "match/%s/%s" % (name, key), v)
        print("match %-24s -> %s" % (name, len(got["uv_match_idx1"]) if got else "{}"))

    for name in ec.OVERLAP_CASES:
        uvs1, uvs2 = ec.overlap_case(name)
        a, b = eg.filter_overlap_uvs(uvs1.copy(), uvs2.copy())
        out["overlap/%s/in_sha" % name] = np.array(rc.sha(uvs1) + rc.sha(uvs2))
        put(out, "overlap/%s/uvs1" % name, a)
        put(out, "overlap/%s/uvs2" % name, b)
        print("overlap %-22s keeps %d of %d" % (name, len(a), len(uvs1)))

    for name in ec.FLOW_CASES:  # one direction of build_set2ds_by_flowds: a single-pair flowds
        flow, mask = ec.flow_case(name)
        got = reg.ReconstructionExtrinsics.build_set2ds_by_flowds({0: {}, 1: {}}, {(0, 1): dict(flow_abs=flow, common_fov_mask=mask)})
        out["flow/%s/in_sha" % name] = np.array(rc.sha(flow) + rc.sha(mask))
        out["flow/%s/pairs" % name] = np.int64(len(got))
        if got:
            put(out, "flow/%s/from" % name, got[frozenset((0, 1))]["uvs_ij_i"])
            put(out, "flow/%s/to" % name, got[frozenset((0, 1))]["uvs_ij_j"])

    for name in ec.FLOWDS_CASES:
        viewds, flowds = ec.flowds_case(name)
        try:
            got = reg.ReconstructionExtrinsics.build_set2ds_by_flowds(viewds, flowds)
        except Exception as e:  # what the reference does with this input is part of the record
            out["flowds/%s/raises" % name] = np.array("%s: %s" % (type(e).__name__, e))
            print("flowds %s: the reference raises %s: %s" % (name, type(e).__name__, e))
            continue
        out["flowds/%s/pairs" % name] = np.array(sorted(",".join(str(v) for v in sorted(k)) for k in got))
        for k, d in got.items():
            pair = ",".join(str(v) for v in sorted(k))
            out["flowds/%s/%s/keys" % (name, pair)] = np.array(list(d))
            for key, v in d.items():
                put(out, "flowds/%s/%s/%s" % (name, pair, key), v)

    for name, (seed, hw, target) in ec.CONVERT_CASES.items():
        flow = ec.flow_abs(seed, hw)
        normal = fu.flow_abs_to_normal(flow)
        put(out, "convert/%s/normal" % name, normal)
        put(out, "convert/%s/abs" % name, np.ascontiguousarray(fu.flow_normal_to_abs(normal, target)))
        put(out, "convert/%s/abs_of_f64" % name, np.ascontiguousarray(fu.flow_normal_to_abs(normal.astype(np.float64), target)))
        put(out, "convert/%s/normal_of_f64" % name, fu.flow_abs_to_normal(flow.astype(np.float64)))

    np.savez_compressed(ec.FIXTURE, **out)
    print("wrote %s (%d KB, %d arrays)" % (os.path.relpath(ec.FIXTURE, ROOT), os.path.getsize(ec.FIXTURE) // 1024, len(out)))


if __name__ == "__main__":
    main()
