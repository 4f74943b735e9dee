#!/usr/bin/env python3
"""Runs the REFERENCE's own sparse <-> dense functions on tests/sparse_cases.py and writes tests/golden/reference_sparse.npz.

BUILD CONTAINER ONLY (it needs the reference checkout, which does not travel to the GPU box; only the .npz does).
    python tests/golden/make_sparse_golden.py

What is executed.  The reference package is imported from where it lies, unmodified, through
``make_reference_golden.import_reference()`` (used as it is: the cv2 / boxx stand-ins described in that script's header),
and its own code runs the cases:
    utils.uvzs_to_arr2d, utils.arr2d_to_uvzs, utils.interpolate_uvzs ("nearest" through scipy.spatial.KDTree, "lstsq"
    through np.linalg.lstsq), utils.interpolate_sparse2d                                           utils.py:291-415
    epipolar_geometry.uvs_to_xyz_noramls + matched_xyz_normals_to_zs                               :84-97
    stereo_matching.FeatureMatchingAsStereoMatching.__call__                                       :113-142
    Stereo.get_depth with that plugin                                                              stereo_camera.py:492-533

Two names the reference uses are missing from what is installed here, and this script adds them IN ITS OWN PROCESS (the
reference's files are not touched):
    np.bool8   removed in NumPy 2 (arr2d_to_uvzs with a mask, utils.py:326-327)  -> np.bool_, what it was an alias of
    boxx.mg    a debugging helper called at stereo_matching.py:141                -> a no-op
Nothing of the reference's text goes into the repository; only the .npz is committed.
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
import reference_cases as rc  # noqa: E402
import sparse_cases as sc  # noqa: E402


def store_result(out, name, res):
    """A get_depth result dict in the layout reference_fixture.check_result reads."""
    keys = sorted(res)
    out[name + "/result_keys"] = np.array(keys)
    for k in keys:
        v = res[k]
        out["%s/out/%s_sha" % (name, k)] = np.array(rc.sha(v))
        out["%s/out/%s_dtype_shape" % (name, k)] = np.array([v.dtype.str] + [str(s) for s in v.shape])
        out["%s/out/%s" % (name, k)] = rc.sample(v)


def main():
    import oracle
    oracle.build()
    cal = mrg.import_reference()
    if not hasattr(np, "bool8"):
        np.bool8 = np.bool_
    sys.modules["boxx"].mg = lambda *a, **k: None
    u = cal.utils
    from calibrating import epipolar_geometry as eg, stereo_matching as sm
    out = {}

    for name in sc.NEAREST_CASES:
        uvzs, hw, distance = sc.nearest_case(name)
        got = u.interpolate_uvzs(uvzs.copy(), hw, inter_type="nearest", distance=distance)
        assert got.dtype == np.float32
        out["nearest/%s_sha" % name] = np.array(rc.sha(got))
        if got.size <= 120 * 160:
            out["nearest/" + name] = got
    uvzs, _, _ = sc.nearest_case(sc.NEAREST_HW_NONE)
    out["nearest/hw_none"] = u.interpolate_uvzs(uvzs.copy(), None, inter_type="nearest")
    empty = u.interpolate_uvzs(np.zeros((0, 3), np.float32), (5, 7), inter_type="nearest")
    out["nearest/empty_dtype_shape"] = np.array([empty.dtype.str] + [str(s) for s in empty.shape])
    for name, (src, grid, hw) in sc.UPSIZE_CASES.items():
        # the plugin's two lines after the fill (stereo_matching.py:139-140) on a fill of the grid
        uvzs = sc.nearest_case(src)[0]
        low = u.interpolate_uvzs(uvzs.copy(), grid, inter_type="nearest")
        low = low * hw[1] / grid[1]
        out["upsize/" + name + "_sha"] = np.array(rc.sha(sys.modules["boxx"].resize(low, hw, sys.modules["cv2"].INTER_NEAREST)))

    for name in sc.SCATTER_CASES:
        uv, values, hw, bg = sc.scatter_case(name)
        out["scatter/" + name] = u.uvzs_to_arr2d(uv.copy(), hw, bg, values=values.copy())
    packed = sc.packed_case()
    out["scatter/packed_hw_none"] = u.uvzs_to_arr2d(packed.copy())
    uv, values, hw, _ = sc.scatter_case("f32_c2")
    base = sc.image(99, hw + (2,), np.float32)
    out["scatter/in_place"] = u.uvzs_to_arr2d(uv.copy(), arr2d=base, values=values.copy())

    for name in sc.ARR2D_CASES:
        arr, mask = sc.arr2d_case(name)
        out["rows/" + name] = u.arr2d_to_uvzs(arr.copy(), None if mask is None else mask.copy())

    for name in sc.PLANE_CASES:
        uvzs, hw = sc.plane_case(name)
        out["plane/" + name] = u.interpolate_uvzs(uvzs.copy(), hw, inter_type="lstsq")
    for name, uvzs in sc.PLANE_DEGENERATE.items():
        out["plane/" + name] = u.interpolate_uvzs(uvzs.copy(), (8, 12), inter_type="lstsq")
    for inter in ("nearest", "lstsq"):
        out["sparse2d/" + inter] = u.interpolate_sparse2d(sc.sparse_image(), None, inter)

    for name in sc.REF_TRI_RELERR:
        uvs1, uvs2, K1, K2, T = sc.tri_case(name)
        zs = eg.matched_xyz_normals_to_zs(eg.uvs_to_xyz_noramls(uvs1, K1), eg.uvs_to_xyz_noramls(uvs2, K2), T)
        out["tri/%s_zs1" % name], out["tri/%s_zs2" % name] = zs["zs1"], zs["zs2"]

    for name, (hw, kw) in sc.PLUGIN_CASES.items():
        img = np.zeros(hw + (3,), np.uint8)
        res = sm.FeatureMatchingAsStereoMatching(sc.FakeFeatureMatcher(**kw))(img, img)
        assert sorted(res) == ["disparity", "matched"]
        out["plugin/%s_sha" % name] = np.array(rc.sha(res["disparity"]))
        out["plugin/" + name] = rc.sample(res["disparity"])

    case = sc.GET_DEPTH_CASE
    st = cal.Stereo().load(rc.rig_record(case))
    st.set_stereo_matching(sm.FeatureMatchingAsStereoMatching(sc.FakeFeatureMatcher(**case["matcher"])), **case["setm"])
    img1, img2 = rc.images(case)
    res = st.get_depth(img1.copy(), img2.copy())
    matched = res.pop("matched")
    assert sorted(matched) == ["uvs1", "uvs2"]
    out[case["name"] + "/img1_sha"], out[case["name"] + "/img2_sha"] = np.array(rc.sha(img1)), np.array(rc.sha(img2))
    store_result(out, case["name"], res)

    np.savez_compressed(sc.FIXTURE, **out)
    print("wrote %s (%d KB, %d arrays)" % (os.path.relpath(sc.FIXTURE, ROOT), os.path.getsize(sc.FIXTURE) // 1024, len(out)))


if __name__ == "__main__":
    main()
