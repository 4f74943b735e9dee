"""The sparse <-> dense family without a GPU: the NumPy restatements (tests/sparse_ref.py) against the reference's own
output (tests/golden/reference_sparse.npz, made by tests/golden/make_sparse_golden.py), the conditions the bit-for-bit
GPU tests rest on, the reference's own distance from the exact plane / triangulation (the yardstick of the GPU tests'
bounds), and the parts of the new surface that need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import reference_cases as rc  # noqa: E402
import sparse_cases as sc  # noqa: E402
import sparse_ref as sr  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    f = sc.load_fixture()
    assert f is not None, "tests/golden/reference_sparse.npz is missing (python tests/golden/make_sparse_golden.py)"
    return f


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- restatements == the reference's output, bit for bit -------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.SCATTER_CASES))
def test_scatter_restatement_equals_the_reference(fx, name):
    uv, values, hw, bg = sc.scatter_case(name)
    assert _same(sr.scatter(uv, values, hw, bg), fx["scatter/" + name])


def test_scatter_quirks_equal_the_reference(fx):
    packed = sc.packed_case()
    got = sr.scatter(packed[:, :2], packed[:, 2:])
    assert _same(got, fx["scatter/packed_hw_none"])
    assert got.shape[0] == int(np.round(packed[:, 0].max())) + 1  # (max u + 1) used as the HEIGHT: the reference's quirk
    uv, values, hw, _ = sc.scatter_case("f32_c2")
    assert _same(sr.scatter(uv, values, arr2d=sc.image(99, hw + (2,), np.float32)), fx["scatter/in_place"])
    # the cases do put several rows on one pixel, and rows outside
    uv, _, hw, _ = sc.scatter_case("u8_c1")
    xs, ys = np.int32(np.round(uv)).T
    inside = (xs >= 0) & (xs < hw[1]) & (ys >= 0) & (ys < hw[0])
    assert 0 < inside.sum() < len(uv) and len(np.unique(ys[inside] * hw[1] + xs[inside])) < inside.sum()


@pytest.mark.parametrize("name", list(sc.ARR2D_CASES))
def test_rows_restatement_equals_the_reference(fx, name):
    arr, mask = sc.arr2d_case(name)
    assert _same(sr.rows_of(arr, mask), fx["rows/" + name])


@pytest.mark.parametrize("name", list(sc.NEAREST_CASES))
def test_nearest_restatements_equal_the_reference_and_their_margins_hold(fx, name):
    uvzs, hw, distance = sc.nearest_case(name)
    stats = {}
    win = sr.nearest_windowed(uvzs, hw, distance, stats)
    assert rc.sha(win) == str(fx["nearest/%s_sha" % name])
    if "nearest/" + name in fx:
        assert _same(win, fx["nearest/" + name])
    # what lets the GPU be compared bit for bit: neither the tie rule nor the threshold decided any value
    print("%s: smallest gap between neighbours %.3g, smallest margin to distance %.3g" % (name, stats["min_gap"], stats["min_edge"]))
    assert stats["min_gap"] > sc.GAP and stats["min_edge"] > sc.GAP
    if hw[0] * hw[1] * len(uvzs) <= 120 * 160 * 1500:
        bstats = {}
        assert _same(sr.nearest_brute(uvzs, hw, distance, bstats), win)
        assert bstats["min_gap"] == stats["min_gap"] and bstats["min_edge"] == stats["min_edge"]


def test_nearest_agrees_with_scipy_when_it_imports():
    spatial = pytest.importorskip("scipy.spatial")
    uvzs, hw, distance = sc.nearest_case("n700_60x80")
    ys, xs = np.mgrid[:hw[0], :hw[1]]
    d, i = spatial.KDTree(uvzs[:, :2]).query(np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64))
    want = np.where(d < distance, np.float32(uvzs[i, 2]), np.float32(0)).reshape(hw)
    assert _same(sr.nearest_brute(uvzs, hw, distance), want)


def test_nearest_quirks_equal_the_reference(fx):
    uvzs, _, _ = sc.nearest_case(sc.NEAREST_HW_NONE)
    hw = int(uvzs[:, 1].max()) + 2, int(uvzs[:, 0].max()) + 2
    assert _same(sr.nearest_windowed(uvzs, hw, 2), fx["nearest/hw_none"])
    assert [str(s) for s in fx["nearest/empty_dtype_shape"]] == [np.dtype(np.float32).str, "5", "7"]
    for name, (src, grid, hw) in sc.UPSIZE_CASES.items():
        low = sr.nearest_windowed(sc.nearest_case(src)[0], grid, 2)
        assert rc.sha(sr.resize_nearest_scaled(low, hw)) == str(fx["upsize/%s_sha" % name]), name


def test_plane_and_sparse2d_restatements_equal_the_reference(fx):
    for name in sc.PLANE_CASES:
        assert _same(sr.plane(*sc.plane_case(name)), fx["plane/" + name]), name
    for name, uvzs in sc.PLANE_DEGENERATE.items():
        assert _same(sr.plane(uvzs, (8, 12)), fx["plane/" + name]), name
    img = sc.sparse_image()
    rows = sr.rows_of(img, (img != 0) & np.isfinite(img))
    assert _same(sr.nearest_windowed(rows, img.shape, 2), fx["sparse2d/nearest"])
    assert _same(sr.plane(rows, img.shape), fx["sparse2d/lstsq"])


# ---- the reference's own distance from the exact answer: the yardstick of the GPU bounds ------------------------------
@pytest.mark.parametrize("name", list(sc.PLANE_CASES))
def test_plane_reference_error(fx, name):
    uvzs, _ = sc.plane_case(name)
    ulps = sr.plane_ulps(fx["plane/" + name], sr.plane_exact(uvzs))
    print("%s: the reference's dense plane lies %.6g float32 ulps from the exact one" % (name, ulps))
    assert ulps == pytest.approx(sc.REF_PLANE_ULPS[name], rel=1e-3), "sparse_cases.REF_PLANE_ULPS is not what is measured"


@pytest.mark.parametrize("name", list(sc.REF_TRI_RELERR))
def test_triangulation_reference_error(fx, name):
    uvs1, uvs2, K1, K2, T = sc.tri_case(name)
    e1, e2 = sr.triangulate_exact(uvs1, uvs2, K1, K2, T)
    err = max(sr.relerr(fx["tri/%s_zs1" % name], e1), sr.relerr(fx["tri/%s_zs2" % name], e2))
    print("%s: the reference's zs lie %.6g (relative) from the exact ones" % (name, err))
    assert err == pytest.approx(sc.REF_TRI_RELERR[name], rel=1e-3), "sparse_cases.REF_TRI_RELERR is not what is measured"
    if name == "tri_rectified":  # zs1 = baseline * fx / d on a rectified rig, exactly
        d = uvs1[:, 0] - uvs2[:, 0]
        assert max(abs(float(z) - 0.12 * K1[0, 0] / dd) / float(z) for z, dd in zip(e1, d)) < 1e-12


# ---- the new surface, as far as it needs no device --------------------------------------------------------------------
def test_surface_without_a_gpu():
    import calibrating_amd as ca
    import calibrating_amd.sparse as sparse
    for name in ("uvzs_to_arr2d", "arr2d_to_uvzs", "interpolate_uvzs", "interpolate_sparse2d", "matched_uvs_to_zs"):
        assert callable(getattr(sparse, name))
    assert "FeatureMatchingAsStereoMatching" in ca.__all__
    plugin = ca.FeatureMatchingAsStereoMatching(sc.FakeFeatureMatcher())
    assert isinstance(plugin, ca.MetaStereoMatching) and plugin.accepts_device_tensors is True and plugin.downscale == 8
    assert not getattr(ca.SemiGlobalBlockMatching, "accepts_device_tensors", False)
    assert callable(ca.Stereo.get_depth_by_matched_uvs)
    uvzs = np.zeros((4, 3))
    with pytest.raises(NotImplementedError, match="thin-plate"):
        sparse.interpolate_uvzs(uvzs, (4, 4), inter_type="rbf")
    with pytest.raises(NotImplementedError, match="convexHull"):
        sparse.interpolate_uvzs(uvzs, (4, 4), constrained_type="convex_hull", inter_type="nearest")
    with pytest.raises(NotImplementedError, match="convexHull"):
        sparse.interpolate_sparse2d(np.zeros((4, 4)), True)
    with pytest.raises(ValueError, match="distance"):
        sparse.interpolate_uvzs(uvzs, (4, 4), inter_type="nearest", distance=sparse.MAX_DISTANCE + 1)
    with pytest.raises(ValueError, match="finite"):
        sparse.interpolate_uvzs(np.array([[np.nan, 1.0, 2.0]]), (4, 4), inter_type="nearest")
    assert sparse.interpolate_uvzs(np.zeros((0, 3), np.float32), (5, 7), inter_type="nearest").dtype == np.float32
