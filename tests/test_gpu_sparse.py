"""Sparse samples <-> dense images on the GPU (-m gpu): calibrating_amd.sparse, FeatureMatchingAsStereoMatching, the
device-resident plugin path of Stereo.get_depth and Stereo.get_depth_by_matched_uvs against the reference's own output
(tests/golden/reference_sparse.npz) and the NumPy restatements (tests/sparse_ref.py).  Scatter, rows and the nearest
fill are compared bit for bit on every pixel -- tests/test_sparse_cpu.py shows that no tie and no threshold decision
comes closer than 1e-9 in the inputs; the plane and the triangulation are bounded by twice the reference's own distance
from the exact answer (sparse_cases.REF_PLANE_ULPS / REF_TRI_RELERR).  Plain imports: a missing feature fails."""
import os
import sys

import numpy as np
import pytest
import torch

import calibrating_amd as ca
from calibrating_amd import sparse

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import reference_cases as rc  # noqa: E402
import reference_fixture as rf  # noqa: E402
import sparse_cases as sc  # noqa: E402
import sparse_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    f = sc.load_fixture()
    assert f is not None, "tests/golden/reference_sparse.npz is missing"
    return f


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    assert isinstance(t, torch.Tensor) and t.is_cuda, type(t)
    return t.cpu().numpy()


# ---- scatter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.SCATTER_CASES))
def test_scatter_equals_the_reference(fx, name):
    uv, values, hw, bg = sc.scatter_case(name)
    want = fx["scatter/" + name]
    assert _same(want, sr.scatter(uv, values, hw, bg))
    got = sparse.uvzs_to_arr2d(uv, hw, bg, values=values)
    assert isinstance(got, np.ndarray) and _same(got, want)
    assert _same(_np(sparse.uvzs_to_arr2d(_cuda(uv), hw, bg, values=_cuda(values))), want)
    assert _same(sparse.uvzs_to_arr2d(uv.astype(np.float32).astype(np.float64), hw, bg, values=values),
                 sparse.uvzs_to_arr2d(uv.astype(np.float32), hw, bg, values=values))  # float32 coordinates round alike


def test_scatter_quirks_equal_the_reference(fx):
    packed = sc.packed_case()
    assert _same(sparse.uvzs_to_arr2d(packed), fx["scatter/packed_hw_none"])            # (n, 2 + C) rows, hw=None
    assert _same(_np(sparse.uvzs_to_arr2d(_cuda(packed))), fx["scatter/packed_hw_none"])
    uv, values, hw, _ = sc.scatter_case("f32_c2")
    base = sc.image(99, hw + (2,), np.float32)
    got = sparse.uvzs_to_arr2d(uv, arr2d=base, values=values)
    assert got is base and _same(base, fx["scatter/in_place"])                             # updated in place and returned
    tbase = _cuda(sc.image(99, hw + (2,), np.float32))
    assert sparse.uvzs_to_arr2d(_cuda(uv), arr2d=tbase, values=_cuda(values)) is tbase and _same(_np(tbase), fx["scatter/in_place"])


def test_scatter_duplicates_the_higher_row_wins():
    uv = np.array([[2.2, 1.0], [1.9, 1.4], [2.5, 0.6], [7.0, 7.0], [2.0, 1.0]] * 50 + [[1.6, 0.5]])
    values = np.arange(len(uv), dtype=np.float32)
    got = sparse.uvzs_to_arr2d(uv, (3, 4), -1, values=values)
    want = np.full((3, 4), -1, np.float32)
    want[1, 2] = 249      # rows 0, 1, 2 (2.5 -> 2, 0.6 -> 1), 4 of every group land on (2, 1): the last of them
    want[0, 2] = 250      # 1.6 -> 2, 0.5 -> 0 (half to even)
    assert _same(got, want)


# ---- rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.ARR2D_CASES))
def test_rows_equal_the_reference(fx, name):
    arr, mask = sc.arr2d_case(name)
    want = fx["rows/" + name]
    assert _same(want, sr.rows_of(arr, mask))
    assert _same(sparse.arr2d_to_uvzs(arr, mask), want)
    assert _same(_np(sparse.arr2d_to_uvzs(_cuda(arr), None if mask is None else _cuda(mask))), want)


# ---- nearest ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.NEAREST_CASES))
def test_nearest_equals_the_reference_on_every_pixel(fx, name):
    uvzs, hw, distance = sc.nearest_case(name)
    want = sr.nearest_windowed(uvzs, hw, distance)
    assert rc.sha(want) == str(fx["nearest/%s_sha" % name])
    got = sparse.interpolate_uvzs(uvzs, hw, inter_type="nearest", distance=distance)
    assert isinstance(got, np.ndarray) and _same(got, want), "%d pixels differ" % (got != want).sum()
    assert rc.sha(got) == str(fx["nearest/%s_sha" % name])
    assert _same(_np(sparse.interpolate_uvzs(_cuda(uvzs), hw, inter_type="nearest", distance=distance)), want)


def test_nearest_quirks_equal_the_reference(fx):
    uvzs, _, _ = sc.nearest_case(sc.NEAREST_HW_NONE)
    assert _same(sparse.interpolate_uvzs(uvzs, None, inter_type="nearest"), fx["nearest/hw_none"])
    assert _same(_np(sparse.interpolate_uvzs(_cuda(uvzs), inter_type="nearest")), fx["nearest/hw_none"])
    empty = sparse.interpolate_uvzs(_cuda(np.zeros((0, 3), np.float32)), (5, 7), inter_type="nearest")
    assert empty.dtype == torch.float32 and tuple(empty.shape) == (5, 7) and not empty.any()
    img = sc.sparse_image()
    assert _same(sparse.interpolate_sparse2d(img, None, "nearest"), fx["sparse2d/nearest"])
    assert _same(_np(sparse.interpolate_sparse2d(_cuda(img), None, "nearest")), fx["sparse2d/nearest"])
    with pytest.raises(ValueError, match="finite"):
        sparse.interpolate_uvzs(_cuda(np.array([[1.0, np.inf, 2.0]])), (4, 4), inter_type="nearest")


def test_nearest_equal_distances_the_lower_index_wins():
    # pixel (2, 1): samples 1 and 2 mirror each other about it (bit-equal distance), sample 0 is farther
    uvzs = np.array([[2.0, 2.5, 10.0], [2.75, 1.5, 20.0], [1.25, 0.5, 30.0], [9.0, 9.0, 40.0]])
    got = sparse.interpolate_uvzs(uvzs, (4, 5), inter_type="nearest")
    assert got[1, 2] == 20.0
    assert sparse.interpolate_uvzs(uvzs[[0, 2, 1, 3]], (4, 5), inter_type="nearest")[1, 2] == 30.0
    assert _same(got, sr.nearest_brute(uvzs, (4, 5)))
    # a sample exactly `distance` away is not taken (<, not <=)
    assert sparse.interpolate_uvzs(np.array([[5.0, 1.0, 7.0]]), (3, 8), inter_type="nearest")[1, 3] == 0.0
    assert sparse.interpolate_uvzs(np.array([[5.0, 1.0, 7.0]]), (3, 8), inter_type="nearest")[1, 4] == 7.0


def test_fused_upsizing_equals_fill_resize_scale(fx):
    for name, (src, grid, hw) in sc.UPSIZE_CASES.items():
        uvzs = sc.nearest_case(src)[0]
        low = sparse.interpolate_uvzs(uvzs, grid, inter_type="nearest")
        want = sr.resize_nearest_scaled(low, hw)
        assert rc.sha(want) == str(fx["upsize/%s_sha" % name])
        got = sparse.interpolate_uvzs(uvzs, grid, inter_type="nearest", resize_hw=hw)
        assert _same(got, want), name


def test_nearest_at_scale_full_resolution():
    """1920x1080, 200 000 samples, no downscaling: the case the reference gave up on."""
    uvzs, hw, distance = sc.scale_case()
    stats = {}
    want = sr.nearest_windowed(uvzs, hw, distance, stats)
    print("scale: smallest gap %.3g, smallest margin to distance %.3g" % (stats["min_gap"], stats["min_edge"]))
    assert stats["min_gap"] > sc.GAP and stats["min_edge"] > sc.GAP
    got = _np(sparse.interpolate_uvzs(_cuda(uvzs), hw, inter_type="nearest", distance=distance))
    assert _same(got, want), "%d pixels differ" % (got != want).sum()

    class Matcher:  # the same samples through the plugin at downscale=1
        cfg = {}

        def __call__(self, img1, img2):
            uv1 = uvzs[:, :2] / np.array([hw[1], hw[0]], np.float64)
            uv2 = uv1.copy()
            uv2[:, 0] -= uvzs[:, 2] / hw[1]
            return dict(uvs1=_cuda(uv1), uvs2=_cuda(uv2))

    img = torch.zeros(hw + (3,), dtype=torch.uint8, device="cuda")
    res = ca.FeatureMatchingAsStereoMatching(Matcher(), downscale=1)(img, img)
    m = Matcher()(img, img)
    s1, s2_ = _np(m["uvs1"]) * (hw[1], hw[0]), _np(m["uvs2"]) * (hw[1], hw[0])
    uvds = np.concatenate([s1, (s1 - s2_)[:, :1]], 1)
    s2 = {}
    want2 = sr.nearest_windowed(uvds, hw, 2, s2)
    assert s2["min_gap"] > sc.GAP and s2["min_edge"] > sc.GAP
    assert _same(_np(res["disparity"]), want2)


# ---- plane -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.PLANE_CASES))
def test_plane_within_twice_the_references_error(name):
    uvzs, hw = sc.plane_case(name)
    got = sparse.interpolate_uvzs(uvzs, hw, inter_type="lstsq")
    assert got.dtype == np.float32 and got.shape == hw
    ulps = sr.plane_ulps(got, sr.plane_exact(uvzs))
    allowed = max(1.0, 2 * sc.REF_PLANE_ULPS[name])
    print("%s: %.6g float32 ulps from the exact plane (reference %.6g, allowed %.6g)" % (name, ulps, sc.REF_PLANE_ULPS[name], allowed))
    assert ulps <= allowed
    again = sparse.interpolate_uvzs(_cuda(uvzs), hw)  # the default inter_type; a second run: the same bits
    assert _same(_np(again), got)


def test_plane_fixed_reduction_order_and_degenerate_sets(fx):
    uvzs = sc.samples(5, 300000, (480, 640))
    a = _np(sparse.interpolate_uvzs(_cuda(uvzs), (480, 640), inter_type="lstsq"))
    b = _np(sparse.interpolate_uvzs(_cuda(uvzs), (480, 640), inter_type="lstsq"))
    assert _same(a, b)
    for name, s in sc.PLANE_DEGENERATE.items():  # no unique plane: the host's minimum-norm answer, the reference's path
        assert _same(sparse.interpolate_uvzs(s, (8, 12), inter_type="lstsq"), fx["plane/" + name]), name
    got = sparse.interpolate_sparse2d(sc.sparse_image(), None, "lstsq")
    want = fx["sparse2d/lstsq"]
    assert np.abs(got.view(np.int32) - want.view(np.int32)).max() <= 1  # (<= 1 + 1/2 ulp from the exact plane between them)


# ---- triangulation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.REF_TRI_RELERR))
def test_triangulation_within_twice_the_references_error(name):
    uvs1, uvs2, K1, K2, T = sc.tri_case(name)
    e1, e2 = sr.triangulate_exact(uvs1, uvs2, K1, K2, T)
    got = sparse.matched_uvs_to_zs(uvs1, uvs2, K1, K2, T)
    assert sorted(got) == ["zs1", "zs2"] and got["zs1"].dtype == np.float64 and got["zs1"].shape == (len(uvs1),)
    err = max(sr.relerr(got["zs1"], e1), sr.relerr(got["zs2"], e2))
    print("%s: %.3g relative from the exact zs (reference %.3g)" % (name, err, sc.REF_TRI_RELERR[name]))
    assert err <= 2 * sc.REF_TRI_RELERR[name]
    gt = sparse.matched_uvs_to_zs(_cuda(uvs1), _cuda(uvs2), K1, K2, T)
    assert _same(_np(gt["zs1"]), got["zs1"]) and _same(_np(gt["zs2"]), got["zs2"])
    if name == "tri_rectified":
        d = uvs1[:, 0] - uvs2[:, 0]
        assert np.abs(got["zs1"] / (0.12 * K1[0, 0] / d) - 1).max() <= 2 * sc.REF_TRI_RELERR[name]


def test_get_depth_by_matched_uvs_uses_the_full_precision_pose():
    uvs1, uvs2, K1, K2, T = sc.tri_case("tri_rig")
    from calibrating_amd import synthetic
    st = ca.Stereo.load(synthetic.rig(640, 480))
    got = st.get_depth_by_matched_uvs(uvs1, uvs2)
    want = sparse.matched_uvs_to_zs(uvs1, uvs2, K1, K2, T)
    assert _same(got["zs1"], want["zs1"]) and _same(got["zs2"], want["zs2"])


# ---- the plugin and Stereo.get_depth ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.PLUGIN_CASES))
def test_plugin_equals_the_reference(fx, name):
    hw, kw = sc.PLUGIN_CASES[name]
    img = np.zeros(hw + (3,), np.uint8)
    res = ca.FeatureMatchingAsStereoMatching(sc.FakeFeatureMatcher(**kw))(img, img)
    assert sorted(res) == ["disparity", "matched"] and isinstance(res["disparity"], np.ndarray)
    assert res["disparity"].dtype == np.float32 and res["disparity"].shape == hw
    assert rc.sha(res["disparity"]) == str(fx["plugin/%s_sha" % name]), \
        "%d sampled values differ" % (rc.sample(res["disparity"]) != fx["plugin/" + name]).sum()
    rt = ca.FeatureMatchingAsStereoMatching(sc.FakeFeatureMatcher(device="cuda", **kw))(_cuda(img), _cuda(img))
    assert rc.sha(_np(rt["disparity"])) == str(fx["plugin/%s_sha" % name])


def _fm_stereo(device=None):
    case = sc.GET_DEPTH_CASE
    matcher = sc.FakeFeatureMatcher(device=device, **case["matcher"])
    st = ca.Stereo().load(rc.rig_record(case))
    st.set_stereo_matching(ca.FeatureMatchingAsStereoMatching(matcher), **case["setm"])
    return st, matcher


def _check(fx, res, what):
    case = sc.GET_DEPTH_CASE
    res = dict(res)
    matched = res.pop("matched")
    u1, u2 = sc.FakeFeatureMatcher(**case["matcher"]).matches()
    host = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else a  # noqa: E731
    assert sorted(matched) == ["uvs1", "uvs2"] and _same(host(matched["uvs1"]), u1) and _same(host(matched["uvs2"]), u2)
    bad, inexact = rf.check_result(fx, case, {k: host(v) for k, v in res.items()})
    assert not bad, (what, bad)
    assert not inexact, (what, "within 1e-4 m but not the reference's float64 bits", inexact)


def test_get_depth_with_the_plugin_equals_the_reference(fx):
    case = sc.GET_DEPTH_CASE
    img1, img2 = rc.images(case)
    assert rc.sha(img1) == str(fx[case["name"] + "/img1_sha"]) and rc.sha(img2) == str(fx[case["name"] + "/img2_sha"])
    # NumPy images, NumPy matches: NumPy results through the sink; the plugin itself is handed CUDA tensors
    st, matcher = _fm_stereo()
    res = st.get_depth(img1, img2)
    assert all(isinstance(v, np.ndarray) for k, v in res.items() if k != "matched")
    assert all(issubclass(a, torch.Tensor) and issubclass(b, torch.Tensor) for a, b in matcher.seen) and matcher.seen
    _check(fx, res, "get_depth(ndarray)")
    # CUDA images, CUDA matches: nothing visits the host
    st, matcher = _fm_stereo(device="cuda")
    rt = st.get_depth(_cuda(img1), _cuda(img2))
    assert matcher.seen == [(torch.Tensor, torch.Tensor)]
    assert isinstance(rt["disparity"], torch.Tensor) and rt["disparity"].is_cuda
    assert isinstance(rt["matched"]["uvs1"], torch.Tensor) and rt["matched"]["uvs1"].is_cuda
    _check(fx, rt, "get_depth(tensors)")


def test_a_plugin_without_the_attribute_still_gets_ndarrays():
    seen = []

    class Foreign(ca.MetaStereoMatching):
        def __call__(self, img1, img2):
            seen.append((type(img1), type(img2)))
            return rc.foreign_disparity(img1, img2)

    case = sc.GET_DEPTH_CASE
    st = ca.Stereo().load(rc.rig_record(case))
    st.set_stereo_matching(Foreign({}), **case["setm"])
    img1, img2 = rc.images(case)
    rt = st.get_depth(_cuda(img1), _cuda(img2))
    assert seen == [(np.ndarray, np.ndarray)] and isinstance(rt["disparity"], torch.Tensor)
