"""The LiDAR path without a GPU: the surface and its refusals (raised before a device is touched), the restatement
(tests/lidar_ref.py) against the example's own NumPy lines, against hull_ref.hull and against SciPy's KDTree, the caps of the
GPU cases (tests/lidar_cases.py), and the figure the round trip's bound rests on."""
import inspect
import os
import sys

import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import lidar, sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_ref  # noqa: E402
import lidar_cases as lc  # noqa: E402
import lidar_ref as lr  # noqa: E402
import pnp_ref  # noqa: E402


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _cam():
    return ca.Cam(lc.CLOUD_K, xy=lc.CLOUD_WH)


def test_exports_and_signatures():
    for name in ("xyzs_to_dense_depth", "uvs_on_depth_to_xyzs", "calibrate_lidar2cam"):
        assert name in ca.__all__ and getattr(ca, name) is getattr(lidar, name)
    p = inspect.signature(ca.xyzs_to_dense_depth).parameters
    assert list(p) == ["xyzs", "cam", "T", "rate", "sparse", "distance", "return_info"]
    assert (p["T"].default, p["rate"].default, p["sparse"].default, p["distance"].default, p["return_info"].default) == (None, 0.5, False, 2, False)
    assert list(inspect.signature(ca.uvs_on_depth_to_xyzs).parameters) == ["uvs_depth", "depth", "K"]
    assert list(inspect.signature(ca.calibrate_lidar2cam).parameters) == ["cam", "uvs_img", "xyzs"]
    q = inspect.signature(sparse.interpolate_uvzs_in_hull).parameters
    assert list(q) == ["uvzs", "hw", "counts", "reciprocal", "keep_last_per_pixel", "return_info", "zero_frames", "inter_type", "distance"]
    assert q["inter_type"].default == "lstsq" and q["distance"].default == 2
    assert list(inspect.signature(sparse.cloud_hull).parameters) == ["uvs"]
    assert list(inspect.signature(sparse.cloud_hull_mask).parameters) == ["uvs", "hw"]
    from calibrating_amd import _native
    for name in ("camd_cloud_to_uvzs", "camd_cloud_workspace_bytes", "camd_hull_row_range", "camd_hull_extremes", "camd_nearest_fill_in_hull"):
        assert name in _native.SIGNATURES


def test_refusals_without_a_device():
    rows = np.zeros((5000, 3))
    near = dict(inter_type="nearest")
    with pytest.raises(ValueError, match="one frame"):
        sparse.interpolate_uvzs_in_hull(np.zeros((2, 5, 3)), (8, 8), **near)
    with pytest.raises(ValueError, match="counts"):
        sparse.interpolate_uvzs_in_hull(rows, (8, 8), counts=[5000], **near)
    with pytest.raises(ValueError, match="one frame"):
        sparse.interpolate_uvzs_in_hull(np.zeros((7, 2)), (8, 8), **near)
    for kw in (dict(reciprocal=True), dict(keep_last_per_pixel=True), dict(zero_frames=np.zeros(1, bool))):
        with pytest.raises(ValueError, match="lstsq"):
            sparse.interpolate_uvzs_in_hull(rows, (8, 8), **near, **kw)
    for bad in (float("nan"), sparse.MAX_DISTANCE + 1):
        with pytest.raises(ValueError, match="distance"):
            sparse.interpolate_uvzs_in_hull(rows, (8, 8), distance=bad, **near)
        with pytest.raises(ValueError, match="distance"):
            ca.xyzs_to_dense_depth(rows, _cam(), distance=bad)
    with pytest.raises(ValueError, match="positive"):
        sparse.interpolate_uvzs_in_hull(rows, (0, 8), **near)
    with pytest.raises(ValueError, match="inter_type"):
        sparse.interpolate_uvzs_in_hull(rows[:5], (8, 8), inter_type="rbf")
    bad = rows.copy()
    bad[17, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        sparse.interpolate_uvzs_in_hull(bad, (8, 8), **near)
    # the defaults keep their limits
    with pytest.raises(ValueError, match="MAX_HULL_POINTS"):
        sparse.interpolate_uvzs_in_hull(rows, (8, 8))
    with pytest.raises(ValueError, match="MAX_HULL_POINTS"):
        sparse.convex_hull_mask(rows[:, :2], (8, 8))
    for fn in (sparse.cloud_hull, lambda u: sparse.cloud_hull_mask(u, (8, 8))):
        with pytest.raises(ValueError, match="one frame"):
            fn(np.zeros((2, 5, 2)))
        with pytest.raises(ValueError, match="one frame"):
            fn(rows)
    with pytest.raises(ValueError, match="positive"):
        sparse.cloud_hull_mask(rows[:, :2], (8, 0))
    # xyzs_to_dense_depth
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        ca.xyzs_to_dense_depth(np.zeros((5, 4)), _cam())
    with pytest.raises(ValueError, match="4x4"):
        ca.xyzs_to_dense_depth(rows, _cam(), T=np.eye(3))
    for bad in (0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="rate"):
            ca.xyzs_to_dense_depth(rows, _cam(), rate=bad)
    with pytest.raises(ValueError, match="empty grid"):
        ca.xyzs_to_dense_depth(rows, _cam(), rate=0.001)
    with pytest.raises(NotImplementedError, match="float64 resize"):
        ca.xyzs_to_dense_depth(rows, _cam(), rate=0.5, sparse=True)
    with pytest.raises(TypeError):
        ca.xyzs_to_dense_depth([[0.0, 0.0, 1.0]], _cam())
    # an empty cloud needs no device either
    got, info = ca.xyzs_to_dense_depth(np.zeros((0, 3), np.float32), _cam(), rate=None, sparse=True, return_info=True)
    assert _same(got, np.zeros((48, 64), np.float32)) and info == dict(rows=0, grid_hw=(12, 16), rate=0.25, hull_counts=0, status=1)
    assert _same(ca.xyzs_to_dense_depth(np.zeros((0, 3)), _cam()), np.zeros((48, 64), np.float32))
    # the host functions
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        ca.uvs_on_depth_to_xyzs(np.zeros((3, 3), int), np.zeros((4, 4)), lc.CLOUD_K)
    with pytest.raises(ValueError, match="whole pixels"):
        ca.uvs_on_depth_to_xyzs(np.array([[1.5, 2.0]]), np.zeros((4, 4)), lc.CLOUD_K)
    with pytest.raises(ValueError, match="leaves"):
        ca.uvs_on_depth_to_xyzs(np.array([[4, 0]]), np.zeros((4, 4)), lc.CLOUD_K)
    with pytest.raises(ValueError, match="fewer than"):
        ca.calibrate_lidar2cam(_cam(), np.zeros((3, 2)), np.zeros((3, 3)))
    with pytest.raises(ValueError, match="fewer than 6"):
        ca.calibrate_lidar2cam(_cam(), np.random.default_rng(0).uniform(0, 40, (5, 2)), np.random.default_rng(1).uniform(1, 4, (5, 3)))


def test_uvs_on_depth_to_xyzs_is_the_examples_lines():
    rng = np.random.default_rng(4)
    depth = rng.uniform(1, 9, (48, 64)).astype(np.float32)
    uvs = np.stack([rng.integers(0, 64, 12), rng.integers(0, 48, 12)], 1)
    got = ca.uvs_on_depth_to_xyzs(uvs, depth, lc.CLOUD_K_FULL)
    want = lr.uvs_on_depth_to_xyzs(uvs, depth, lc.CLOUD_K_FULL)
    assert got.dtype == np.float64 and got.shape == (12, 3) and np.abs(got - want).max() <= 4 * np.finfo(np.float64).eps * np.abs(want).max()
    # a point goes back where it came from
    K = lc.CLOUD_K
    back = ca.uvs_on_depth_to_xyzs(uvs, depth, K)
    p = back @ K.T
    assert np.allclose(p[:, :2] / p[:, 2:], uvs) and np.allclose(back[:, 2], depth[uvs[:, 1], uvs[:, 0]])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("with_T", [False, True])
def test_restatement_is_the_examples_lines_bit_for_bit_on_exact_inputs(dtype, with_T):
    """integer fx, fy, cx, cy; z a power of two; x, y multiples of 1/8; T a quarter turn plus a dyadic shift: every product and
    sum is exact, so BLAS's order and fusing cannot show and the two must agree in every bit"""
    P = lc.cloud(exact=True).astype(dtype)
    T = lc.quarter_turn_T() if with_T else None
    for rate in (1.0, 0.5, 0.25):
        got, n_pos = lr.cloud_to_uvzs(P, lc.CLOUD_K, lc.CLOUD_WH, T, rate)
        with np.errstate(all="ignore"):
            want, n_pos_want = lr.example_uvzs(P, lc.CLOUD_K, lc.CLOUD_WH, T, rate)
        assert 60 < len(got) < 280 and n_pos == n_pos_want
        assert _same(got, np.float64(want))
    # the marked rows: u == 0 and v == 0 stay, u == w and v == h go
    rows, _ = lr.cloud_to_uvzs(lc.cloud()[50:54], lc.CLOUD_K, lc.CLOUD_WH)
    assert rows.tolist() == [[0.0, 24.0, 50.0], [32.0, 0.0, 50.0]]
    assert len(lr.cloud_to_uvzs(lc.lost_cloud(), lc.CLOUD_K, lc.CLOUD_WH)[0]) == 0


def test_generic_inputs_agree_with_the_examples_lines_to_rounding():
    P, T = lc.cloud(), lc.generic_T()
    got, n_pos = lr.cloud_to_uvzs(P, lc.CLOUD_K_FULL, lc.CLOUD_WH, T, 0.5)
    with np.errstate(all="ignore"):
        want, n_pos_want = lr.example_uvzs(P, lc.CLOUD_K_FULL, lc.CLOUD_WH, T, 0.5)
    assert n_pos == n_pos_want and got.shape == want.shape and np.allclose(got, want, rtol=1e-13, atol=1e-12)
    assert lr.auto_rate(5000, 90, 162) == 0.25 and lr.auto_rate(5001, 90, 162) == (5001 / 90 / 162) ** 0.5


@pytest.mark.parametrize("name", list(lc.hull_cases()))
def test_per_row_extremes_have_the_hull_of_all_samples_and_the_cases_keep_their_caps(name):
    uvs, hw = lc.hull_cases()[name]
    vertices, rounds, table, status = lr.cloud_hull(uvs)
    want = hull_ref.hull(hull_ref.pixels(uvs))
    assert vertices == want  # the same vertices in the same order
    assert len(vertices) <= lr.MAX_HULL_POINTS
    assert np.array_equal(lr.cloud_hull_mask(uvs, hw), hull_ref.mask(uvs, hw))
    ncand = len(lr.candidates(table, 0))
    if name == "tall":
        assert ncand == 6002 and rounds == 2 and len(vertices) > 8  # really needs a second round
    else:
        assert rounds == 1 and ncand <= lr.MAX_HULL_POINTS
    if name.startswith(("many", "disc")):
        assert len(uvs) > lr.MAX_HULL_POINTS
    if name.startswith("small"):
        assert len(uvs) <= lr.MAX_HULL_POINTS
    if name.startswith("single"):
        assert (table[:, 0] == table[:, 1]).sum() >= 1  # rows that hold one sample
    assert status == (5 if name == "nobody" else 0)


def test_rounds_that_do_not_shrink_are_refused():
    circle = [(x, y) for x in range(-60, 61) for y in range(-60, 61) if 3480 <= x * x + y * y <= 3600]
    assert len(hull_ref.hull(circle)) > 16
    with pytest.raises(ValueError, match="MAX_HULL_POINTS"):
        lr.hull_in_rounds(hull_ref.hull(circle), capacity=16)
    assert lr.hull_in_rounds(circle, capacity=64)[0] == hull_ref.hull(circle)


@pytest.mark.parametrize("hw", lc.FILL_GRIDS)
@pytest.mark.parametrize("distance", lc.FILL_DISTANCES)
def test_nearest_in_hull_is_scipys_kdtree_inside_the_mask(hw, distance):
    from scipy.spatial import KDTree
    uvzs = lc.fill_case(hw)
    got, vertices, status = lr.nearest_in_hull(uvzs, hw, distance)
    h, w = hw
    ys, xs = np.mgrid[:h, :w]
    d, i = KDTree(uvzs[:, :2]).query(np.stack([xs.ravel(), ys.ravel()], 1), k=2)
    assert (d[:, 1] - d[:, 0])[d[:, 0] < distance].min() > 1e-9  # tie-free: the tree's choice is the only one
    want = np.where(d[:, 0] < distance, uvzs[i[:, 0], 2], 0).astype(np.float32).reshape(h, w)
    mask = hull_ref.mask(uvzs[:, :2], hw)
    assert _same(got, np.where(mask != 0, want, np.float32(0)))
    assert status == 0 and mask[0].sum() == 0 and mask[:, -1].sum() == 0 and 0 < mask.sum() < h * w  # whole rows are missed


def _round_trip_reference(oracle):
    uv_img, uv_depth = lc.annotated_pairs()
    depth, info = lr.xyzs_to_dense_depth(lc.plane_cloud(8000), lc.DEPTH_K, lc.DEPTH_WH, rate=0.5, resize=oracle.resize_linear)
    xyz = lr.uvs_on_depth_to_xyzs(uv_depth, depth, lc.DEPTH_K)
    res = pnp_ref.solve(xyz, uv_img, lc.DEPTH_K, lc.DEPTH_D.reshape(-1))
    return depth, xyz, res


def test_round_trip_reference_error_is_what_the_cases_record(oracle):
    depth, xyz, res = _round_trip_reference(oracle)
    assert res["status"] == 0 and (depth[lc.ANNOTATED[:, 1], lc.ANNOTATED[:, 0]] > 0).all()
    planar, _ = pnp_ref.plane_of(xyz)
    s = np.linalg.svd(xyz - xyz.mean(0), compute_uv=False)
    print("annotated points: s2 / s1 = %.3g (planar below 1e-3)" % (s[2] / s[1]))
    assert planar and s[2] / s[1] < 0.5e-3  # decidedly a plane for the solver: a margin of two
    angle, shift = lc.pose_error(res["T"], lc.lidar_pose())
    print("the restatement's round trip: %.9g rad, %.9g m from the pose that made the cloud (recorded %r)" % (angle, shift, lc.REF_ROUNDTRIP))
    assert abs(angle - lc.REF_ROUNDTRIP["angle"]) <= 1e-3 * lc.REF_ROUNDTRIP["angle"]
    assert abs(shift - lc.REF_ROUNDTRIP["shift"]) <= 1e-3 * lc.REF_ROUNDTRIP["shift"]
    assert angle > 1e-6 and shift > 1e-5  # the depth picture's own error, far above the solvers' rounding
