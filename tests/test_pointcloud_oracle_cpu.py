"""The exact C oracle of the point-cloud and z-buffer family (oracle/pointcloud_ref.c) against everything else that
states the same operations, without a GPU.  This is leg 2 of the family's parity: tests/test_gpu_zbuffer_exact.py holds
the kernels to the C oracle bit for bit (leg 1); here the C oracle is held to

  * the NumPy restatements oracle/pointcloud_ref.py and tests/reproject_ref.py (kind="stable"), whose matrix products
    are NumPy's BLAS -- a property of the machine, so this leg alone keeps the share ``reproject_cases.CAP``;
  * what the reference's own Python produced (tests/golden/reference_reproject.npz, the post/* entries of
    tests/golden/reference_plumbing.npz) -- fixed data on both sides, asserted exactly;
  * exact constructions that need no matrix product at all (tests/pointcloud_exact_cases.py).

Measured shares of bit-equal rows / pixels (x86-64, NumPy 2.2.6 with its bundled OpenBLAS), every case of this file:
  oracle vs NumPy      depth_to_point_cloud at rates 1, 1.5, 2, 0.75, 1.37 (61 492 ... 245 968 points)      1.0
                       the 5 x 300 full depth and the uint16 millimetre depth                               1.0
                       apply_T_to_point_cloud, point_cloud_to_depth of the moved cloud                      1.0
                       project_cam2_depth at interpolation 1.5, 1, 0                                        1.0
                       get_reproject_remap at rates 1, 1.5, 0.75, RATE_NATIVE, float64 and uint16 depth     1.0
                       R = I at rate 1.5 (replicated-cell ties, stable sort)                                1.0
                       point_cloud_to_arr2d, float64 / float32 / uint8 x 1, 2, 3 channels                   1.0
  oracle vs goldens    reference_reproject.npz: remap_rate1, remap_rate1.5, coloured                        1.0
                       reference_plumbing.npz: post/cloud_rate* (n, uv hash, sampled rows), cloud_mm,
                       moved, back, moved_depth, project_1.5 / 1 / 0                                        1.0
"""
import numpy as np
import pytest

from calibrating_amd import geometry
from oracle import pointcloud_ref as npref

import pointcloud_exact_cases as exact
import reference_fixture as rf
import reproject_cases as cases
import reproject_ref
from reference_fixture import rc

K = np.array([[420.0, 0, 161.3], [0, 424.0, 118.9], [0, 0, 1]])     # the rig of tests/test_gpu_pointcloud.py
ALL_RATES = (1, 1.5, 0.75, cases.RATE_NATIVE)


def _share(got, want, what):
    """Share of rows (first axis) whose every value has the same bits."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.size == 0:
        return 1.0
    a = np.ascontiguousarray(got).reshape(got.shape[0], -1)
    b = np.ascontiguousarray(want).reshape(want.shape[0], -1)
    share = (a.view(np.uint8).reshape(len(a), -1) == b.view(np.uint8).reshape(len(b), -1)).all(1).mean()
    print("%s: %.6f bit-equal" % (what, share))
    return share


def _pixels(img):
    """(h, w[, C]) or (C, h, w) maps -> one row per pixel."""
    return img.reshape(-1, 1) if img.ndim == 2 else img.reshape(-1, img.shape[-1])


def _pose_pointcloud():
    T = np.eye(4)
    T[:3, :3] = geometry.rodrigues(np.array([0.02, -0.05, 0.01]))
    T[:3, 3] = [0.06, -0.01, 0.02]
    return T


# ---- against the NumPy restatements: the share is a property of this machine's BLAS ------------------------------
@pytest.mark.parametrize("rate", [1, 1.5, 2, 0.75, 1.37])
def test_depth_to_point_cloud_equals_numpy(oracle, rate):
    depth = cases.scene_depth(1, 240, 320)
    got = oracle.depth_to_point_cloud(depth, K, rate, return_xyzuv=True)
    want = npref.depth_to_point_cloud(depth, K, interpolation_rate=rate, return_xyzuv=True)
    assert got.shape == want.shape and np.array_equal(got[:, 3:], want[:, 3:])    # no matrix product in (u, v)
    assert _share(got[:, :3], want[:, :3], "depth_to_point_cloud rate %s" % rate) >= cases.CAP
    assert np.array_equal(oracle.depth_to_point_cloud(depth, K, rate), got[:, :3])


def test_depth_to_point_cloud_edge_cases_equal_numpy(oracle):
    assert oracle.depth_to_point_cloud(np.zeros((7, 9)), K).shape == (0, 3)
    full = np.full((5, 300), 2.0)
    mm = (np.arange(12, dtype=np.uint16).reshape(3, 4) * 250)
    for name, depth in (("full", full), ("uint16", mm)):
        assert _share(oracle.depth_to_point_cloud(depth, K), npref.depth_to_point_cloud(depth, K), name) >= cases.CAP


def test_apply_T_and_point_cloud_to_depth_equal_numpy(oracle):
    cloud = npref.depth_to_point_cloud(cases.scene_depth(2, 240, 320), K)
    T = _pose_pointcloud()
    moved = npref.apply_T_to_point_cloud(T, cloud)
    assert _share(oracle.apply_T_to_point_cloud(T, cloud), moved, "apply_T") >= cases.CAP
    extra = np.concatenate([cloud, np.arange(len(cloud))[:, None] * 1.0, cloud[:, :1]], 1)      # rows of 5
    got = oracle.apply_T_to_point_cloud(T, extra)
    assert np.array_equal(got[:, 3:], extra[:, 3:]) and np.array_equal(got[:, :3], oracle.apply_T_to_point_cloud(T, cloud))
    for name, pts in (("identity", cloud), ("moved", moved)):
        got = oracle.point_cloud_to_depth(pts, K, (320, 240))
        assert _share(_pixels(got), _pixels(npref.point_cloud_to_depth(pts, K, (320, 240))), "to_depth " + name) >= cases.CAP
    # rows of 5 columns: the stride is the row length
    assert np.array_equal(oracle.point_cloud_to_depth(extra, K, (320, 240)), oracle.point_cloud_to_depth(cloud, K, (320, 240)))
    pts = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 1.0], [0.0, 0.0, -3.0], [50.0, 0.0, 1.0], [0.1, 0.1, 0.0], [0.2, -0.1, 4.0]])
    want = npref.point_cloud_to_depth(pts[[0, 1, 2, 3, 5]], K, (320, 240), bg_value=-1)   # z = 0 divides by zero there
    assert np.array_equal(oracle.point_cloud_to_depth(pts, K, (320, 240), bg_value=-1), want)


@pytest.mark.parametrize("interpolation", [1.5, 1, 0])
def test_project_depth_equals_numpy(oracle, interpolation):
    rate = npref.interpolation_rate(cases.K1, cases.K2, interpolation)
    d2, T = cases.depth2(), cases.pose()
    got = oracle.project_depth(d2, cases.K2, T, cases.K1, cases.XY1, rate)
    want = npref.project_cam2_depth(cases.K1, cases.XY1, cases.K2, d2, T, interpolation=interpolation)
    assert _share(_pixels(got), _pixels(want), "project_depth interpolation %s" % interpolation) >= cases.CAP


@pytest.mark.parametrize("rate", ALL_RATES)
def test_get_reproject_remap_equals_numpy_and_the_reference_run(oracle, rate):
    d2, T = cases.depth2(), cases.pose()
    got = oracle.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, rate)
    want = reproject_ref.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, rate, kind="stable")
    assert _share(_pixels(got.transpose(1, 2, 0)), _pixels(want.transpose(1, 2, 0)), "remap rate %s" % rate) >= cases.CAP
    if rate in cases.GOLDEN_RATES:       # fixed data on both sides: exactly what was measured
        fx = cases.load_fixture()
        assert fx is not None, "tests/golden/reference_reproject.npz is missing"
        assert got.tobytes() == fx["remap_rate%s" % rate].tobytes()
    mm = np.uint16(np.round(d2 * 1000))
    got = oracle.get_reproject_remap(cases.K1, cases.K2, T, mm, cases.XY1, rate)
    want = reproject_ref.get_reproject_remap(cases.K1, cases.K2, T, mm, cases.XY1, rate, kind="stable")
    assert _share(_pixels(got.transpose(1, 2, 0)), _pixels(want.transpose(1, 2, 0)), "uint16, rate %s" % rate) >= cases.CAP


def test_tie_rule_equals_the_stable_sort(oracle):
    """R = I at rate 1.5: more than 10 000 points share a pixel and a bit-equal z with another one."""
    d2, T = cases.depth2(), cases.pose(rotated=False)
    got = oracle.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, 1.5)
    want = reproject_ref.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, 1.5, kind="stable")
    assert _share(_pixels(got.transpose(1, 2, 0)), _pixels(want.transpose(1, 2, 0)), "R = I, rate 1.5") >= cases.CAP


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.uint8])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_point_cloud_to_arr2d_equals_numpy(oracle, dtype, channels):
    cloud, _ = cases.coloured_cloud()
    rng = np.random.default_rng(channels * 10 + np.dtype(dtype).itemsize)
    if dtype == np.uint8:
        values, bg = rng.integers(0, 256, (len(cloud), channels)).astype(np.uint8), 7
    else:
        values, bg = rng.standard_normal((len(cloud), channels)).astype(dtype), -2.5
    want = reproject_ref.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=values, bg_value=bg, kind="stable")
    for v in ((values, values[:, 0]) if channels == 1 else (values,)):
        got = oracle.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=v, bg_value=bg)
        assert _share(_pixels(got), _pixels(want), "arr2d %s x%d" % (np.dtype(dtype).name, channels)) >= cases.CAP


# ---- against the reference's recorded runs: fixed data on both sides, exact ---------------------------------------
def test_coloured_cloud_equals_the_reference_run(oracle):
    fx = cases.load_fixture()
    assert fx is not None, "tests/golden/reference_reproject.npz is missing"
    cloud, colours = cases.coloured_cloud()
    got = oracle.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=colours, bg_value=7)
    assert got.dtype == np.uint8 and got.tobytes() == fx["coloured"].tobytes()


@pytest.mark.parametrize("rate", rc.POST_RATES)
def test_depth_to_point_cloud_equals_the_reference_run(oracle, rate):
    fx = rf.fixture()
    depth = rc.post_depth(1, rc.POST_XY1[1], rc.POST_XY1[0])
    got = oracle.depth_to_point_cloud(depth, rc.POST_K1, rate, return_xyzuv=True)
    assert len(got) == int(fx["post/cloud_rate%s_n" % rate])
    assert rc.sha(got[:, 3:]) == str(fx["post/cloud_rate%s_uv_sha" % rate])
    assert got[::rc.CLOUD_ROWS].tobytes() == fx["post/cloud_rate%s" % rate].tobytes()


def test_scatter_and_projection_equal_the_reference_run(oracle):
    fx = rf.fixture()
    mm = (np.arange(12, dtype=np.uint16).reshape(3, 4) * 250)
    assert oracle.depth_to_point_cloud(mm, rc.POST_K1).tobytes() == fx["post/cloud_mm"].tobytes()
    cloud = oracle.depth_to_point_cloud(rc.post_depth(2, rc.POST_XY1[1], rc.POST_XY1[0]), rc.POST_K1)
    moved = oracle.apply_T_to_point_cloud(rc.post_T(), cloud)
    assert moved[::rc.CLOUD_ROWS].tobytes() == fx["post/moved"].tobytes()
    s = rc.POST_SAMPLE
    assert rc.sample(oracle.point_cloud_to_depth(cloud, rc.POST_K1, rc.POST_XY1), s).tobytes() == fx["post/back"].tobytes()
    assert rc.sample(oracle.point_cloud_to_depth(moved, rc.POST_K1, rc.POST_XY1), s).tobytes() == \
        fx["post/moved_depth"].tobytes()
    depth3 = rc.post_depth(3, rc.POST_XY2[1], rc.POST_XY2[0])
    for interp in rc.POST_INTERPOLATIONS:
        rate = npref.interpolation_rate(rc.POST_K1, rc.POST_K2, interp)
        got = oracle.project_depth(depth3, rc.POST_K2, fx["post/T2"], rc.POST_K1, rc.POST_XY1, rate)
        assert rc.sample(got, s).tobytes() == fx["post/project_%s" % interp].tobytes(), interp


# ---- exact constructions: no matrix product of NumPy's ------------------------------------------------------------
def test_half_to_even_and_the_image_edges(oracle):
    owner, zs = oracle.zbuffer_points(exact.half_points(), exact.HALF_K, exact.XY)
    want = np.full((exact.XY[1], exact.XY[0]), -1, np.int64)
    for i, (_, _, pixel) in enumerate(exact.HALF_CASES):
        if pixel is not None:
            want[pixel[1], pixel[0]] = i
    assert np.array_equal(owner, want)
    assert np.array_equal(zs, np.where(want >= 0, 1.0, 0.0))


def test_negative_z_wins_and_z_ordering(oracle):
    x, y = exact.CENTRE_PIXEL
    zs_all = exact.Z_ASCENDING
    assert all(a < b for a, b in zip(zs_all, zs_all[1:]))
    for first in range(len(zs_all)):
        tail = zs_all[first:]                       # its smallest value must win, wherever it stands in the cloud
        for order in (tail, tail[::-1], tail[1:] + tail[:1]):
            owner, zs = oracle.zbuffer_points(exact.centre_points(order), exact.CENTRE_K, exact.XY)
            assert (owner >= 0).sum() == 1 and owner[y, x] == order.index(tail[0]), (first, order)
            assert zs[y, x].tobytes() == np.float64(tail[0]).tobytes()
    # bit-equal ties: the later row wins
    owner, _ = oracle.zbuffer_points(exact.centre_points([2.0, 1.0, 1.0, 3.0, 1.0, 2.0]), exact.CENTRE_K, exact.XY)
    assert owner[y, x] == 4


def test_dropped_points(oracle):
    pts = np.concatenate([exact.DROPPED, exact.KEPT_AMONG_DROPPED[None], exact.DROPPED])
    with np.errstate(all="ignore"):
        owner, zs = oracle.zbuffer_points(pts, exact.CENTRE_K, exact.XY)
    x, y = exact.KEPT_PIXEL
    assert (owner >= 0).sum() == 1 and owner[y, x] == len(exact.DROPPED) and zs[y, x] == 2.0
    depth = oracle.point_cloud_to_depth(pts, exact.CENTRE_K, exact.XY, bg_value=-7)
    assert (depth == -7).sum() == depth.size - 1 and depth[y, x] == 2.0


def test_contention_clouds_have_the_ties_they_are_for(oracle):
    for spread, Km, xy in ((False, exact.CENTRE_K, exact.XY), (True, exact.SPREAD_K, exact.SPREAD_XY)):
        cloud = exact.contention_cloud(spread)
        owner, zs = oracle.zbuffer_points(cloud, Km, xy)
        hit = owner >= 0
        assert hit.sum() == (16 if spread else 1) and (zs[hit] == 1.0).all()
        for o in owner[hit]:            # the winner is the LAST of many points with z == 1.0 on its pixel
            same = (cloud == cloud[o]).all(1)
            assert same.sum() > (100 if spread else 3000) and np.nonzero(same)[0].max() == o
