"""The LiDAR path on the GPU (-m gpu): csrc/lidar.hip through calibrating_amd.sparse and calibrating_amd.lidar against
tests/lidar_ref.py, bit for bit -- rows, counters, the extremes table, the hull's vertices, the mask, the fill, the final
depth, the status.  The cases are tests/lidar_cases.py's; tests/test_lidar_cpu.py holds them to their caps.  The round trip
(cloud -> depth picture -> annotated pairs -> T) may err at most twice what the NumPy restatement of the same steps does
on that case: lidar_cases.REF_ROUNDTRIP, 2.06592074e-06 rad and 1.45255799e-05 m, measured on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

import calibrating_amd as ca
from calibrating_amd import _native, sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_ref  # noqa: E402
import lidar_cases as lc  # noqa: E402
import lidar_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1a ------------------------------------------------------------------------------------------------------------------
def _rows(pts, stride, n, K, wh, T, rate, stages=3):
    """camd_cloud_to_uvzs through the raw entry: (rows, kept, n_positive)"""
    ws = torch.empty(max(8, _native.lib().camd_cloud_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    counters = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    rows = torch.full((n + 1, 3), -7.0, dtype=torch.float64, device="cuda")
    K = np.ascontiguousarray(K, np.float64)
    T = None if T is None else np.ascontiguousarray(T, np.float64)
    vt = _native.VALUE_F64 if pts.dtype == torch.float64 else _native.VALUE_F32
    for s in ((1, 2) if stages == 12 else (stages,)):
        _native.call("camd_cloud_to_uvzs", pts.device, pts.data_ptr(), vt, n, stride, None if T is None else T.ctypes.data,
                     K.ctypes.data, wh[0], wh[1], rate, s, rows.data_ptr(), n, counters.data_ptr(), ws.data_ptr())
    kept, n_pos = (int(x) for x in counters.cpu().numpy())
    out = rows.cpu().numpy()
    assert (out[kept:] == -7.0).all()  # nothing is written beyond the count
    return out[:kept], kept, n_pos


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("with_T", [False, True])
def test_cloud_to_uvzs_rows_and_counters(dtype, with_T):
    P = lc.cloud().astype(dtype)
    T = lc.generic_T() if with_T else None
    for K, rate in ((lc.CLOUD_K, 1.0), (lc.CLOUD_K_FULL, 0.37)):
        want, n_pos = lr.cloud_to_uvzs(P, K, lc.CLOUD_WH, T, rate)
        got, kept, got_pos = _rows(_cuda(P), 3, len(P), K, lc.CLOUD_WH, T, rate)
        assert 100 < len(want) < len(P) and (kept, got_pos) == (len(want), n_pos) and _same(got, want)
        # count, then emit: the same rows
        again, _, _ = _rows(_cuda(P), 3, len(P), K, lc.CLOUD_WH, T, rate, stages=12)
        assert _same(again, want)
        # the column view of an (n, 4) array, read in place
        wide = _cuda(np.concatenate([np.full((len(P), 1), 99, dtype), P], 1))
        view, _, _ = _rows(wide[:, 1:], 4, len(P), K, lc.CLOUD_WH, T, rate)
        assert _same(view, want)


def test_cloud_rows_at_the_image_border_and_a_cloud_that_loses_every_row():
    got, kept, n_pos = _rows(_cuda(lc.cloud()[50:54]), 3, 4, lc.CLOUD_K, lc.CLOUD_WH, None, 1.0)
    assert got.tolist() == [[0.0, 24.0, 50.0], [32.0, 0.0, 50.0]] and (kept, n_pos) == (2, 4)  # u == 0, v == 0 stay; u == w, v == h go
    lost = lc.lost_cloud()
    got, kept, n_pos = _rows(_cuda(lost), 3, len(lost), lc.CLOUD_K, lc.CLOUD_WH, None, 0.5)
    assert kept == 0 and n_pos == lr.cloud_to_uvzs(lost, lc.CLOUD_K, lc.CLOUD_WH)[1] == 100
    cam = ca.Cam(lc.CLOUD_K, xy=lc.CLOUD_WH)
    for sp, dt in ((False, np.float32), (True, np.float64)):
        depth, info = ca.xyzs_to_dense_depth(lost, cam, rate=1, sparse=sp, return_info=True)
        assert _same(depth, np.zeros((48, 64), dt)) and info == dict(rows=0, grid_hw=(48, 64), rate=1.0, hull_counts=0, status=1)
    none, info = ca.xyzs_to_dense_depth(lost, cam, rate=None, return_info=True)
    assert _same(none, np.zeros((48, 64), np.float32)) and info["rate"] == 0.25 and info["grid_hw"] == (12, 16)


# ---- 1b ------------------------------------------------------------------------------------------------------------------
HULLS = lc.hull_cases()


@pytest.mark.parametrize("name", list(HULLS))
def test_hull_of_any_number_of_samples(name):
    uvs, hw = HULLS[name]
    want_v, rounds, want_table, want_status = lr.cloud_hull(uvs)
    uv = _cuda(uvs)
    rec = sparse._cloud_hull_record(uv, 2, len(uvs))
    lo, hi, _ = lr.row_range(uvs)
    assert rec["rows_range"] == ((lo, hi - lo + 1) if lo <= hi else (0, 1))
    assert _same(rec["table"].cpu().numpy(), want_table)
    assert int(rec["status"].item()) == want_status
    k = int(rec["hull_counts"].item())
    assert [tuple(int(c) for c in p) for p in rec["vertices"][0, :k].cpu().numpy()] == want_v
    got_v = sparse.cloud_hull(uvs)
    assert got_v.dtype == np.int32 and _same(got_v, np.array(want_v, np.int32).reshape(-1, 2))
    want_mask = hull_ref.mask_of_hull(want_v, hw)
    mask = sparse.cloud_hull_mask(uvs, hw)
    assert mask.dtype == np.uint8 and _same(mask, want_mask)
    assert _same(sparse.cloud_hull_mask(uv, hw).cpu().numpy(), want_mask) and _same(sparse.cloud_hull(uv).cpu().numpy(), got_v)
    if len(uvs) <= sparse.MAX_HULL_POINTS:
        assert _same(mask, sparse.convex_hull_mask(uvs, hw))
    if name == "tall":
        assert rounds == 2 and want_mask.sum() > 3001


def test_a_round_that_does_not_shrink_is_refused():
    """more than MAX_HULL_POINTS hull vertices: the polygon whose edges are all primitive vectors (a, b), |a|, |b| <= 45, by angle
    -- every corner is a strict vertex, so the second round cannot drop one"""
    uvs = lc.many_vertex_polygon()
    assert len(uvs) > sparse.MAX_HULL_POINTS and np.abs(uvs).max() < 2 ** 20
    with pytest.raises(ValueError, match="MAX_HULL_POINTS"):
        sparse.cloud_hull(uvs)


# ---- 1c ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", lc.FILL_GRIDS)
@pytest.mark.parametrize("distance", lc.FILL_DISTANCES)
def test_nearest_fill_inside_the_hull(hw, distance):
    uvzs = lc.fill_case(hw)
    want, vertices, status = lr.nearest_in_hull(uvzs, hw, distance)
    got, info = sparse.interpolate_uvzs_in_hull(uvzs, hw, inter_type="nearest", distance=distance, return_info=True)
    assert got.dtype == np.float32 and _same(got, want)
    assert int(info["status"]) == status == 0 and int(info["hull_counts"]) == len(vertices)
    # the definition: the unconstrained fill times the mask
    full = sparse.interpolate_uvzs(uvzs, hw, None, "nearest", distance)
    assert _same(got, np.where(sparse.cloud_hull_mask(uvzs[:, :2].copy(), hw) != 0, full, np.float32(0)))
    assert (want[0] == 0).all() and (full != 0).sum() >= (got != 0).sum() + (distance == 7)  # the plain fill reaches beyond the hull
    # CUDA in -> CUDA out; float32 rows: the values of float32 z at float64 copies of u, v
    dev = sparse.interpolate_uvzs_in_hull(_cuda(uvzs), hw, inter_type="nearest", distance=distance)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and _same(dev.cpu().numpy(), want)
    r32 = uvzs.astype(np.float32)
    assert _same(sparse.interpolate_uvzs_in_hull(r32, hw, inter_type="nearest", distance=distance),
                 lr.nearest_in_hull(r32, hw, distance)[0])


def test_nearest_fill_of_many_samples_and_of_none():
    uvs, hw = HULLS["many_37x70"]
    uvzs = np.concatenate([uvs, np.random.default_rng(1).uniform(1, 9, (len(uvs), 1))], 1)
    want, vertices, status = lr.nearest_in_hull(uvzs, hw, 2)
    got, info = sparse.interpolate_uvzs_in_hull(uvzs, hw, inter_type="nearest", return_info=True)
    assert len(uvzs) > sparse.MAX_HULL_POINTS and _same(got, want) and int(info["hull_counts"]) == len(vertices)
    empty, info = sparse.interpolate_uvzs_in_hull(np.zeros((0, 3)), hw, inter_type="nearest", return_info=True)
    assert _same(empty, np.zeros(hw, np.float32)) and int(info["status"]) == 1 and int(info["hull_counts"]) == 0
    far, info = sparse.interpolate_uvzs_in_hull(np.array([[2.0 ** 21, 3.0, 1.0]]), hw, inter_type="nearest", return_info=True)
    assert _same(far, np.zeros(hw, np.float32)) and int(info["status"]) == 5


# ---- xyzs_to_dense_depth ---------------------------------------------------------------------------------------------------
def _cam():
    return ca.Cam(lc.DEPTH_K, lc.DEPTH_D, xy=lc.DEPTH_WH)


@pytest.mark.parametrize("n", [3000, 8000])
@pytest.mark.parametrize("rate", [0.5, 1, None])
def test_dense_depth_bit_for_bit(oracle, n, rate):
    cam, T = _cam(), lc.lidar_pose()
    P = lc.plane_cloud(n, seed=n)
    for kw in (dict(), dict(T=T)):
        want, winfo = lr.xyzs_to_dense_depth(P, lc.DEPTH_K, lc.DEPTH_WH, kw.get("T"), rate, resize=oracle.resize_linear)
        got, info = ca.xyzs_to_dense_depth(P, cam, rate=rate, return_info=True, **kw)
        assert got.dtype == np.float32 and got.shape == (90, 162) and _same(got, want)
        assert info == winfo, (info, winfo)
        assert (rate is not None) or ((info["rate"] == 0.25) == (n == 3000))  # both sides of 5 000 points
    dev = ca.xyzs_to_dense_depth(_cuda(P), cam, T=T, rate=rate)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and _same(dev.cpu().numpy(), want)
    # sparse: the scatter in the cloud's dtype; float64 only at the camera's own size
    P32 = P.astype(np.float32)
    want32, winfo = lr.xyzs_to_dense_depth(P32, lc.DEPTH_K, lc.DEPTH_WH, T, rate, sparse=True, resize=oracle.resize_linear)
    got32, info = ca.xyzs_to_dense_depth(P32, cam, T, rate, True, return_info=True)
    assert got32.dtype == np.float32 and _same(got32, want32) and info == winfo
    assert _same(ca.xyzs_to_dense_depth(_cuda(P32), cam, T, rate, True).cpu().numpy(), want32)
    if rate == 1:
        want64, _ = lr.xyzs_to_dense_depth(P, lc.DEPTH_K, lc.DEPTH_WH, T, rate, sparse=True)
        assert _same(ca.xyzs_to_dense_depth(P, cam, T, rate, sparse=True), want64) and want64.dtype == np.float64
    else:
        with pytest.raises(NotImplementedError, match="float64 resize"):
            ca.xyzs_to_dense_depth(P, cam, T, rate, sparse=True)


def test_round_trip_cloud_to_depth_picture_to_pose():
    """the example's flow in this package's names; the bound is twice the restatement's own error (lidar_cases.REF_ROUNDTRIP)"""
    cam, pinhole = _cam(), ca.Cam(lc.DEPTH_K, xy=lc.DEPTH_WH)
    cloud = lc.plane_cloud(8000)
    depth = ca.xyzs_to_dense_depth(cloud, pinhole)                       # the depth picture to annotate
    assert ca.vis_depth(depth).shape[:2] == (90, 162)
    uv_img, uv_depth = lc.annotated_pairs()
    xyz = ca.uvs_on_depth_to_xyzs(uv_depth, depth, pinhole.K)
    res = ca.calibrate_lidar2cam(cam, uv_img, xyz)
    angle, shift = lc.pose_error(res["T"], lc.lidar_pose())
    print("round trip: %.9g rad, %.9g m from the pose that made the cloud; the restatement: %r" % (angle, shift, lc.REF_ROUNDTRIP))
    assert res["status"] == 0 and angle <= 2 * lc.REF_ROUNDTRIP["angle"] and shift <= 2 * lc.REF_ROUNDTRIP["shift"]
    # the cloud through the solved pose: the sparse depth the example overlays on the photo
    check = ca.xyzs_to_dense_depth(cloud, pinhole, T=res["T"], rate=1, sparse=True)
    want, _ = lr.xyzs_to_dense_depth(cloud, lc.DEPTH_K, lc.DEPTH_WH, res["T"], 1, sparse=True)
    assert _same(check, want) and (check > 0).sum() > 3000
