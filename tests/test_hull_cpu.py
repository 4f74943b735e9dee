"""The hull fill without a GPU: the restatement of its mask contract (tests/hull_ref.py) against a brute-force definition,
the figures of tests/hull_cases.py, the new surface and its refusals, and the old refusal, which stays."""
import itertools
import os
import sys

import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_cases as hc  # noqa: E402
import hull_ref  # noqa: E402


def _brute_mask(points, hw):
    """The definition: a pixel is inside iff it is a sample, or lies on a segment between two samples, or lies in a
    (closed) triangle of three samples -- all in Python integers."""
    pts = sorted(set(points))
    out = np.zeros(hw, np.uint8)
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])  # noqa: E731
    for y in range(hw[0]):
        for x in range(hw[1]):
            p = (x, y)
            inside = p in pts
            if not inside:
                for a, b in itertools.combinations(pts, 2):
                    if cross(a, b, p) == 0 and min(a[0], b[0]) <= x <= max(a[0], b[0]) and min(a[1], b[1]) <= y <= max(a[1], b[1]):
                        inside = True
                        break
            if not inside:
                for a, b, c in itertools.combinations(pts, 3):
                    s = (cross(a, b, p), cross(b, c, p), cross(c, a, p))
                    if cross(a, b, c) != 0 and (all(v >= 0 for v in s) or all(v <= 0 for v in s)):
                        inside = True
                        break
            out[y, x] = inside
    return out


def _seeded_sets():
    rng = np.random.default_rng(2024)
    for k in range(300):
        h, w = int(rng.integers(1, 17)), int(rng.integers(1, 17))
        n = int(rng.integers(1, 8))
        kind = k % 4
        if kind == 0:  # anywhere, also outside the image
            pts = [(int(rng.integers(-4, w + 4)), int(rng.integers(-4, h + 4))) for _ in range(n)]
        elif kind == 1:  # with duplicates
            base = [(int(rng.integers(0, w)), int(rng.integers(0, h))) for _ in range(max(1, n // 2))]
            pts = [base[int(rng.integers(len(base)))] for _ in range(n)]
        elif kind == 2:  # collinear
            dx, dy = int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            pts = [(x0 + int(t) * dx, y0 + int(t) * dy) for t in rng.integers(-3, 4, n)]
        else:  # a collinear run plus one point beside it
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            pts = [(x0 + t, y0 + 2 * t) for t in range(-2, 3)] + [(int(rng.integers(0, w)), int(rng.integers(0, h)))]
        yield pts, (h, w)


def test_restatement_equals_the_brute_force_definition():
    for pts, hw in _seeded_sets():
        rows = np.array(pts, np.float64)
        got = hull_ref.mask(rows, hw)
        assert np.array_equal(got, _brute_mask(pts, hw)), (pts, hw)
        v = hull_ref.hull(pts)
        assert len(set(v)) == len(v) and set(v) <= set(pts)


def test_restatement_rounding_validity_and_keep_last():
    rows = np.array([[0.5, 1.5, 1.0], [2.5, 3.5, 1.0], [np.nan, 0, 1.0], [1, 1, 0.0], [1, 1, np.inf], [2.0 ** 20 + 1, 0, 1.0]])
    assert hull_ref.pixels(rows) == [(0, 2), (2, 4)]  # half to even; invalid rows take no part
    assert hull_ref.mask(hc.INVALID, hc.HW).sum() == 0
    d, hw, _ = hc.PLANE_FRAMES["duplicates"]
    assert list(hull_ref.valid_rows(d, hw, True)) == [1, 3 + 1, 5, 6, 8]  # the last of each pixel, inside the image
    assert len(hull_ref.valid_rows(d, hw, False)) == len(d)


@pytest.mark.parametrize("name", [k for k in hc.PLANE_FRAMES if k not in hc.SAMPLED and k != "big4096"])
def test_reference_plane_error_is_what_the_cases_record(name):
    got = hc.reference_ulps(name)
    print("%s: the reference's own formula lies %.6g float32 ulps from the exact plane (recorded %.6g)" % (name, got, hc.REF_PLANE_ULPS[name]))
    assert got <= 0.5 + 1e-6 and abs(got - hc.REF_PLANE_ULPS[name]) < 5e-3


def test_board_reference_error_is_what_the_cases_record():
    for pose, want in hc.REF_BOARD_RELERR.items():
        got = hc.board_reference_relerr(pose)
        print("pose %d: the composition lies %.6g from the closed form (recorded %.6g)" % (pose, got, want))
        assert abs(got - want) <= 1e-3 * want


def test_surface_without_a_gpu():
    for name in ("convex_hull_mask", "interpolate_uvzs_in_hull", "interpolate_sparse2d_in_hull", "MAX_HULL_POINTS"):
        assert hasattr(sparse, name), name
    assert sparse.MAX_HULL_POINTS == 4096
    for name in ("get_board", "get_calibration_board_T", "get_calibration_board_depth", "get_calibration_board_depth_batch"):
        assert hasattr(ca.Cam, name), name
    assert "MatchingByBoard" in ca.__all__ and ca.MatchingByBoard.accepts_device_tensors is True
    assert issubclass(ca.MatchingByBoard, ca.MetaStereoMatching)
    m = ca.MatchingByBoard("board", dense_predict=False)
    assert m.board == "board" and m.dense_predict is False
    # refused before the device is touched (this machine may have none)
    big = np.zeros((sparse.MAX_HULL_POINTS + 1, 3))
    with pytest.raises(ValueError, match="MAX_HULL_POINTS"):
        sparse.interpolate_uvzs_in_hull(big, (8, 8))
    with pytest.raises(ValueError, match="MAX_HULL_POINTS"):
        sparse.interpolate_uvzs_in_hull(np.zeros((2, sparse.MAX_HULL_POINTS + 1, 3)), (8, 8))
    with pytest.raises(ValueError, match="MAX_HULL_POINTS"):
        sparse.interpolate_uvzs_in_hull(big, (8, 8), counts=[0, sparse.MAX_HULL_POINTS + 1])
    with pytest.raises(ValueError, match="MAX_HULL_POINTS"):
        sparse.convex_hull_mask(big[:, :2], (8, 8))
    with pytest.raises(ValueError, match="MAX_HULL_POINTS"):
        sparse.interpolate_sparse2d_in_hull(np.ones((80, 80)))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        sparse.interpolate_uvzs_in_hull(np.zeros((4, 2)), (8, 8))
    with pytest.raises(ValueError, match="counts"):
        sparse.interpolate_uvzs_in_hull(np.zeros((4, 3)), (8, 8), counts=[1, 2])
    with pytest.raises(ValueError, match="positive"):
        sparse.interpolate_uvzs_in_hull(np.zeros((4, 3)), (0, 8))
    with pytest.raises(ValueError, match="zero_frames"):
        sparse.interpolate_uvzs_in_hull(np.zeros((4, 3)), (8, 8), zero_frames=np.zeros(1, bool))
    with pytest.raises(ValueError, match=r"\(h, w\)"):
        sparse.interpolate_sparse2d_in_hull(np.zeros((4, 4, 3)))
    cam = ca.Cam(np.array([[100.0, 0, 32], [0, 100.0, 24], [0, 0, 1]]), xy=(64, 48))
    with pytest.raises(ValueError, match="not read from paths"):
        cam.get_calibration_board_T("frame.png", board=ca.Chessboard((4, 3)))
    with pytest.raises(ValueError, match="not read from paths"):
        cam.get_calibration_board_depth(dict(path="frame.png"), board=ca.Chessboard((4, 3)))
    with pytest.raises(ValueError, match="images must be"):
        cam.get_calibration_board_depth_batch(np.zeros((2, 10, 10), np.uint8), board=ca.Chessboard((4, 3)))
    with pytest.raises(AssertionError, match="board"):
        cam.get_board(None, None)


def test_the_old_refusal_stays():
    uvzs = np.array([[1.0, 2.0, 3.0], [4.0, 1.0, 2.0], [2.0, 5.0, 1.0]])
    for constrained in (True, "convex_hull", 1):
        with pytest.raises(NotImplementedError, match="convexHull"):
            sparse.interpolate_uvzs(uvzs, (8, 8), constrained_type=constrained)
        with pytest.raises(NotImplementedError, match="convexHull"):
            sparse.interpolate_sparse2d(np.eye(4), constrained)
