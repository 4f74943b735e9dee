"""The plane inside the samples' convex hull on the GPU (-m gpu): csrc/hull.hip through calibrating_amd.sparse against the
restatement of its own contract (tests/hull_ref.py).  The mask and the hull's vertex set are compared bit for bit; the
plane inside the hull by the rule of the existing plane tests, kept as it stands (tests/hull_cases.py: float32 ulps from
the exact plane, at most max(1, 2 x the reference's own distance)); the degenerate planes of the (n, 3) form bit for bit
with sparse_ref.plane.  Plain imports: a missing feature fails."""
import os
import sys

import numpy as np
import pytest
import torch

from calibrating_amd import _native, sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_cases as hc  # noqa: E402
import hull_ref  # noqa: E402
import sparse_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _vertices(rows, hw, keep_last):
    """the vertex set of stage A's record for one frame"""
    rows = np.ascontiguousarray(rows, np.float64)
    n = len(rows)
    uv, z = _cuda(rows[:, :2]), _cuda(rows[:, 2])
    cap = max(1, n)
    verts = torch.full((cap, 2), -7, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    abc = torch.zeros(3, dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    _native.call("camd_hull_fit", uv.device, uv.data_ptr(), 2, z.data_ptr(), _native.VALUE_F64, n, None, 1, hw[1], hw[0],
                 int(keep_last), cap, verts.data_ptr(), count.data_ptr(), abc.data_ptr(), status.data_ptr())
    k = int(count.item())
    v = verts.cpu().numpy()
    assert (v[k:] == -7).all()  # nothing is written beyond the count
    return [tuple(int(c) for c in p) for p in v[:k]]


def _check_mask_and_hull(rows, hw, keep_last=False):
    want = hull_ref.mask(rows, hw, keep_last)
    got, info = sparse.interpolate_uvzs_in_hull(rows, hw, keep_last_per_pixel=keep_last, return_info=True)
    assert got.dtype == np.float32 and got.shape == tuple(hw)
    outside = got[want == 0]
    assert _same(outside, np.zeros_like(outside))  # +0.0 outside
    assert np.array_equal((got != 0) | np.isnan(got), want != 0)  # (no case's plane passes through 0 inside its hull)
    v = _vertices(rows, hw, keep_last)
    ref_v = hull_ref.hull(hull_ref.pixels(rows, hw, keep_last))
    assert len(v) == len(set(v)) == int(info["hull_counts"]) and set(v) == set(ref_v)
    if not keep_last:
        m = sparse.convex_hull_mask(np.ascontiguousarray(rows[:, :2]), hw)
        assert m.dtype == np.uint8 and _same(m, want)
        assert _same(sparse.convex_hull_mask(_cuda(rows[:, :2]), hw).cpu().numpy(), want)
    return got, want, info


@pytest.mark.parametrize("name", list(hc.PLANE_FRAMES))
def test_mask_bit_equal_and_plane_within_twice_the_references_error(name):
    rows, hw, keep = hc.PLANE_FRAMES[name]
    got, mask, info = _check_mask_and_hull(rows, hw, keep)
    assert int(info["status"]) == 0
    part = rows[hull_ref.valid_rows(rows, hw, keep)]
    ulps = hc.ulps_inside(got, sr.plane_exact(part), mask, hc.SAMPLED.get(name, 1))
    allowed = max(1.0, 2 * hc.REF_PLANE_ULPS[name])
    print("%s: %.6g float32 ulps from the exact plane (reference %.6g, allowed %.6g)" % (name, ulps, hc.REF_PLANE_ULPS[name], allowed))
    assert ulps <= allowed
    inside = mask != 0
    # CUDA in -> CUDA out, a second run: the same bits; float32 rows: the bits of their float64 copies
    again = sparse.interpolate_uvzs_in_hull(_cuda(rows), hw, keep_last_per_pixel=keep)
    assert isinstance(again, torch.Tensor) and again.is_cuda and _same(again.cpu().numpy(), got)
    r32 = rows.astype(np.float32)
    assert _same(sparse.interpolate_uvzs_in_hull(r32, hw, keep_last_per_pixel=keep),
                 sparse.interpolate_uvzs_in_hull(r32.astype(np.float64), hw, keep_last_per_pixel=keep))
    # reciprocal: float32 1 / x of the plain output, +inf outside the hull
    rec = sparse.interpolate_uvzs_in_hull(rows, hw, reciprocal=True, keep_last_per_pixel=keep)
    with np.errstate(divide="ignore"):
        assert _same(rec, np.float32(1) / got)
    assert np.isposinf(rec[~inside]).all()
    if hw[0] * hw[1] <= 4096 and not keep:  # the image form: the samples scattered, then filled
        img = sr.scatter(rows[:, :2], rows[:, 2], hw)
        want_rows = sr.rows_of(img, (img != 0) & np.isfinite(img))
        assert _same(sparse.interpolate_sparse2d_in_hull(img), sparse.interpolate_uvzs_in_hull(want_rows, hw))
        assert _same(sparse.interpolate_sparse2d_in_hull(_cuda(img), reciprocal=True).cpu().numpy(),
                     sparse.interpolate_uvzs_in_hull(want_rows, hw, reciprocal=True))


def test_keep_last_per_pixel_changes_the_fit_and_the_hull():
    rows, hw, _ = hc.PLANE_FRAMES["duplicates"]
    a, ia = sparse.interpolate_uvzs_in_hull(rows, hw, return_info=True)
    b, ib = sparse.interpolate_uvzs_in_hull(rows, hw, keep_last_per_pixel=True, return_info=True)
    assert not np.array_equal(ia["abc"], ib["abc"])
    assert (a != 0).sum() > (b != 0).sum()  # the row outside the image is a vertex only without the flag
    part = rows[hull_ref.valid_rows(rows, hw, True)]
    assert np.array_equal(b != 0, sparse.interpolate_uvzs_in_hull(part, hw) != 0)  # the rows that stay, given alone: the same hull


@pytest.mark.parametrize("name", list(hc.DEGENERATE_FRAMES))
def test_degenerate_planes(name):
    rows, hw = hc.DEGENERATE_FRAMES[name]
    got, mask, info = _check_mask_and_hull(rows, hw)
    assert int(info["status"]) == sparse.STATUS_DEGENERATE and mask.sum() >= 1
    inside = mask != 0
    # the (n, 3) form: the host's minimum-norm plane, as interpolate_uvzs gives it
    assert _same(got[inside], sr.plane(rows, hw)[inside]), name
    # a batch: the status bit and NaN inside the hull
    b, ib = sparse.interpolate_uvzs_in_hull(rows[None], hw, return_info=True)
    assert b.shape == (1,) + tuple(hw) and int(ib["status"][0]) == sparse.STATUS_DEGENERATE and np.isnan(ib["abc"]).all()
    assert np.isnan(b[0][inside]).all() and _same(b[0][~inside], np.zeros(int((~inside).sum()), np.float32))


def test_collinear_masks_are_the_pixel_centres_on_the_segment():
    m = hull_ref.mask(hc.DEGENERATE_FRAMES["slope_2_7"][0], hc.HW)
    assert sorted(zip(*np.nonzero(m)[::-1])) == [(3 + 7 * k, 4 + 2 * k) for k in range(7)]
    assert _same(sparse.convex_hull_mask(hc.DEGENERATE_FRAMES["slope_2_7"][0][:, :2].copy(), hc.HW), m)
    one = sparse.convex_hull_mask(np.array([[20.4, 17.6]]), hc.HW)
    assert one.sum() == 1 and one[18, 20] == 1


def test_all_rows_invalid_and_no_rows():
    for rows in (hc.INVALID, np.zeros((0, 3))):
        got, info = sparse.interpolate_uvzs_in_hull(rows, hc.HW, return_info=True)
        assert _same(got, np.zeros(hc.HW, np.float32)) and int(info["hull_counts"]) == 0
        assert int(info["status"]) & sparse.STATUS_NO_SAMPLE
        assert np.isposinf(sparse.interpolate_uvzs_in_hull(rows, hc.HW, reciprocal=True)).all()
    assert int(sparse.interpolate_uvzs_in_hull(hc.INVALID, hc.HW, return_info=True)[1]["status"]) & sparse.STATUS_OUT_OF_RANGE
    assert sparse.convex_hull_mask(hc.INVALID[:, :2].copy(), hc.HW).sum() == 3  # without z, (5, 6) and (7, 8) are samples


def test_ragged_batch_frame_by_frame_and_reversed():
    rows, counts, hw, frames = hc.ragged()
    got, info = sparse.interpolate_uvzs_in_hull(rows, hw, counts=counts, return_info=True)
    assert got.shape == (len(counts),) + tuple(hw)
    alone = [sparse.interpolate_uvzs_in_hull(f[None], hw, return_info=True) for f in frames]
    for i, (a, ia) in enumerate(alone):
        assert _same(got[i], a[0]), i
        assert _same(info["abc"][i], ia["abc"][0]) and info["status"][i] == ia["status"][0] and info["hull_counts"][i] == ia["hull_counts"][0]
        assert _same((got[i] != 0) | np.isnan(got[i]), hull_ref.mask(frames[i], hw) != 0), i
    assert list(info["status"]) == [1, 2, 2, 0, 0]
    back = sparse.interpolate_uvzs_in_hull(_cuda(np.concatenate(frames[::-1])), hw, counts=counts[::-1])
    assert _same(back.cpu().numpy()[::-1], got)
    masks = sparse.convex_hull_mask(np.ascontiguousarray(rows[:, :2]), hw, counts=counts)
    for i, f in enumerate(frames):
        assert _same(masks[i], hull_ref.mask(f, hw)), i
    # a dense batch and zero_frames
    two = np.stack([frames[4], frames[4][::-1]])
    z = sparse.interpolate_uvzs_in_hull(two, hw, reciprocal=True, zero_frames=np.array([False, True]))
    assert _same(z[0], sparse.interpolate_uvzs_in_hull(frames[4], hw, reciprocal=True)) and _same(z[1], np.zeros(hw, np.float32))
