"""CPU tests of the picture fixtures and front end (no GPU): tests/vis_ref.py, the NumPy restatement the GPU tests
compare against, equals what the REFERENCE's own vis_depth_l1 / vis_depth / vis_stereo / vis_align returned
(tests/golden/reference_vis.npz) bit for bit; the cases do what they are there for; the wrappers refuse bad arguments
before they touch a device."""
import numpy as np
import pytest

import vis_cases as cases
import vis_ref


@pytest.fixture(scope="module")
def golden():
    fx = cases.load_fixture()
    assert fx is not None, "tests/golden/reference_vis.npz is missing (tests/golden/make_vis_golden.py makes it)"
    return fx


def test_restatement_equals_the_reference_l1(golden):
    for name, (re, gt, kw) in cases.l1_cases().items():
        got = vis_ref.vis_depth_l1(re, gt, **kw)
        assert got.dtype == np.uint8 and np.array_equal(got, golden["l1/" + name]), name
    # a bar 0 wide: every placement gives one picture; a bar 2 wide: they differ
    assert all(np.array_equal(golden["l1/p37x53_fixed_u"], golden["l1/p37x53_fixed_" + b]) for b in cases.BARS)
    assert len({golden["l1/p72x131_top20_" + b].tobytes() for b in "udlr"}) == 4
    assert np.array_equal(golden["l1/p72x131_top20_auto"], golden["l1/p72x131_top20_l"])  # the shorter side: left
    # over-exposure is there to be seen, on both sides
    pic = golden["l1/p131x257_none_nobar"]
    assert ((pic == (255, 255, 0)).all(-1)).sum() > 100 and ((pic == (230, 255, 230)).all(-1)).sum() > 100


def test_restatement_equals_the_reference_depth(golden):
    for name, (d, kw) in cases.depth_cases().items():
        kw = dict(kw)
        cm = kw.pop("colormap", None)
        table = None if cm is None else vis_ref._vis.colormap_table(cm)
        assert np.array_equal(vis_ref.vis_depth(d, table=table, **kw), golden["depth/" + name]), name
    d = cases.depth_image((37, 53), 1)
    assert (golden["depth/d37x53_f64_range5"][d == 0] == 0).all() and (d == 0).sum() > 20


def test_restatement_equals_the_reference_lines(golden):
    for name, (a, b, n_line) in cases.line_cases().items():
        assert np.array_equal(vis_ref.vis_stereo(a, b, n_line), golden["stereo/" + name]), name
        for t, tile in enumerate(vis_ref.vis_align(a, b, n_line)):
            assert np.array_equal(tile, golden["align/%s/%d" % (name, t)]), (name, t)


def test_line_table_is_the_reference_loop():
    from calibrating_amd import vis
    for size, n_line in ((40, 21), (61, 5), (10, 30), (7, 64), (120, 1), (1, 3)):
        want = np.full(size, -1, np.int8)
        for rows, c in vis_ref._line_rows(size, n_line):
            want[list(rows)] = c
        assert np.array_equal(vis.line_table(size, n_line), want), (size, n_line)


def test_selection_inputs_stress_the_select():
    s = cases.selection_inputs()
    l1, mask, _ = vis_ref.l1_planes(*s["quantised"], max_l1=-0.2, colorbar=None)
    a = np.abs(l1[mask])
    assert len(np.unique(a)) < 0.5 * a.size  # ties
    l1, mask, limit = vis_ref.l1_planes(*s["lowest_byte"], max_l1=-0.2, colorbar=None)
    keys = np.abs(l1[mask]).view(np.uint64)
    assert len(np.unique(keys >> 8)) == 1 and len(np.unique(keys)) > 100  # only the last digit tells them apart
    l1, mask, _ = vis_ref.l1_planes(*s["binades"], max_l1=-0.2, colorbar=None)
    a = np.abs(l1[mask])
    assert (a == 0).sum() > 50 and ((a > 0) & (a < 2.3e-308)).sum() > 50 and a.max() / a[a > 1e-300].min() > 2.0 ** 38
    assert vis_ref.resolve_max_l1(*s["no_valid"], max_l1=-0.2) == 1.0
    l1, mask, limit = vis_ref.l1_planes(*s["k_zero"], max_l1=-0.2, colorbar=None)
    assert mask.sum() == 4 and limit == np.abs(l1).max()
    # each stated limit equals np.partition's, the reference's own way to it
    for name, (re, gt) in s.items():
        for m in (-0.05, -0.2, -0.999):
            l1, mask, limit = vis_ref.l1_planes(re, gt, max_l1=m, colorbar=None)
            if mask.any():
                k = int(-m * mask.sum())
                assert limit == (-np.partition(-np.abs(l1)[mask], k)[:k + 1]).min(), (name, m)


def test_defined_cases_of_the_restatement():
    re, gt = cases.depth_pair((72, 131), 2)
    # max_l1=None with a bar: the limit of the picture without the bar, then the bar from it
    limit = vis_ref.resolve_max_l1(re, gt, colorbar="auto")
    assert limit == vis_ref.resolve_max_l1(re, gt, colorbar=None)
    pic = vis_ref.vis_depth_l1(re, gt)
    assert np.array_equal(pic[:, 2:], vis_ref.vis_depth_l1(re, gt, max_l1=float(limit), colorbar=None)[:, 2:])
    assert tuple(pic[0, 0]) == (230, 255, 230) and tuple(pic[-1, 0]) == (255, 255, 0)  # the bar's over-exposed ends
    # a limit of 0: valid pixels are the grey 25
    same = np.where(gt != 0, gt, 1.0)
    assert (vis_ref.vis_depth_l1(same, same, max_l1=0, colorbar=None) == 25).all()
    with pytest.raises(ValueError):
        vis_ref.vis_depth_l1(np.where(re > 2, np.nan, re), gt)
    assert (vis_ref.vis_depth(np.full((5, 7), 1.5)) == vis_ref._vis.colormap_table(2)[0]).all()  # a constant image


def test_colour_tables():
    from calibrating_amd import vis
    for cm in (vis.COLORMAP_JET, vis.COLORMAP_HSV):
        t = vis.colormap_table(cm)
        assert t.shape == (256, 3) and t.dtype == np.uint8 and len(np.unique(t, axis=0)) > 200
    with pytest.raises(ValueError):
        vis.colormap_table(5)


def test_argument_validation_without_gpu():
    import calibrating_amd as ca
    from calibrating_amd import vis
    for name in ("vis_depth", "vis_depth_l1", "resolve_max_l1", "vis_stereo", "vis_align"):
        assert getattr(ca, name) is getattr(vis, name) and name in ca.__all__
    d = np.ones((8, 12))
    with pytest.raises(TypeError, match="float32 or float64"):
        ca.vis_depth_l1(d.astype(np.uint16))
    with pytest.raises(ValueError, match="shape"):
        ca.vis_depth_l1(d, np.ones((8, 13)))
    with pytest.raises(ValueError, match="colorbar"):
        ca.vis_depth_l1(d, 1.0, colorbar="x")
    with pytest.raises(ValueError, match="does not fit"):
        ca.vis_depth_l1(np.ones((1, 300)), 1.0, max_l1=1.0, colorbar="u")
    with pytest.raises(ValueError, match="finite"):
        ca.vis_depth_l1(d, np.inf)
    with pytest.raises(ValueError, match="finite"):
        ca.resolve_max_l1(d, 1.0, max_l1=np.nan)
    with pytest.raises(TypeError):
        ca.vis_depth(d.astype(np.int32))
    with pytest.raises(ValueError, match="fix_range"):
        ca.vis_depth(d, fix_range=(2.0, 1.0))
    with pytest.raises(ValueError, match="slicen"):
        ca.vis_depth(d, slicen=-1)
    rgba = np.zeros((8, 12, 4), np.uint8)
    assert ca.vis_depth(rgba) is rgba
    img = np.zeros((8, 12), np.uint8)
    with pytest.raises(ValueError, match="one size"):
        ca.vis_stereo(img, np.zeros((8, 13), np.uint8))
    with pytest.raises(ValueError, match="n_line"):
        ca.vis_align(img, img, n_line=-1)
    with pytest.raises(TypeError):
        ca.vis_stereo(img.tolist(), img)
    cam = ca.Cam(np.array([[100.0, 0, 6], [0, 100, 4], [0, 0, 1]]), None, (12, 8))
    bent = ca.Cam(cam.K, [0.1, 0, 0, 0, 0], (12, 8))
    with pytest.raises(ValueError, match="distort"):
        cam.vis_reproject_img_alignment(bent, d, img, img, T=np.eye(4))
    with pytest.raises(NotImplementedError):
        cam.vis_reproject_img_alignment(cam, d, img, img)


def test_c_entry_points_refuse_without_gpu():
    """The C ABI's own refusals come before the device check, with a message."""
    import ctypes
    from calibrating_amd import _native
    lib = _native.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    BAD = _native.CAMD_ERR_BAD_ARG

    def error(w=4, h=4, batch=1, place=0, width=0, vt=0):
        return lib.camd_vis_l1_error(p, None, 1.0, vt, w, h, batch, place, width, 1.0, p, p, p, p, None)

    assert error(w=0) == BAD and error(batch=70000) == BAD and error(vt=2) == BAD
    assert error(w=65536, h=65536) == BAD and "int32" in _native.last_error()
    assert error(place=1, width=5) == BAD and "does not fit" in _native.last_error()
    assert error(place=7, width=1) == BAD
    assert lib.camd_vis_l1_bar(p, p, 4, 4, 1, 3, 5, p, None) == BAD
    limit = lambda mode, value, npix=16: lib.camd_vis_l1_limit(p, p, npix, 1, mode, value, p, p, p, None)  # noqa: E731
    assert limit(0, 0.0) == BAD and limit(2, 1.0) == BAD and limit(2, 0.0) == BAD and limit(3, 0.5) == BAD
    assert limit(1, 0.0, npix=0) == BAD
    assert lib.camd_vis_l1_colour(p, p, 16, 1, None, 1, p, None) == BAD
    depth = lambda vt=0, div=1.0, lo=0.0, hi=1.0, mode=0, scale=255.9: lib.camd_vis_depth(  # noqa: E731
        p, vt, 16, 1, div, lo, hi, 0.0, 1.0, None, mode, 0.0, scale, p, 1, p, None)
    assert depth(vt=2) == BAD and depth(div=0.0) == BAD and depth(lo=2.0) == BAD and depth(mode=1) == BAD
    assert depth(scale=256.0) == BAD
    assert lib.camd_vis_depth_range(p, 2, 16, 1, 1.0, 0.0, 1.0, p, None) == BAD
    lines = lambda cn=1, tiles=2, pitch=12: lib.camd_vis_lines(p, cn, p, 3, 4, 4, 1, p, None, tiles, p, pitch, 12, 96, None)  # noqa: E731
    assert lines(cn=2) == BAD and lines(tiles=3) == BAD and lines(pitch=11) == BAD
    assert lib.camd_vis_l1_limit_workspace_bytes(3) == 3 * (8 * 256 * 4 + 32)
    import torch
    if not torch.cuda.is_available():
        NO = _native.CAMD_ERR_NO_DEVICE  # (valid arguments reach the device check)
        assert error() == NO and error(place=1, width=2) == NO and limit(2, 0.05) == NO and depth() == NO and lines() == NO
