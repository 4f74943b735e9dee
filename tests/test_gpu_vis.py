"""The pictures on the GPU (-m gpu), bit-equal throughout: against what the REFERENCE's own vis_depth_l1 / vis_depth /
vis_stereo / vis_align returned (tests/golden/reference_vis.npz) and, where the fixture cannot go (the limit itself,
batches, a caller's table, the three cases calibrating_amd defines), against their NumPy restatement tests/vis_ref.py
(which tests/test_vis_cpu.py pins to that fixture)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
import vis_cases as cases  # noqa: E402
import vis_ref  # noqa: E402


def _cuda(a):
    return torch.from_numpy(a).cuda() if isinstance(a, np.ndarray) else a


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %d bytes differ" % (what, (got != want).sum())


@pytest.fixture(scope="module")
def golden():
    fx = cases.load_fixture()
    assert fx is not None
    return fx


def test_l1_golden_cases(golden):
    for name, (re, gt, kw) in cases.l1_cases().items():
        _same(ca.vis_depth_l1(re, gt, **kw), golden["l1/" + name], name)
        got = ca.vis_depth_l1(_cuda(re), _cuda(gt), **kw)
        assert got.is_cuda
        _same(got.cpu().numpy(), golden["l1/" + name], name + " (tensors)")
    re, gt, kw = cases.l1_cases()["p72x131_f32"]  # float32 is widened: the picture of the float64 copy
    _same(ca.vis_depth_l1(re.astype(np.float64), gt.astype(np.float64), **kw), golden["l1/p72x131_f32"], "widened")


def test_selection_through_resolve_max_l1():
    for name, (re, gt) in cases.selection_inputs().items():
        for m in cases.MAX_L1S:
            for over in (True, False):
                got = ca.resolve_max_l1(re, gt, max_l1=m, overexposed=over)
                want = vis_ref.resolve_max_l1(re, gt, max_l1=m, overexposed=over)
                assert got.dtype == np.float64 and got.shape == () and got.tobytes() == want.tobytes(), (name, m, over, got, want)
    assert ca.resolve_max_l1(*cases.selection_inputs()["no_valid"], max_l1=-0.2) == 1.0
    # the bar's pixels take part when the limit is asked for with one
    re, gt = cases.depth_pair((72, 131), 2)
    for bar in cases.BARS:
        assert ca.resolve_max_l1(re, gt, max_l1=-0.2, colorbar=bar) == vis_ref.resolve_max_l1(re, gt, max_l1=-0.2, colorbar=bar)
    # larger pictures: several workgroups per histogram
    re, gt = cases.depth_pair((131, 257), 3)
    for m in (None, -0.2, -0.999, -1, 0):
        assert ca.resolve_max_l1(re, gt, max_l1=m) == vis_ref.resolve_max_l1(re, gt, max_l1=m), m


def test_l1_batch_has_a_limit_per_image():
    pairs = [cases.depth_pair((72, 131), 10 + s, holes=h) for s, h in ((0, 0.02), (1, 0.3), (2, 0.7))]
    re, gt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    valid = [int(((r != 0) & (g != 0)).sum()) for r, g in pairs]
    assert len(set(valid)) == 3
    limits = ca.resolve_max_l1(re, gt)
    assert limits.shape == (3,) and len(set(limits.tolist())) == 3
    for kw in (dict(), dict(max_l1=-0.2, colorbar="u"), dict(max_l1=0.03, overexposed=False)):
        got = ca.vis_depth_l1(re, gt, **kw)
        assert got.shape == (3, 72, 131, 3)
        for i in range(3):
            _same(got[i], vis_ref.vis_depth_l1(re[i], gt[i], **kw), (kw, i))
    for i in range(3):
        assert limits[i] == vis_ref.resolve_max_l1(re[i], gt[i])
    t = ca.vis_depth_l1(_cuda(re), 1.6)
    _same(t.cpu().numpy(), np.stack([vis_ref.vis_depth_l1(re[i], 1.6) for i in range(3)]), "gt as a number")


def test_l1_defined_cases():
    for hw, seed in (((1, 1), 0), ((37, 53), 1), ((72, 131), 2), ((131, 257), 3)):
        re, gt = cases.depth_pair(hw, seed)
        for bar in cases.BARS + (None,):  # max_l1=None with a bar: the reference raises; the limit first, then the bar
            for over in (True, False):
                _same(ca.vis_depth_l1(re, gt, overexposed=over, colorbar=bar),
                      vis_ref.vis_depth_l1(re, gt, overexposed=over, colorbar=bar), (hw, bar, over))
    assert ca.vis_depth_l1.__defaults__ == (0, None, True, "auto")
    re, gt = cases.depth_pair((72, 131), 2)
    same = np.where(gt != 0, gt, 1.0)  # a limit of 0: the grey 25 on every valid pixel
    for m in (0, -0.5, None):
        got = ca.vis_depth_l1(same, same, max_l1=m, colorbar=None)
        assert (got == 25).all(), m
        _same(got, vis_ref.vis_depth_l1(same, same, max_l1=m, colorbar=None), m)
    for bad in (np.nan, np.inf, -np.inf):
        broken = re.copy()
        broken[40, 100] = bad
        with pytest.raises(ValueError, match="NaN or infinite"):
            ca.vis_depth_l1(broken, gt)
        with pytest.raises(ValueError, match="NaN or infinite"):
            ca.vis_depth_l1(_cuda(re), _cuda(np.where(gt == 0, bad, gt)), max_l1=0.03)
        with pytest.raises(ValueError, match="NaN or infinite"):
            ca.resolve_max_l1(re.astype(np.float32), broken.astype(np.float32))


def test_l1_repeats_are_identical():
    re, gt = (_cuda(a) for a in cases.depth_pair((131, 257), 3))
    first = ca.vis_depth_l1(re, gt).cpu().numpy()
    second = ca.vis_depth_l1(re, gt).cpu().numpy()
    assert first.tobytes() == second.tobytes()


def test_vis_depth(golden):
    for name, (d, kw) in cases.depth_cases().items():
        _same(ca.vis_depth(d, **kw), golden["depth/" + name], name)
        _same(ca.vis_depth(_cuda(d), **kw).cpu().numpy(), golden["depth/" + name], name + " (tensors)")
    table = np.random.default_rng(5).integers(0, 256, (256, 3), dtype=np.uint8)  # a caller's table: the lookup is exact
    for dtype in (np.float64, np.float32, np.uint16):
        d = cases.depth_image((131, 257), 4, dtype)
        for kw in (dict(fix_range=5), dict(fix_range=(0.5, 4.25)), dict(), dict(slicen=10), dict(fix_range=3.0, slicen=30)):
            got = ca.vis_depth(d, colormap=table, **kw)
            _same(got, vis_ref.vis_depth(d, table=table, **kw), (dtype.__name__, kw))
            assert (got[d == 0] == 0).all() and (d == 0).sum() > 100
        _same(ca.vis_depth(_cuda(d), colormap=_cuda(table)).cpu().numpy(), vis_ref.vis_depth(d, table=table), "table tensor")
    batch = np.stack([cases.depth_image((37, 53), s) for s in range(3)])
    got = ca.vis_depth(batch, slicen=10)
    for i in range(3):  # norma: every image has its own range
        _same(got[i], vis_ref.vis_depth(batch[i], slicen=10), i)
    for const in (np.full((37, 53), 1.5), np.full((5, 7), 2, np.uint16)):  # a constant image: index 0
        _same(ca.vis_depth(const, colormap=table), np.broadcast_to(table[0], const.shape + (3,)).copy(), "constant")
    rgb = torch.zeros((4, 5, 3), dtype=torch.uint8, device="cuda")
    assert ca.vis_depth(rgb) is rgb


def test_vis_stereo_and_align(golden):
    for name, (a, b, n_line) in cases.line_cases().items():
        _same(ca.vis_stereo(a, b, n_line=n_line), golden["stereo/" + name], name)
        tiles = ca.vis_align(a, b, n_line=n_line)
        dev = ca.vis_align(_cuda(a), _cuda(b), n_line=n_line)
        assert len(tiles) == 4 and len(dev) == 4
        for t in range(4):
            _same(tiles[t], golden["align/%s/%d" % (name, t)], (name, t))
            _same(dev[t].cpu().numpy(), golden["align/%s/%d" % (name, t)], (name, t, "tensors"))
    a, b = cases.picture((40, 60), 7, 3), cases.picture((40, 60), 8, 3)
    _same(ca.vis_stereo(a, b, n_line=7, thickness=0.4), vis_ref.vis_stereo(a, b, 7, 0.4), "thickness")
    batch1, batch2 = np.stack([a, b]), np.stack([b[..., 0], a[..., 0]])
    got = ca.vis_align(batch1, batch2, n_line=5)
    for i in range(2):
        for t, tile in enumerate(vis_ref.vis_align(batch1[i], batch2[i], 5)):
            _same(got[t][i], tile, (i, t))


def _cams():
    K = np.array([[90.0, 0, 48.5], [0, 92.0, 31.0], [0, 0, 1]])
    cam1 = ca.Cam(K, [0.08, -0.02, 0.001, -0.002, 0.01], (96, 64))
    cam2 = ca.Cam(K * np.array([[1.1], [1.1], [1]]), None, (96, 64))
    T = np.eye(4)
    T[:3, 3] = (0.05, -0.01, 0.02)
    return cam1, cam2, T


def test_cam_alignment_pictures():
    from calibrating_amd import vis
    cam1, cam2, T = _cams()
    img1, img2 = cases.picture((64, 96), 1, 3), cases.picture((64, 96), 2, 3)
    for depth in (cases.depth_image((64, 96), 5), cases.depth_image((64, 96), 5, np.uint16)):
        top = 5000 if depth.dtype == np.uint16 else 5
        clipped = depth.clip(0, top)
        pic = vis._jet_bgr_075()[np.uint8(clipped / clipped.max() * 255)]  # camera.py:317-319
        want = ca.vis_align(cam1.undistort_img(img1), pic)
        got = cam1.vis_depth_alignment(img1, depth)
        dev = cam1.vis_depth_alignment(_cuda(img1), _cuda(depth))
        for t in range(4):
            _same(got[t], want[t], ("depth alignment", t))
            _same(dev[t].cpu().numpy(), want[t], ("depth alignment, tensors", t))
    depth2 = cases.depth_image((64, 96), 6)
    want = ca.vis_align(cam1.undistort_img(img1), cam1.reproject_img(cam2, depth2, img2, T))
    got = cam1.vis_reproject_img_alignment(cam2, depth2, img2, img1, T=T)
    for t in range(4):
        _same(got[t], want[t], ("reproject alignment", t))
    with pytest.raises(NotImplementedError):
        cam1.vis_reproject_img_alignment(cam2, depth2, img2, img1)
    with pytest.raises(ValueError, match="distort"):
        cam2.vis_reproject_img_alignment(cam1, depth2, img2, img1, T=T)
