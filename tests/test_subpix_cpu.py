"""Without a GPU: the NumPy restatement of cornerSubPix (tests/subpix_ref.py) on rendered boards with analytic corners
(tests/subpix_cases.py), its two summation orders against each other (tests/golden/subpix_order.json), the host side of
``imgproc.corner_sub_pix`` (mask, zero zone, criteria, refusals), the order of the entry points' checks, and
``calibrating_amd.boards`` against what the reference's own boards.py returned (tests/golden/reference_boards.npz)."""
import ast
import ctypes
import os

import numpy as np
import pytest

import subpix_cases as sc
import subpix_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WINDOWS = [(4, 4), (1, 1), (5, 3), (11, 11)]


@pytest.mark.parametrize("i", range(len(sc.POSES)))
def test_refinement_brings_every_seed_closer_to_the_analytic_corner(i):
    f = sc.frame(i)
    assert f["truth"].min() > 16 and (f["truth"].max(0) < (sc.W - 16, sc.H - 16)).all()  # windows up to 11 stay inside
    start = np.linalg.norm(f["seeds"] - f["truth"], axis=1)
    assert start.max() > 2.8 and start.min() > 0.05
    for order in ("cv2", "wave"):
        out, its, sts = ref.corner_sub_pix(f["img"], f["seeds"], order=order)
        end = np.linalg.norm(out - f["truth"], axis=1)
        print(order, "iterations", its.min(), its.max(), "start %.3f end %.4f" % (start.max(), end.max()))
        assert out.dtype == np.float32 and (sts == 0).all() and (its < 30).all()
        assert (end < start).all()


def test_the_two_orders_agree_and_the_file_holds_the_measurement():
    import json
    with open(sc.ORDER_PATH) as fh:
        rec = json.load(fh)
    now = sc.measure_order()
    assert now["same_iterations"] and rec["same_iterations"]
    assert now["corners"] == rec["corners"] == len(sc.POSES) * len(sc.ORDER_WINDOWS) * 12
    assert now["corner_disagreement"] == rec["corner_disagreement"]
    # U31's other switch, cv2's running product against the kernel's four taps: the last float32 bit of a sample, which
    # reaches a corner as a few float32 ulp of a coordinate below 128 (one ulp there is 7.6e-6 px) or not at all
    assert now["bilinear_same_iterations"] and rec["bilinear_same_iterations"]
    assert now["bilinear_disagreement"] == rec["bilinear_disagreement"] <= 4 * 2.0 ** -17


def test_the_bilinear_switch_is_the_last_bit_only():
    f = sc.frame(0)
    a = ref.rect_sub_pix(f["img"], 50.3, 40.7, 11, 11, "four_tap")
    b = ref.rect_sub_pix(f["img"], 50.3, 40.7, 11, 11, "running")
    assert a.dtype == b.dtype == np.float32 and np.abs(a - b).max() <= 255 * 2.0 ** -22
    assert np.array_equal(ref.rect_sub_pix(f["img"], 50.0, 40.0, 5, 3), f["img"][39:42, 48:53].astype(np.float32))
    # replicate border
    assert np.array_equal(ref.rect_sub_pix(f["img"], 0.0, 0.0, 5, 5), f["img"][np.ix_([0, 0, 0, 1, 2], [0, 0, 0, 1, 2])].astype(np.float32))


def test_gray_restatement():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    for bits in (15, 14):
        assert sum(ref.GRAY_WEIGHTS[bits]) == 1 << bits
        g = ref.gray(img, "bgr", bits)
        assert g.dtype == np.uint8 and np.array_equal(g, ref.gray(img[..., ::-1], "rgb", bits))
        assert not np.array_equal(g, ref.gray(img, "rgb", bits))
        assert np.abs(g.astype(int) - np.rint(img @ np.array([0.114, 0.587, 0.299]))).max() <= 1
        flat = np.full((2, 2, 3), 200, np.uint8)
        assert (ref.gray(flat, "bgr", bits) == 200).all()


# ---- the host side of imgproc.corner_sub_pix ----
@pytest.mark.parametrize("win", WINDOWS)
def test_mask_values(win):
    from calibrating_amd import imgproc
    m = imgproc.sub_pix_mask(win)
    ww, wh = win
    assert m.dtype == np.float32 and m.shape == (2 * wh + 1, 2 * ww + 1) and m.flags.c_contiguous
    assert np.array_equal(m, ref.mask(win))
    e1 = np.float32(np.exp(-1.0))
    assert m[wh, ww] == 1 and m[0, 0] == np.float32(e1 * e1) and m[wh, 0] == e1 and m[0, ww] == e1
    assert np.array_equal(m, m[::-1]) and np.array_equal(m, m[:, ::-1])
    # the float32 steps: y = (float)(i - win) / win, squared in float32
    y = np.float32(1 - wh) / np.float32(wh)
    assert m[1, ww] == np.float32(np.exp(np.float64(-(y * y))))


def test_zero_zone():
    from calibrating_amd import imgproc
    full = imgproc.sub_pix_mask((4, 4))
    for zone in [(-1, -1), (0, 0), (1, 1), (3, 3), (2, 1)]:
        m = imgproc.sub_pix_mask((4, 4), zone)
        assert np.array_equal(m, ref.mask((4, 4), zone))
        zx, zy = zone
        hole = np.zeros_like(m, bool)
        if zx >= 0:
            hole[4 - zy:4 + zy + 1, 4 - zx:4 + zx + 1] = True
        assert (m[hole] == 0).all() and np.array_equal(m[~hole], full[~hole]) and hole.sum() == (0 if zx < 0 else (2 * zx + 1) * (2 * zy + 1))
    # not applied: a zone as large as the window, or given on one axis only
    for zone in [(4, 4), (4, 0), (0, 9), (-1, 1), (1, -1)]:
        assert np.array_equal(imgproc.sub_pix_mask((4, 4), zone), full) and np.array_equal(ref.mask((4, 4), zone), full)
    assert np.array_equal(imgproc.sub_pix_mask((5, 3), (4, 2)), ref.mask((5, 3), (4, 2)))
    with pytest.raises(ValueError):
        imgproc.sub_pix_mask((0, 4))


def test_criteria_parsing():
    from calibrating_amd import imgproc
    COUNT, EPS = imgproc.TERM_CRITERIA_COUNT, imgproc.TERM_CRITERIA_EPS
    cases = [((30, 0.01), (30, 0.01 * 0.01)), ((COUNT + EPS, 30, 0.01), (30, 0.01 * 0.01)), ((COUNT, 7, 0.5), (7, 0.0)),
             ((EPS, 7, 0.5), (100, 0.25)), ((None, 0.1), (100, 0.1 * 0.1)), ((12, None), (12, 0.0)), ((0, 0.01), (1, 0.01 * 0.01)),
             ((-5, -1.0), (1, 0.0)), ((1000, 0.0), (100, 0.0)), ((COUNT + EPS, 1000, -3.0), (100, 0.0))]
    for given, want in cases:
        assert imgproc.sub_pix_criteria(given) == want, given
        assert ref.criteria(given) == want, given
    for bad in [(30,), (0, 30, 0.01), (4, 30, 0.01), (1, 2, 3, 4)]:
        with pytest.raises(ValueError):
            imgproc.sub_pix_criteria(bad)


def test_corner_sub_pix_refuses_before_the_device():
    from calibrating_amd import imgproc
    img, c = np.zeros((20, 30), np.uint8), np.zeros((5, 2), np.float32)
    for images, corners, kw in [(img.astype(np.float32), c, {}), (img, c.astype(np.int32), {}), (img, np.zeros((5, 3), np.float32), {}),
                                (np.stack([img, img]), c, {}), (np.stack([img, img]), np.zeros((3, 5, 2), np.float32), {}),
                                (img, c, dict(counts=[2, 3])), (np.stack([img, img]), c, dict(counts=[2, 2])),
                                (img, c, dict(win=(0, 4))), (img, c, dict(criteria=(1, 2, 3, 4))), (img[None, None, None], c, {})]:
        with pytest.raises(ValueError):
            imgproc.corner_sub_pix(images, corners, **kw)
    import torch
    with pytest.raises(ValueError, match="GPU"):
        imgproc.corner_sub_pix(torch.zeros((20, 30), dtype=torch.uint8), torch.zeros((5, 2)))
    with pytest.raises(TypeError):
        imgproc.corner_sub_pix([[0]], c)
    # an input that breaks two rules: the images' dtype is refused before the corners are looked at, their rank after
    for images, corners in [(img.astype(np.float32), c.tolist()), (img.astype(np.float32), torch.zeros((5, 2))), (img.astype(np.int8), c.astype(np.int32))]:
        with pytest.raises(ValueError, match="uint8"):
            imgproc.corner_sub_pix(images, corners)
    with pytest.raises(TypeError):
        imgproc.corner_sub_pix(img[None, None, None], c.tolist())
    with pytest.raises(ValueError):
        imgproc.cvt_gray(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        imgproc.cvt_gray(np.zeros((4, 4, 3), np.uint8), code="gray")


def test_the_new_entry_points_check_before_they_probe():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the formed calls must not reach a kernel")
    from calibrating_amd import _native
    lib = _native.lib()
    A = lambda k: 0x7000000000 + (k << 20)  # made-up device addresses, never read
    dbl = ctypes.c_double

    def sub(w=64, h=48, frames=1, rows=8, start=None, win=(4, 4), iters=30, eps=1e-4, type_=_native.VALUE_F32, gray=A(0)):
        return lib.camd_corner_sub_pix(gray, w, h, w, w * h, frames, A(1), type_, rows, start, win[0], win[1], A(2), iters,
                                       dbl(eps), A(3), A(4), A(5), None)
    assert sub() == _native.CAMD_ERR_NO_DEVICE
    assert sub(start=A(6), frames=3) == _native.CAMD_ERR_NO_DEVICE and sub(win=(11, 11)) == _native.CAMD_ERR_NO_DEVICE
    assert sub(win=(30, 30), w=80, h=80) == _native.CAMD_ERR_NO_DEVICE
    for kw in [dict(win=(0, 4)), dict(win=(4, -1)), dict(w=12), dict(h=12), dict(win=(11, 11), w=26, h=48)]:
        assert sub(**kw) == _native.CAMD_ERR_BAD_ARG, kw
    assert "window" in _native.last_error()
    assert sub(w=13, h=13) == _native.CAMD_ERR_NO_DEVICE  # 2 * 4 + 5: cv2's smallest
    for kw in [dict(iters=0), dict(iters=101), dict(eps=-1.0), dict(eps=float("nan")), dict(type_=_native.VALUE_U8),
               dict(frames=3, rows=8), dict(frames=0), dict(gray=None), dict(start=A(6) + 4)]:
        assert sub(**kw) == _native.CAMD_ERR_BAD_ARG, kw
    assert sub(win=(31, 31), w=100, h=100) == _native.CAMD_ERR_UNSUPPORTED and "patch" in _native.last_error()
    assert sub(rows=0) == _native.CAMD_OK  # nothing to launch: no probe

    def gray(w=8, h=6, pitch=24, dpitch=8, batch=1, k=(3735, 19235, 9798), shift=15, src=A(0)):
        return lib.camd_bgr_to_gray_u8(src, w, h, pitch, pitch * h, A(1), dpitch, dpitch * h, batch, k[0], k[1], k[2], shift, None)
    assert gray() == _native.CAMD_ERR_NO_DEVICE and gray(k=(1868, 9617, 4899), shift=14) == _native.CAMD_ERR_NO_DEVICE
    for kw in [dict(w=0), dict(pitch=23), dict(dpitch=7), dict(batch=0), dict(shift=14), dict(k=(-1, 19235, 13534)), dict(src=None),
               dict(shift=0, k=(0, 0, 1))]:
        assert gray(**kw) == _native.CAMD_ERR_BAD_ARG, kw


# ---- boards ----
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "reference_boards.npz"))


def test_chessboard_object_points_equal_the_references(fx):
    import calibrating_amd as ca
    n = 0
    while "board%d/args" % n in fx:
        cw, ch, size_mm = fx["board%d/args" % n]
        size_mm = int(size_mm) if size_mm == int(size_mm) else float(size_mm)
        b = ca.Chessboard(checkboard=(int(cw), int(ch)), size_mm=size_mm)
        want = fx["board%d/object_points" % n]
        assert b.object_points.dtype == want.dtype == np.float32 and np.array_equal(b.object_points, want)
        assert np.abs(b.object_points.mean(0)).max() < 1e-7
        n += 1
    assert n >= 4
    d = ca.Chessboard()
    assert d.checkboard == (11, 8) and d.size_mm == 25 and d.object_points.shape == (88, 3) and str(d) == str(d.init_kwargs)
    assert issubclass(ca.Chessboard, ca.BaseBoard)
    with pytest.raises(NotImplementedError):
        ca.BaseBoard().find_image_points({})
    pts = {0: np.ones((4, 3)), 1: np.full((2, 3), 4.0)}
    centred = ca.BaseBoard.set_origin_to_center(pts)
    assert np.allclose(centred[0], -1) and np.allclose(centred[1], 2)


def test_build_with_calibration_img_equals_the_references(fx):
    import calibrating_amd as ca
    n = 0
    while "image%d/args" % n in fx:
        h, w, k, ppi = fx["image%d/args" % n]
        ppi = int(ppi) if ppi == int(ppi) else float(ppi)
        b = ca.Chessboard.build_with_calibration_img(hw=(int(h), int(w)), n=int(k), ppi=ppi)
        assert tuple(b.checkboard) == tuple(fx["image%d/checkboard" % n]) and b.calibration_img_name == str(fx["image%d/name" % n])
        assert np.array_equal(b.object_points, fx["image%d/object_points" % n])
        assert b.calibration_img.dtype == np.uint8 and b.calibration_img.shape == (int(h), int(w))
        assert set(np.unique(b.calibration_img)) <= {0, 255}
        assert np.array_equal(np.packbits(b.calibration_img == 255), fx["image%d/img_bits" % n])
        assert sorted(b.calibration_img_info.items()) == ast.literal_eval(str(fx["image%d/info" % n]))
        n += 1
    assert n >= 4


def test_without_a_coarse_guess_the_quad_search_is_refused():
    import calibrating_amd as ca
    board = ca.Chessboard((4, 3))
    img = sc.frame(0)["img"]
    d = dict(img=img)
    with pytest.raises(NotImplementedError) as e:
        board.find_image_points(d)
    msg = str(e.value)
    assert "findChessboardCorners" in msg and "not provided" in msg and "coarse_corners" in msg and "project_points" in msg
    assert set(d) == {"img"}
    # through a region of interest too, and the record keeps its image
    roi = ca.Chessboard.get_roi_class((8, 90, 10, 120))((4, 3))
    with pytest.raises(NotImplementedError):
        roi.find_image_points(d)
    assert d["img"] is img
    # a guess of the wrong size is refused before the device
    for bad in (np.zeros((11, 2), np.float32), np.zeros((12, 3), np.float32), np.zeros((12, 2, 2), np.float32)):
        with pytest.raises(ValueError):
            board.find_image_points(dict(img=img, coarse_corners=bad))
    with pytest.raises(ValueError):
        board.find_image_points_batch(np.stack([img, img]), np.zeros((3, 12, 2), np.float32))
    with pytest.raises(ValueError, match=r"got \(3, 2\)"):  # a list, not an array
        board.find_image_points(dict(img=img, coarse_corners=[[1.0, 2.0]] * 3))


def test_what_cv2_returned_when_the_export_tool_has_run():
    """tools/export_cv2_golden.py writes tests/golden/cv2_subpix.npz on a machine that has cv2: inputs and what cv2's
    cvtColor and cornerSubPix returned.  Where the file is committed, the restatement with its default switches (the
    kernel's arithmetic) must equal it, which pins U31 and U32; a file that differs fails.  Without the file nothing is
    pinned and the test is skipped."""
    path = os.path.join(GOLDEN, "cv2_subpix.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/cv2_subpix.npz is absent: cv2's cornerSubPix and cvtColor stay unpinned (U31, U32)")
    fx = np.load(path)
    crit = (3, 30, 0.01)
    i = 0
    while "frame%d/rgb" % i in fx:
        rgb, seeds = fx["frame%d/rgb" % i], fx["frame%d/seeds" % i]
        assert np.array_equal(ref.gray(rgb, "bgr"), fx["frame%d/gray" % i]), "U32, frame %d" % i
        img = sc.frame(i)["img"]
        for key in [k for k in fx.files if k.startswith("frame%d/win" % i)]:
            win, zone = key.split("/")[1].split("_")
            win = tuple(int(v) for v in win[3:].split("x"))
            zone = (int(zone[4:]),) * 2
            got = ref.corner_sub_pix(img, seeds, win, zone, crit)[0]
            assert np.array_equal(got, fx[key][:, 0]), "U31, %s" % key
        i += 1
    assert i == len(sc.POSES)
