"""Sub-pixel corners on the MI355X (-m gpu): ``imgproc.corner_sub_pix``, ``imgproc.cvt_gray`` and ``boards.Chessboard``
against the NumPy restatement tests/subpix_ref.py with the kernel's summation order (``order="wave"``): corners,
iterations and status bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import imgproc  # noqa: E402

import subpix_cases as sc  # noqa: E402
import subpix_ref as ref  # noqa: E402


def want(images, corners, frame_of=None, **kw):
    """the restatement on (n, 2) rows, reshaped like ``corners``"""
    c = np.asarray(corners)
    out, its, sts = ref.corner_sub_pix(images, c.reshape(-1, 2), frame_of=frame_of, order="wave", **kw)
    return out.reshape(c.shape), its.reshape(c.shape[:-1]), sts.reshape(c.shape[:-1])


def same(got, exp):
    assert len(got) == len(exp) == 3
    for g, e in zip(got, exp):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == e.dtype and g.shape == e.shape
        assert np.array_equal(g.view(np.uint8), e.view(np.uint8)), (g, e)


@pytest.fixture(scope="module")
def rendered():
    images, seeds, truth = sc.batch()
    exp = want(images, seeds, frame_of=np.repeat(np.arange(len(images)), seeds.shape[1]))
    for a in exp:
        a.setflags(write=False)
    return images, seeds, truth, exp


def test_one_frame_and_three_frames_batched(rendered):
    images, seeds, truth, exp = rendered
    got = imgproc.corner_sub_pix(images, seeds, return_info=True)
    same(got, exp)
    assert (got[2] == 0).all() and (np.linalg.norm(got[0] - truth, axis=-1) < np.linalg.norm(seeds - truth, axis=-1)).all()
    for f in range(len(images)):
        one = imgproc.corner_sub_pix(images[f], seeds[f], return_info=True)
        same(one, [a[f] for a in exp])
    # cv2's (n, 1, 2), and corners alone without the info
    c = imgproc.corner_sub_pix(images[0], seeds[0][:, None])
    assert c.shape == (12, 1, 2) and np.array_equal(c[:, 0], exp[0][0])
    assert np.array_equal(seeds, sc.batch()[1])  # (not refined in place)


@pytest.mark.parametrize("n", [1, 5])
def test_corner_counts_that_are_no_multiple_of_four(rendered, n):
    images, seeds, _, exp = rendered
    same(imgproc.corner_sub_pix(images, seeds[:, :n], return_info=True), [a[:, :n] for a in exp])


def test_ragged_counts_with_an_empty_frame_and_a_frame_alone_or_last(rendered):
    images, seeds, _, exp = rendered
    counts = [5, 0, 12]
    imgs = np.stack([images[0], images[1], images[2]])
    rows = np.concatenate([seeds[0, :5], seeds[2]])
    got = imgproc.corner_sub_pix(imgs, rows, counts=counts, return_info=True)
    same(got, [np.concatenate([a[0, :5], a[2]]) for a in exp])
    # the last frame's bits: alone, at the end of the dense batch, at the end of the ragged one
    alone = imgproc.corner_sub_pix(images[2], seeds[2], return_info=True)
    same([g[5:] for g in got], alone)
    same([g[2] for g in imgproc.corner_sub_pix(images, seeds, return_info=True)], alone)
    # every frame empty but one; an empty call
    got = imgproc.corner_sub_pix(imgs, seeds[1], counts=[0, 12, 0], return_info=True)
    same(got, [a[1] for a in exp])
    none = imgproc.corner_sub_pix(imgs, np.zeros((0, 2), np.float32), counts=[0, 0, 0], return_info=True)
    assert none[0].shape == (0, 2) and none[1].shape == (0,)


@pytest.mark.parametrize("win", [(4, 4), (1, 1), (5, 3), (11, 11)])
def test_windows(win):
    f = sc.frame(1)
    got = imgproc.corner_sub_pix(f["img"], f["seeds"], win=win, return_info=True)
    same(got, want(f["img"], f["seeds"], win=win))
    if win == (1, 1):
        assert (got[2] & imgproc.SUBPIX_REVERTED).any()  # 2 px from the corner with a 3 x 3 window: some drift away


def test_a_window_beyond_the_slice_is_refused():
    img = np.zeros((100, 100), np.uint8)
    imgproc.corner_sub_pix(img, np.full((1, 2), 50, np.float32), win=(30, 30))
    with pytest.raises(ValueError, match="patch"):
        imgproc.corner_sub_pix(img, np.full((1, 2), 50, np.float32), win=(31, 31))
    with pytest.raises(ValueError):
        imgproc.corner_sub_pix(img[:12], np.full((1, 2), 5, np.float32))


@pytest.mark.parametrize("zone", [(-1, -1), (0, 0), (1, 1)])
def test_zero_zones(zone):
    f = sc.frame(2)
    same(imgproc.corner_sub_pix(f["img"], f["seeds"], zero_zone=zone, return_info=True), want(f["img"], f["seeds"], zero_zone=zone))


@pytest.mark.parametrize("crit", [(30, 0.01), (3, 30, 0.01), (2, None), (1, 2, 0.0), (None, 0.05), (2, 0, 0.05), (100, 0.0)])
def test_criteria(crit):
    f = sc.frame(0)
    got = imgproc.corner_sub_pix(f["img"], f["seeds"], criteria=crit, return_info=True)
    same(got, want(f["img"], f["seeds"], crit=crit))
    if crit[:2] in ((2, None), (1, 2)):
        assert (got[1] == 2).all()


def test_a_13x13_image_with_corners_near_each_border():
    img, starts = sc.small_corner()
    got = imgproc.corner_sub_pix(img, starts, return_info=True)
    same(got, want(img, starts))
    assert (got[2][-3:] == 0).all() and np.abs(got[0][-3:] - (6.3, 6.6)).max() < 0.1


def test_status_bits():
    S = imgproc
    flat = np.full((20, 24), 77, np.uint8)
    c = np.array([[5.5, 6.25], [0, 0], [23.9, 19.9]], np.float32)
    got = imgproc.corner_sub_pix(flat, c, return_info=True)
    same(got, want(flat, c))
    assert (got[2] == S.SUBPIX_SINGULAR).all() and (got[1] == 1).all() and np.array_equal(got[0], c)
    img, starts = sc.slanted_edge()
    got = imgproc.corner_sub_pix(img, starts, return_info=True)
    same(got, want(img, starts))
    assert (got[2][:2] == S.SUBPIX_LEFT_IMAGE).all() and (got[0][:2, 0] < 0).all()
    assert (got[2][2:] == S.SUBPIX_LEFT_IMAGE | S.SUBPIX_REVERTED).all() and np.array_equal(got[0][2:], starts[2:])
    f = sc.frame(0)
    got = imgproc.corner_sub_pix(f["img"], f["seeds"], win=(1, 1), return_info=True)
    drifted = got[2] == S.SUBPIX_REVERTED
    assert drifted.any() and np.array_equal(got[0][drifted], f["seeds"][drifted])
    # starts that are no pixel of the image: returned as they came, float64 ones to the last bit
    for dtype in (np.float32, np.float64):
        bad = np.array([[np.nan, 5], [5, np.inf], [-0.001, 5], [5, -3], [sc.W, 5], [5, sc.H], [-np.inf, np.nan], [1e30, 1 / 3]], dtype)
        mixed = np.concatenate([bad[:4], f["seeds"][:3].astype(dtype), bad[4:]])
        got = imgproc.corner_sub_pix(f["img"], mixed, return_info=True)
        same(got, want(f["img"], mixed))
        at = np.r_[0:4, 7:11]
        assert (got[2][at] == S.SUBPIX_BAD_START).all() and (got[1][at] == 0).all() and (got[2][4:7] == 0).all()
        assert np.array_equal(got[0][at].view(np.uint8), bad.view(np.uint8))


def test_pitched_images_float64_corners_numpy_and_cuda(rendered):
    images, seeds, _, exp = rendered
    # a crop of a wider, taller batch: rows and images apart by more than their bytes
    big = torch.full((3, sc.H + 7, sc.W + 9), 255, dtype=torch.uint8, device="cuda")
    big[:, 3:3 + sc.H, 5:5 + sc.W] = torch.from_numpy(images).cuda()
    view = big[:, 3:3 + sc.H, 5:5 + sc.W]
    assert not view.is_contiguous()
    t = imgproc.corner_sub_pix(view, torch.from_numpy(seeds).cuda(), return_info=True)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in t)
    same(t, exp)
    same(imgproc.corner_sub_pix(view[1], torch.from_numpy(seeds[1]).cuda(), return_info=True), [a[1] for a in exp])
    # float64 corners hold the float32 result exactly; a float64 start is rounded to float32 first
    s64 = sc.batch()[2] + 1.2345678901234567
    got = imgproc.corner_sub_pix(images, s64, return_info=True)
    assert got[0].dtype == np.float64
    same(got, want(images, s64, frame_of=np.repeat(np.arange(3), 12)))
    as32 = imgproc.corner_sub_pix(images, s64.astype(np.float32), return_info=True)
    assert np.array_equal(got[0], as32[0].astype(np.float64)) and np.array_equal(got[1], as32[1])
    same(imgproc.corner_sub_pix(torch.from_numpy(images).cuda(), torch.from_numpy(s64).cuda(), return_info=True), got)


@pytest.mark.parametrize("shape", [(5, 7), (17, 33)])
def test_cvt_gray(shape):
    rng = np.random.default_rng(shape[0])
    img = rng.integers(0, 256, (2,) + shape + (3,), dtype=np.uint8)
    img[0, 0, :3] = [[255, 255, 255], [0, 0, 0], [255, 0, 255]]
    for code in ("bgr", "rgb"):
        exp = ref.gray(img, code)
        got = imgproc.cvt_gray(img, code)
        assert got.dtype == np.uint8 and np.array_equal(got, exp)
        assert np.array_equal(imgproc.cvt_gray(img[1], code), exp[1])
        # pitched: a crop of a wider batch, at an odd byte offset
        big = torch.zeros((2, shape[0] + 3, shape[1] + 5, 3), dtype=torch.uint8, device="cuda")
        big[:, 2:2 + shape[0], 3:3 + shape[1]] = torch.from_numpy(img).cuda()
        view = big[:, 2:2 + shape[0], 3:3 + shape[1]]
        assert not view.is_contiguous()
        t = imgproc.cvt_gray(view, code)
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), exp)
    assert not np.array_equal(ref.gray(img, "bgr"), ref.gray(img, "rgb"))
    try:
        imgproc.GRAY_BITS = 14
        assert np.array_equal(imgproc.cvt_gray(img), ref.gray(img, "bgr", bits=14))
    finally:
        imgproc.GRAY_BITS = 15


def test_a_colour_image_is_gray_then_refine(rendered):
    images, seeds, _, _ = rendered
    rgb = np.stack([sc.colour(i) for i in images])
    gray = imgproc.cvt_gray(rgb, "bgr")
    assert np.array_equal(gray, ref.gray(rgb, "bgr"))
    exp = want(gray, seeds, frame_of=np.repeat(np.arange(3), 12))
    same(imgproc.corner_sub_pix(rgb, seeds, return_info=True), exp)
    same(imgproc.corner_sub_pix(rgb[0], seeds[0], return_info=True), [a[0] for a in exp])
    same(imgproc.corner_sub_pix(torch.from_numpy(rgb).cuda(), torch.from_numpy(seeds).cuda(), return_info=True), exp)


def test_chessboard_find_image_points_and_batch(rendered):
    images, seeds, truth, exp = rendered
    board = ca.Chessboard((sc.COLS, sc.ROWS))
    assert np.allclose(board.object_points, sc.object_points(), atol=1e-8)
    for key, guess in (("coarse_corners", seeds[0]), ("corners", seeds[0][:, None])):
        d = {"img": images[0], key: guess}
        board.find_image_points(d)
        assert d["corners"].shape == (12, 1, 2) and d["corners"].dtype == np.float32
        assert np.array_equal(d["image_points"], exp[0][0]) and np.array_equal(d["corners"][:, 0], d["image_points"])
        assert d["object_points"] is board.object_points
    # the reference hands its RGB image to COLOR_BGR2GRAY: channel 0 gets blue's weight
    rgb = sc.colour(images[1])
    d = dict(img=rgb, coarse_corners=seeds[1])
    board.find_image_points(d)
    assert np.array_equal(d["image_points"], want(ref.gray(rgb, "bgr"), seeds[1])[0])
    d = dict(img=torch.from_numpy(images[2]).cuda(), coarse_corners=seeds[2])
    board.find_image_points(d)
    assert isinstance(d["image_points"], np.ndarray) and np.array_equal(d["image_points"], exp[0][2])
    same(board.find_image_points_batch(images, seeds, return_info=True), exp)
    assert np.array_equal(board.find_image_points_batch(images, seeds), exp[0])
    # a region of interest: the guess and the result are in the whole image's pixels
    roi = ca.Chessboard.get_roi_class((8, 92, 12, 124))((sc.COLS, sc.ROWS))
    whole = images[0]
    d = dict(img=whole, coarse_corners=seeds[0])
    roi.find_image_points(d)
    crop = np.ascontiguousarray(whole[8:92, 12:124])
    inner = want(crop, (seeds[0] - np.float32([12, 8])).astype(np.float32))[0]
    assert d["img"] is whole and np.array_equal(d["image_points"], np.float32(inner + (12, 8)))
    assert np.array_equal(d["coarse_corners"], seeds[0])


def test_rendered_frames_refine_calibrate():
    n = len(sc.POSES)
    frames = [sc.frame(i) for i in range(n)]
    images, seeds = np.stack([f["img"] for f in frames]), np.stack([f["seeds"] for f in frames])
    board = ca.Chessboard((sc.COLS, sc.ROWS))
    gpu = board.find_image_points_batch(images, seeds)
    cpu = want(images, seeds, frame_of=np.repeat(np.arange(n), 12))[0]
    assert np.array_equal(gpu, cpu)
    rms = []
    for corners in (gpu, cpu):
        cam = ca.Cam.from_detections({i: dict(image_points=corners[i], object_points=board.object_points) for i in range(n)},
                                     (sc.W, sc.H), undistorted=True).calibrate()
        rms.append(cam.retval)
        assert np.isfinite(cam.K).all() and all("T" in cam[i] for i in range(n))
    print("calibrate RMS", rms, "K", cam.K.tolist())
    assert rms[0] == rms[1] and rms[0] < 0.5
    assert abs(cam.K[0, 0] - sc.K[0, 0]) < 0.1 * sc.K[0, 0]
