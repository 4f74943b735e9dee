"""The chessboard detector on the MI355X (-m gpu): ``imgproc.chess_response``, ``chess_peaks``, ``find_chessboard_corners``
and ``boards.Chessboard(detector="chess")`` against the NumPy restatement tests/chessboard_ref.py -- response plane,
per-frame maximum, candidate list, counts, status, found and corners bit for bit: every value is an integer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import imgproc  # noqa: E402

import chessboard_cases as cc  # noqa: E402
import chessboard_ref as ref  # noqa: E402
import subpix_cases as sc  # noqa: E402
import subpix_ref  # noqa: E402


def host(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def same(got, exp, what=""):
    got, exp = np.ascontiguousarray(np.atleast_1d(host(got))), np.ascontiguousarray(np.atleast_1d(exp))
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape, exp.dtype, exp.shape)
    assert np.array_equal(got.view(np.uint8), exp.view(np.uint8)), (what, got, exp)


def check_all(images, pattern, exp=None, **kw):
    """every stage of the GPU path on ``images`` (f, h, w) against the restatement"""
    exp = ref.find(images, pattern, **kw) if exp is None else exp
    r, rmax = imgproc.chess_response(images)
    same(r, exp["response"], "response")
    same(rmax, exp["rmax"], "rmax")
    peaks, counts = imgproc.chess_peaks(r, rmax, **kw)
    same(peaks, exp["peaks"], "peaks")
    same(counts, exp["counts"], "counts")
    found, corners, status, counts = imgproc.find_chessboard_corners(images, pattern, return_info=True, **kw)
    same(found, exp["found"], "found")
    same(corners, exp["corners"], "corners")
    same(status, exp["status"], "status")
    same(counts, exp["counts"], "counts")
    return exp


@pytest.fixture(scope="module")
def mixed():
    images, names = cc.mixed_batch()
    exp = ref.find(images, cc.PATTERN)
    for a in exp.values():
        a.setflags(write=False)
    return images, names, exp


def test_every_fixture_in_one_batch_equals_the_restatement(mixed):
    images, names, exp = mixed
    check_all(images, cc.PATTERN, exp)
    assert exp["found"].tolist() == [k in cc.boards() for k in names]
    truth = np.stack([cc.boards()[k][1] for k in cc.boards()])
    got = imgproc.find_chessboard_corners(images, cc.PATTERN)[1][:len(truth)]
    assert np.abs(got - truth).max() <= cc.MAX_OFFSET


def test_a_frame_alone_and_at_any_place_of_a_batch(mixed):
    images, names, exp = mixed
    keys = ("found", "corners", "status", "counts")
    for k in (0, len(names) - 3, len(names) - 1):  # a found frame, the blank one, the last
        alone = imgproc.find_chessboard_corners(images[k], cc.PATTERN, return_info=True)
        assert isinstance(alone[0], bool) and alone[1].shape == (12, 2)
        for key, a in zip(keys, alone):
            same(np.asarray(a), exp[key][k], (names[k], key))
        r, rmax = imgproc.chess_response(images[k])
        same(r, exp["response"][k])
        same(rmax, exp["rmax"][k])
    order = np.array([9, 0, 10, 5, 8, 3, 11, 1])
    got = imgproc.find_chessboard_corners(images[order], cc.PATTERN, return_info=True)
    for key, g in zip(keys, got):
        same(g, exp[key][order], key)


def test_a_square_pattern(mixed):
    img, truth = cc.square_board()
    exp = check_all(img[None], cc.SQUARE_PATTERN)
    assert exp["found"].tolist() == [True] and np.abs(exp["corners"][0] - truth).max() <= cc.MAX_OFFSET


def test_numpy_cuda_and_colour_inputs_agree(mixed):
    images, names, exp = mixed
    t = torch.from_numpy(images).cuda()
    got = imgproc.find_chessboard_corners(t, cc.PATTERN, return_info=True)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got) and got[0].dtype == torch.bool
    for key, g in zip(("found", "corners", "status", "counts"), got):
        same(g, exp[key], key)
    one = imgproc.find_chessboard_corners(t[1], cc.PATTERN)
    assert one[0].shape == () and bool(one[0]) and np.array_equal(host(one[1]), exp["corners"][1])
    r, rmax = imgproc.chess_response(t)
    assert r.is_cuda and rmax.is_cuda
    same(r, exp["response"])
    # colour: the detector sees cvt_gray's image
    rgb = np.stack([sc.colour(i) for i in images[:3]])
    gray = subpix_ref.gray(rgb, "bgr")
    want = ref.find(gray, cc.PATTERN)
    for rgb_in in (rgb, torch.from_numpy(rgb).cuda()):
        got = imgproc.find_chessboard_corners(rgb_in, cc.PATTERN, return_info=True)
        for key, g in zip(("found", "corners", "status", "counts"), got):
            same(g, want[key], key)
        same(imgproc.chess_response(rgb_in)[0], want["response"])
    same(imgproc.find_chessboard_corners(rgb[0], cc.PATTERN)[1], want["corners"][0])


def test_odd_sizes_strides_and_tile_edges():
    # 133 x 101: no multiple of the 128 x 32 tile, of four pixels or of a dword; a view whose rows and frames lie apart
    rng = np.random.default_rng(7)
    big = rng.integers(0, 256, (3, 101 + 6, 133 + 10), dtype=np.uint8)
    big[1, 2:2 + sc.H, 3:3 + sc.W] = cc.boards()["pose2"][0]
    view = torch.from_numpy(big).cuda()[:, 2:2 + 101, 3:3 + 133]
    assert not view.is_contiguous()
    tight = np.ascontiguousarray(big[:, 2:2 + 101, 3:3 + 133])
    exp = ref.find(tight, cc.PATTERN, relative=4, nms_radius=2)
    r, rmax = imgproc.chess_response(view)
    same(r, exp["response"])
    same(rmax, exp["rmax"])
    check_all(tight, cc.PATTERN, exp, relative=4, nms_radius=2)
    got = imgproc.find_chessboard_corners(view[::2], cc.PATTERN, 4, 2, return_info=True)  # frames two apart
    for key, g in zip(("found", "corners", "status", "counts"), got):
        same(g, exp[key][::2], key)
    # a dword-aligned pitch with an unaligned width, and an image narrower than a halo
    wide = torch.from_numpy(big).cuda()[:, :96, 4:4 + 126]
    same(imgproc.chess_response(wide)[0], ref.response(np.ascontiguousarray(big[:, :96, 4:4 + 126]))[0])
    for shape in ((1, 7, 300), (2, 40, 9), (1, 33, 129)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        r, rmax = imgproc.chess_response(img)
        e = ref.response(img)
        same(r, e[0], shape)
        same(rmax, e[1], shape)


def test_ties_and_every_window_radius():
    r, rmax, radius1, radius2 = cc.tie_plane()
    for radius, want in ((1, radius1), (2, radius2), (8, None)):
        exp = ref.peaks(r, rmax, 8, radius)
        peaks, counts = imgproc.chess_peaks(r, rmax, 8, radius)
        same(peaks, exp[0])
        same(counts, exp[1])
        if want is not None:
            assert peaks[0, :len(want)].tolist() == [list(p) for p in want]
    planes = np.random.default_rng(1).integers(-50, 60, (3, 37, 41)).astype(np.int16)  # many equal neighbours
    pmax = planes.reshape(3, -1).max(1).astype(np.int32)
    for relative, radius in ((1, 1), (8, 3), (64, 5)):
        exp = ref.peaks(planes, pmax, relative, radius)
        peaks, counts = imgproc.chess_peaks(torch.from_numpy(planes).cuda(), torch.from_numpy(pmax).cuda(), relative, radius)
        same(peaks, exp[0])
        same(counts, exp[1])


def test_more_candidates_than_the_capacity():
    """A fine checker of 12 px squares: at 256 x 256 it has 20 x 20 corners, which the 1024 kept per frame still hold
    (status 4, another size); at 512 x 512 it has 42 x 42 = 1764 and overflows (status 2).  Both in one call, padded to a
    batch, with a board between them."""
    images = np.full((3, 512, 512), sc.PAPER, np.uint8)
    images[0] = cc.fine_checker(512)
    images[1, :256, :256] = cc.fine_checker(256)
    images[2, 100:100 + sc.H, 200:200 + sc.W] = cc.boards()["pose0"][0]
    exp = check_all(images, cc.PATTERN)
    assert exp["counts"].tolist()[0] == 42 * 42 and exp["status"].tolist() == [ref.OVERFLOW, ref.INCOMPLETE, ref.FOUND]
    assert exp["counts"][1] < ref.CAPACITY
    small = check_all(cc.fine_checker(256)[None], cc.PATTERN)
    assert small["counts"].tolist() == [400] and small["status"].tolist() == [ref.INCOMPLETE]
    big = check_all(cc.fine_checker(256)[None], (20, 20))  # the whole checker as one board of 400 corners
    assert big["status"].tolist() == [ref.FOUND]


def test_limits_are_refused():
    img = cc.boards()["pose0"][0]
    for kw in (dict(pattern=(1, 12)), dict(pattern=(32, 17)), dict(relative=65), dict(nms_radius=0)):
        with pytest.raises(ValueError):
            imgproc.find_chessboard_corners(img, **dict(dict(pattern=cc.PATTERN), **kw))
    found, corners = imgproc.find_chessboard_corners(img, (32, 16))  # the largest pattern: 512 corners, none here
    assert found is False and corners.shape == (512, 2) and np.isnan(corners).all()


def test_find_image_points_batch_detects_then_refines(mixed):
    images, names, exp = mixed
    board = ca.Chessboard(cc.PATTERN)
    found, corners = board.find_image_points_batch(images)
    same(found, exp["found"])
    want = subpix_ref.corner_sub_pix(images, exp["corners"].reshape(-1, 2), frame_of=np.repeat(np.arange(len(images)), 12),
                                     order="wave")
    same(corners, want[0].reshape(-1, 12, 2))
    assert np.isnan(corners[~found]).all() and np.isfinite(corners[found]).all()
    same(corners[found], imgproc.corner_sub_pix(images[found], exp["corners"][found], (4, 4), (-1, -1), (3, 30, 0.01)))
    info = board.find_image_points_batch(torch.from_numpy(images).cuda(), return_info=True)
    assert len(info) == 6 and all(v.is_cuda for v in info)
    for g, e in zip(info, (exp["found"], want[0].reshape(-1, 12, 2), want[1].reshape(-1, 12), want[2].reshape(-1, 12),
                           exp["status"], exp["counts"])):
        same(g, e)
    # a coarse guess is taken as before
    seeds = sc.batch()[1]
    same(board.find_image_points_batch(sc.batch()[0], seeds), subpix_ref.corner_sub_pix(
        sc.batch()[0], seeds.reshape(-1, 2), frame_of=np.repeat(np.arange(3), 12), order="wave")[0].reshape(3, 12, 2))


def test_a_chess_board_detects_refines_and_calibrates(mixed):
    n = len(sc.POSES)
    images = np.stack([sc.frame(i)["img"] for i in range(n)])
    seeds = ref.find(images, cc.PATTERN)["corners"]
    assert np.isfinite(seeds).all()
    plain, chess = ca.Chessboard(cc.PATTERN), ca.Chessboard(cc.PATTERN, detector="chess")
    cams = []
    for board, guess in ((plain, seeds), (chess, [None] * n)):
        records = {i: dict(img=images[i]) for i in range(n)}
        for i in range(n):
            if guess[i] is not None:
                records[i]["coarse_corners"] = guess[i]
            board.find_image_points(records[i])
        cams.append((records, ca.Cam.from_detections(records, (sc.W, sc.H), undistorted=True).calibrate()))
    (rec_a, cam_a), (rec_b, cam_b) = cams
    for i in range(n):
        same(rec_b[i]["image_points"], rec_a[i]["image_points"])
        assert rec_b[i]["corners"].shape == (12, 1, 2) and rec_b[i]["object_points"] is chess.object_points
        same(np.asarray(cam_b[i]["T"]), np.asarray(cam_a[i]["T"]))
    assert cam_a.retval == cam_b.retval and cam_b.retval < 0.5
    same(np.asarray(cam_b.K), np.asarray(cam_a.K))
    assert abs(cam_b.K[0, 0] - sc.K[0, 0]) < 0.1 * sc.K[0, 0]
    same(chess.detect_corners(images[0]), seeds[0])
    # a frame without the board: the record gets no image points, as after the reference's `if ok`
    for img in (cc.blank(), torch.from_numpy(cc.cut_board()).cuda()):
        d = dict(img=img)
        chess.find_image_points(d)
        assert set(d) == {"img"} and chess.detect_corners(img) is None
    d = dict(img=torch.from_numpy(images[1]).cuda())
    chess.find_image_points(d)
    same(d["image_points"], rec_a[1]["image_points"])
    # a region of interest: detected inside the window, reported in the whole image's pixels
    roi = ca.Chessboard.get_roi_class((4, 92, 8, 124))(cc.PATTERN, detector="chess")
    whole = images[0]
    d = dict(img=whole)
    roi.find_image_points(d)
    crop = np.ascontiguousarray(whole[4:92, 8:124])
    inner = ref.find(crop, cc.PATTERN)["corners"][0]
    want = subpix_ref.corner_sub_pix(crop, inner, order="wave")[0]
    assert d["img"] is whole and np.array_equal(d["image_points"], np.float32(want + (8, 4)))
    with pytest.raises(NotImplementedError):
        plain.find_image_points(dict(img=images[0]))
