"""The chessboard detector without a GPU: its NumPy restatement (tests/chessboard_ref.py) on rendered boards with analytic
corners, the frames it must not find a board in, the tie rule of the peaks, and the refusals of the Python and C entries.

The bound on a detected corner, 2 px per axis from the analytic one (``subpix_cases.MAX_SEED_OFFSET``), is the seed
offset the refinement is shown to converge from (tests/test_subpix_cpu.py); measured here: at most 1.18 px."""
import numpy as np
import pytest

import chessboard_cases as cc
import chessboard_ref as ref
import subpix_cases as sc

BOARDS = list(cc.boards())


def check_found(img, truth, pattern):
    got = ref.find(img, pattern)
    n = pattern[0] * pattern[1]
    assert got["status"].tolist() == [ref.FOUND] and got["found"].tolist() == [True] and got["counts"][0] >= n
    corners = got["corners"][0]
    assert corners.dtype == np.float32 and corners.shape == (n, 2) and np.array_equal(corners, np.rint(corners))
    off = np.abs(corners - truth).max()
    print("largest offset per axis: %.3f px, %d candidates" % (off, got["counts"][0]))
    assert off <= cc.MAX_OFFSET
    assert corners.min() >= ref.BORDER and (corners.max(0) < (sc.W - ref.BORDER, sc.H - ref.BORDER)).all()


@pytest.mark.parametrize("name", BOARDS)
def test_the_restatement_finds_every_board_in_the_rules_order(name):
    img, truth = cc.boards()[name]
    check_found(img, truth, cc.PATTERN)


def test_a_square_pattern_has_four_numberings_and_the_rule_picks_one():
    img, truth = cc.square_board()
    check_found(img, truth, cc.SQUARE_PATTERN)
    # the same picture is no 4 x 3 board: 16 candidates, a lattice of another size
    got = ref.find(img, cc.PATTERN)
    assert got["status"].tolist() == [ref.INCOMPLETE] and np.isnan(got["corners"]).all()


def test_turned_views_are_numbered_from_the_corner_that_comes_first_in_pixel_order():
    for name in ("quarter_turn", "half_turn", "quarter_turn_back"):
        c = ref.find(cc.boards()[name][0], cc.PATTERN)["corners"][0].reshape(sc.ROWS, sc.COLS, 2)
        other = c[-1, -1]  # the half turn's corner 0
        assert c[0, 0, 1] * sc.W + c[0, 0, 0] < other[1] * sc.W + other[0]
        row, col = (c[:, -1] - c[:, 0]).sum(0), (c[-1] - c[0]).sum(0)
        assert row[0] * col[1] - row[1] * col[0] > 0  # right-handed, y down
    quarter = ref.find(cc.boards()["quarter_turn"][0], cc.PATTERN)["corners"][0].reshape(sc.ROWS, sc.COLS, 2)
    assert abs(quarter[0, -1, 1] - quarter[0, 0, 1]) > abs(quarter[0, -1, 0] - quarter[0, 0, 0])  # "across" runs down the image


def test_frames_without_a_whole_board():
    got = ref.find(cc.blank(), cc.PATTERN)
    assert got["status"].tolist() == [ref.FEW] and got["counts"].tolist() == [0] and got["rmax"].tolist() == [0]
    assert not got["found"][0] and np.isnan(got["corners"]).all()
    got = ref.find(cc.cut_board(), cc.PATTERN)
    assert not got["found"][0] and got["status"][0] in (ref.FEW, ref.INCOMPLETE) and np.isnan(got["corners"]).all()
    images, names = cc.mixed_batch()
    got = ref.find(images, cc.PATTERN)
    assert got["found"].tolist() == [k in cc.boards() for k in names]
    for k in range(len(names)):  # a frame's result does not depend on its place
        alone = ref.find(images[k], cc.PATTERN)
        for key in ("response", "rmax", "peaks", "counts", "corners", "status"):
            assert np.array_equal(got[key][k], alone[key][0], equal_nan=True), (names[k], key)


def test_more_candidates_than_the_capacity():
    small = ref.find(cc.fine_checker(256), cc.PATTERN)  # 20 x 20 corners: no overflow yet
    assert small["counts"].tolist() == [400] and small["status"].tolist() == [ref.INCOMPLETE]
    got = ref.find(cc.fine_checker(512), cc.PATTERN)
    assert got["counts"].tolist() == [42 * 42] and got["status"].tolist() == [ref.OVERFLOW] and not got["found"][0]
    assert (got["peaks"][0] >= 0).all()  # the first 1024 in pixel order are kept
    index = got["peaks"][0, :, 1] * 512 + got["peaks"][0, :, 0]
    assert (np.diff(index) > 0).all()


def test_the_response_is_an_int16_that_vanishes_near_the_borders():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (2, 23, 31), dtype=np.uint8)
    r, rmax = ref.response(img)
    assert r.dtype == np.int16 and rmax.dtype == np.int32 and (rmax >= 0).all()
    inner = np.zeros(r.shape, bool)
    inner[:, 5:-5, 5:-5] = True
    assert (r[~inner] == 0).all() and (r[inner] != 0).any()
    # the extremes of the range: a ring that alternates in quarters, and a dot on the opposite ground
    x, y = np.meshgrid(np.arange(11) - 5, np.arange(11) - 5)
    assert ref.response(np.where((x + 0.5) * (y + 0.5) > 0, 255, 0).astype(np.uint8))[0][5, 5] > 0
    dot = np.zeros((11, 11), np.uint8)
    dot[4:7, 4:7] = 255
    assert ref.response(dot)[0][5, 5] == -16 * 5 * 255
    half = np.where(x > 0, 255, 0).astype(np.uint8)
    assert ref.response(half)[0][5, 5] < 0
    assert ref.response(np.zeros((10, 40), np.uint8))[0].any() == 0  # no pixel 5 from both borders


def test_of_equal_responses_the_first_in_pixel_order_is_the_peak():
    r, rmax, radius1, radius2 = cc.tie_plane()
    for radius, want in ((1, radius1), (2, radius2)):
        peaks, counts = ref.peaks(r, rmax, 8, radius)
        assert counts.tolist() == [len(want)] and peaks[0, :len(want)].tolist() == [list(p) for p in want]
        assert (peaks[0, len(want):] == -1).all()
    peaks, counts = ref.peaks(r, rmax, 9, 1)  # 9 * 99 >= 800
    assert counts[0] == len(radius1) + 1 and [8, 10] in peaks[0, :counts[0]].tolist()


def test_lattice_ties_go_to_the_lowest_candidate_index():
    # an exact lattice of 3 x 3 with 10 px steps: every distance ties; candidates come in pixel order
    pts = np.array([(x, y) for y in (10, 20, 30) for x in (10, 20, 30)])
    corners, status = ref.lattice_one(pts, 64, 3, 3)
    assert status == ref.FOUND and np.array_equal(corners, pts)
    # one candidate short, one too many
    assert ref.lattice_one(pts[:8], 64, 3, 3) == (None, ref.FEW)
    more = np.concatenate([pts, [(40, 10)]])
    assert ref.lattice_one(more[np.lexsort((more[:, 0], more[:, 1]))], 64, 3, 3)[1] == ref.INCOMPLETE
    # a 4 x 2 board lying along y: "across" follows the long side, right-handed
    tall = np.array([(x, y) for y in (10, 20, 30, 40) for x in (10, 20)])
    corners, status = ref.lattice_one(tall, 64, 4, 2)
    assert status == ref.FOUND and corners[0].tolist() == [20, 10] and corners[3].tolist() == [20, 40] and corners[4].tolist() == [10, 10]
    # collinear candidates have no second direction
    line = np.array([(10 * k, 7) for k in range(1, 7)])
    assert ref.lattice_one(line, 64, 3, 2) == (None, ref.INCOMPLETE)


BAD_ARGUMENTS = [dict(pattern=(1, 5)), dict(pattern=(4, 1)), dict(pattern=(32, 17)), dict(pattern=(4,)), dict(pattern=4),
                 dict(pattern=(4.5, 3)), dict(relative=0), dict(relative=65), dict(nms_radius=0), dict(nms_radius=9),
                 dict(relative=2.5)]


def test_arguments_are_refused_before_the_library_is_loaded(monkeypatch):
    from calibrating_amd import _native, imgproc

    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_native, "lib", no_library)
    monkeypatch.setattr(_native, "require_device", no_library)
    img = np.zeros((40, 50), np.uint8)
    for kw in BAD_ARGUMENTS:
        kw = dict(dict(pattern=(4, 3)), **kw)
        with pytest.raises(ValueError):
            imgproc.find_chessboard_corners(img, **kw)
    for images in (img.astype(np.int16), img[None, None, None], np.zeros((2, 3, 4, 5), np.uint8), np.zeros((0, 50), np.uint8),
                   np.zeros((1, 16385), np.uint8)):
        with pytest.raises(ValueError):
            imgproc.find_chessboard_corners(images, (4, 3))
        if images.shape[-1] != 16385:
            with pytest.raises(ValueError):
                imgproc.chess_response(images)
    with pytest.raises(TypeError):
        imgproc.find_chessboard_corners([[0]], (4, 3))
    import torch
    with pytest.raises(ValueError, match="GPU"):
        imgproc.find_chessboard_corners(torch.zeros((40, 50), dtype=torch.uint8), (4, 3))
    r, rmax = np.zeros((1, 8, 8), np.int16), np.zeros(1, np.int32)
    for a, b, kw in ((r, rmax, dict(relative=0)), (r, rmax, dict(nms_radius=9)), (r.astype(np.int32), rmax, {}), (r[0], rmax, {}),
                     (r, np.zeros(2, np.int32), {}), (r, rmax.astype(np.int64), {})):
        with pytest.raises(ValueError):
            imgproc.chess_peaks(a, b, **kw)
    import calibrating_amd as ca
    with pytest.raises(ValueError):
        ca.Chessboard((4, 3), detector="quads")
    with pytest.raises(ValueError):
        ca.Chessboard((1, 3), detector="chess").detect_corners(img)
    # the restatement refuses the same
    for kw in BAD_ARGUMENTS:
        kw = dict(dict(pattern=(4, 3), relative=8, nms_radius=3), **kw)
        with pytest.raises((ValueError, TypeError)):
            ref.check_arguments(**kw)


def test_the_c_entries_refuse_before_they_probe_the_device():
    from calibrating_amd import _native
    lib = _native.lib()
    A = lambda k: 0x7000000000 + (k << 20)  # made-up device addresses, never read
    U, B = _native.CAMD_ERR_UNSUPPORTED, _native.CAMD_ERR_BAD_ARG

    def lattice(across=4, down=3, w=128, h=96, frames=2, peaks=A(0)):
        return lib.camd_chess_lattice(peaks, A(1), w, h, frames, across, down, A(2), A(3), None)
    for kw in (dict(across=1), dict(down=1), dict(across=32, down=17), dict(across=-4, down=-3), dict(w=16385), dict(h=16385)):
        assert lattice(**kw) == U, kw
    for kw in (dict(frames=0), dict(peaks=None), dict(peaks=A(0) + 2), dict(w=0)):
        assert lattice(**kw) == B, kw

    def peaks(relative=8, radius=3, w=128, h=96, frames=2, ws=A(4)):
        return lib.camd_chess_peaks(A(0), A(1), w, h, frames, relative, radius, ws, A(2), A(3), None)
    for kw in (dict(relative=0), dict(relative=65), dict(radius=0), dict(radius=9)):
        assert peaks(**kw) == U, kw
    assert "nms_radius" in _native.last_error()
    for kw in (dict(ws=None), dict(ws=A(4) + 4), dict(h=0), dict(frames=1 << 20, h=1 << 11)):
        assert peaks(**kw) == B, kw

    def response(w=128, h=96, pitch=128, stride=128 * 96, frames=2, gray=A(0), out=A(1)):
        return lib.camd_chess_response(gray, w, h, pitch, stride, frames, out, A(2), None)
    for kw in (dict(w=0), dict(pitch=127), dict(stride=128 * 95), dict(frames=0), dict(gray=None), dict(out=A(1) + 1)):
        assert response(**kw) == B, kw
    assert lib.camd_chess_peaks_workspace_bytes(96, 2) >= 2 * 96 * 12 + 8 and lib.camd_chess_peaks_workspace_bytes(0, 2) == 0


def test_the_default_board_still_refuses_and_only_chess_is_another_detector():
    import calibrating_amd as ca
    from calibrating_amd import boards
    board = ca.Chessboard((4, 3))
    assert board.detector is None and board.init_kwargs == dict(checkboard=(4, 3), size_mm=25)
    with pytest.raises(NotImplementedError) as e:
        board.find_image_points({"img": sc.frame(0)["img"]})
    assert str(e.value) == boards.NO_QUAD_SEARCH
    chess = ca.Chessboard((4, 3), 25, detector="chess")
    assert chess.detector == "chess" and chess.init_kwargs["detector"] == "chess"
    assert np.array_equal(chess.object_points, board.object_points)
