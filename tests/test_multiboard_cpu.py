"""The restatement of the one-pass detector of several ChArUco boards (tests/multiboard_ref.py) against rendered scenes
with analytic corners (tests/multiboard_cases.py), without a GPU: the fixtures are known good before a kernel is held to
them.  With one board the restatement is ``charuco_ref``'s in every array; the Laplacian's sums against a double loop;
what the Python layer refuses before it touches a device."""
import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import boards, imgproc

import charuco_cases as cc
import charuco_ref
import multiboard_cases as mc
import multiboard_ref as ref
from chessboard_cases import MAX_OFFSET


@pytest.fixture(scope="module")
def detected():
    images, names = mc.batch()
    exp = ref.find(images, **mc.kwargs())
    for a in exp.values():
        a.setflags(write=False)
    return names, exp


def test_every_scene_reports_its_boards_by_name_and_id(detected):
    names, exp = detected
    for k, name in enumerate(names):
        mc.check_against_truth(name, exp["seen"][k], exp["corners"][k], MAX_OFFSET)
        present = mc.scene(name)["present"]
        assert (exp["status"][k][present] == ref.FOUND).all() and (exp["status"][k][~present] != ref.FOUND).all(), name
        assert (exp["marker_ids"][k][~present] == -1).all(), name
    row = exp["marker_ids"][names.index("row")]
    for b, first in enumerate(mc.SET3):  # the markers between inner corners, under their own board
        ids = row[b][row[b] >= 0]
        assert len(ids) >= 2 and (ids >= first).all() and (ids < first + 10).all()
    assert exp["counts"][names.index("few")] < charuco_ref.MIN_PEAKS and (exp["status"][names.index("few")] == ref.FEW).all()
    assert exp["counts"][names.index("plain")] >= charuco_ref.MIN_PEAKS
    assert (exp["status"][names.index("plain")] == ref.NO_LATTICE).all()
    # the centroid of the row falls in the middle board, and of the foreign scene in the board of no set
    assert exp["status"][names.index("foreign")].tolist() == [ref.FOUND, ref.FOUND, ref.NO_LATTICE]


def test_four_boards_two_by_two_tilted_and_turned():
    s = mc.scene("grid")
    exp = ref.find(s["img"], **mc.kwargs(mc.FIRST_IDS))
    assert exp["status"].tolist() == [[0, 0, 0, 0]] and exp["seen"].all()
    mc.check_against_truth("grid", exp["seen"][0], exp["corners"][0], MAX_OFFSET)


def test_one_board_is_the_single_board_restatement():
    images, _ = cc.mixed_batch()
    want = charuco_ref.find(images, **cc.SMALL.kwargs())
    got = ref.find(images, cc.SMALL.squares, cc.SMALL.dictionary, (cc.SMALL.first_id,), cc.SMALL.ratio)
    for key in ("peaks", "counts"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("corners", "marker_ids", "status"):
        assert got[key].shape[1] == 1 and got[key].dtype == want[key].dtype
        assert np.array_equal(got[key][:, 0].view(np.uint8), np.ascontiguousarray(want[key]).view(np.uint8)), key
    assert {ref.FOUND, ref.NO_LATTICE, ref.FEW} <= set(want["status"].tolist())


@pytest.mark.parametrize("shape", [(2, 2), (3, 5), (17, 13)])
def test_laplacian_sums_against_a_double_loop(shape):
    g = np.random.default_rng(shape[0]).integers(0, 256, shape, dtype=np.uint8)
    h, w = shape
    s1 = s2 = 0
    mirror = lambda i, n: -i if i < 0 else 2 * (n - 1) - i if i >= n else i  # noqa: E731
    for y in range(h):
        for x in range(w):
            at = lambda yy, xx: int(g[mirror(yy, h), mirror(xx, w)])  # noqa: E731
            lap = at(y, x - 1) + at(y, x + 1) + at(y - 1, x) + at(y + 1, x) - 4 * at(y, x)
            s1, s2 = s1 + lap, s2 + lap * lap
    assert ref.laplacian_sums(g) == (s1, s2)
    n = h * w
    assert abs((n * s2 - s1 * s1) / (n * n) - ref.laplacian(g).var()) <= 1e-12 * max(1.0, ref.laplacian(g).var())


def test_limits_are_refused_without_a_device():
    img = mc.scene("paper")["img"]
    base = dict(squares_xy=mc.SQUARES, dictionary=mc.DICTIONARY, marker_ratio=mc.RATIO)
    for first_ids in ((), tuple(range(0, 54, 6)), (1, 5), (1, 10), (49,), (-1,), (1.5,), 3):
        with pytest.raises(ValueError):
            imgproc.find_charuco_boards(img, first_ids=first_ids, **base)
        if not isinstance(first_ids, int):
            with pytest.raises(ValueError):
                ref.check_arguments(mc.SQUARES, mc.DICTIONARY, first_ids, mc.RATIO, 8, 3, 2)
    for kw in (dict(squares_xy=(2, 4)), dict(marker_ratio=(3, 3)), dict(min_markers=0), dict(relative=65)):
        with pytest.raises(ValueError):
            imgproc.find_charuco_boards(img, first_ids=mc.SET3, **dict(base, **kw))
    for bad in (np.zeros((1, 5), np.uint8), np.zeros((4, 1), np.uint8), np.zeros((4, 4), np.float32)):
        with pytest.raises(ValueError):
            imgproc.sharpness(bad)
    with pytest.raises(ValueError):
        ref.laplacian_sums(np.zeros((1, 5), np.uint8))
    with pytest.raises(ValueError):
        ca.MultiBoardsCam(["a.jpg"], [None])
    with pytest.raises(ValueError):
        ca.MultiBoardsCam({"a~b": img}, [None])


def test_which_boards_form_a_set():
    make = lambda first, **kw: ca.CharucoBoard(**dict(dict(square_xy=mc.SQUARES, square_size_mm=30.0, marker_size_mm=20.0,  # noqa: E731
                                                           dictionary=mc.DICTIONARY, first_id=first), **kw))
    assert ca.MultiBoards([make(k) for k in mc.SET3]).first_ids == list(mc.SET3)
    assert ca.MultiBoards({"b": make(1), "a": make(12)}).first_ids == [12, 1]  # (a dict: in the order of its sorted keys)
    assert ca.MultiBoards([make(1), make(12, dictionary=mc.DICTIONARY.copy())]).first_ids == [1, 12]  # equal bits
    for other in (make(5), make(12, square_size_mm=40.0, marker_size_mm=20.0), make(12, invert_color=True),
                  make(12, dictionary=boards.make_marker_dictionary(58, 4, 2)), ca.Chessboard((4, 3))):
        mb = ca.MultiBoards([make(1), other])
        assert mb.first_ids is None
        with pytest.raises(ValueError):
            mb.find_image_points_batch(np.zeros((1, 48, 64), np.uint8))
    assert ca.MultiBoards([make(k) for k in range(0, 54, 6)][:9]).first_ids is None
