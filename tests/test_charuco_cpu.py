"""The ChArUco detector's restatement (tests/charuco_ref.py) against rendered boards with analytic corners
(tests/charuco_cases.py), and the host side of ``boards.CharucoBoard``: no GPU."""
import numpy as np
import pytest

from calibrating_amd import boards

import charuco_cases as cc
import charuco_ref as ref
from chessboard_cases import MAX_OFFSET


@pytest.fixture(scope="module")
def mixed():
    images, names = cc.mixed_batch()
    exp = ref.find(images, **cc.SMALL.kwargs())
    for a in exp.values():
        a.setflags(write=False)
    return images, names, exp


def check_view(v, corners, marker_ids, found):
    seen = ~np.isnan(corners[:, 0])
    assert found and np.array_equal(seen, ~np.isnan(corners[:, 1]))
    assert np.abs(corners[seen] - v["truth"][seen]).max() <= MAX_OFFSET  # every reported corner is the one of its id
    assert not (v["required"] & ~seen).any()
    if v["whole"]:
        assert seen.all() and v["required"].all()
    setup = v["setup"]
    want = cc.marker_cells(setup)  # (only to know the squares with a marker)
    k = setup.first_id
    for y in range(setup.squares[1]):
        for x in range(setup.squares[0]):
            if x % 2 != y % 2:
                assert marker_ids[y * setup.squares[0] + x] in (-1, k)
                k += 1
            else:
                assert marker_ids[y * setup.squares[0] + x] == -1 and want[y, x].all()
    assert (marker_ids >= 0).sum() >= 2


def test_every_view_of_the_small_board(mixed):
    images, names, exp = mixed
    for k, name in enumerate(names):
        v = cc.expected(name)
        if v is None:
            assert not exp["found"][k] and np.isnan(exp["corners"][k]).all() and (exp["marker_ids"][k] == -1).all(), name
        else:
            check_view(v, exp["corners"][k], exp["marker_ids"][k], exp["found"][k])
    status = dict(zip(names, exp["status"].tolist()))
    assert status["blank"] == ref.FEW and status["one_marker"] == ref.NO_CONSENSUS and status["plain"] == ref.NO_LATTICE
    assert (~np.isnan(exp["corners"][names.index("covered")][:, 0])).sum() < cc.SMALL.n  # the cover does hide corners


@pytest.mark.parametrize("name", ["wide", "wide_cut"])
def test_the_wide_board_with_6x6_bits(name):
    v = cc.view(name)
    exp = ref.find(v["img"], **cc.WIDE.kwargs())
    check_view(v, exp["corners"][0], exp["marker_ids"][0], exp["found"][0])
    if name == "wide_cut":
        assert np.isnan(exp["corners"][0]).any() and v["required"].sum() >= 16


def test_a_frame_alone_equals_its_place_in_the_batch(mixed):
    images, names, exp = mixed
    for k in (1, len(names) - 1):
        one = ref.find(images[k], **cc.SMALL.kwargs())
        for key in ("corners", "marker_ids", "status", "counts"):
            assert np.array_equal(one[key][0], exp[key][k], equal_nan=True)


def test_dictionary_helpers():
    for n, s, need in ((13, 4, None), (25, 6, 10), (8, 7, None)):
        d = boards.make_marker_dictionary(n, s, seed=3, min_distance=need)
        need = s * s // 4 if need is None else need
        assert d.shape == (n, s, s) and d.dtype == np.uint8 and np.array_equal(d, boards.make_marker_dictionary(n, s, 3, need))
        for i in range(n):
            assert boards.marker_distance(d[i]) >= need
            for j in range(i):
                assert boards.marker_distance(d[i], d[j]) >= need
        packed = boards.marker_bytes_list(d)
        assert packed.shape == (n, (s * s + 7) // 8, 4) and packed.dtype == np.uint8
        assert np.array_equal(boards.marker_bits_from_bytes_list(packed, s), d)
        for k in range(1, 4):  # plane k: the marker turned k quarter turns clockwise
            turned = boards.marker_bits_from_bytes_list(np.roll(packed, -k, axis=2), s)
            assert np.array_equal(turned, np.rot90(d, -k, axes=(1, 2)))
        assert [int(w) for w in boards.marker_words(d)] == ref.words(d)
    assert not np.array_equal(boards.make_marker_dictionary(5, 4, 0), boards.make_marker_dictionary(5, 4, 1))
    # a last byte that is not full holds its bits in its low end: 36 bits, the last four in 0x0f
    one = np.zeros((1, 6, 6), np.uint8)
    one[0, 5, 2:] = 1
    assert boards.marker_bytes_list(one)[0, :, 0].tolist() == [0, 0, 0, 0, 0x0f]
    with pytest.raises(ValueError):
        boards.make_marker_dictionary(1024, 4, 0, 6)
    with pytest.raises(ValueError):
        boards.marker_bits_from_bytes_list(np.zeros((3, 2, 4), np.uint8), 5)


def test_object_points_and_refusals():
    d = boards.make_marker_dictionary(22, 4, 0)
    board = boards.CharucoBoard(dictionary=d)
    assert board.square_xy == (9, 5) and board.marker_ratio == (1, 2) and sorted(board.object_points) == list(range(32))
    x, y = np.meshgrid(np.arange(8), np.arange(4))
    grid = np.zeros((32, 3), np.float32)
    grid[:, 0], grid[:, 1] = (x.ravel() + 1) * (44.95 / 1000.0), (y.ravel() + 1) * (44.95 / 1000.0)
    grid -= grid.mean(0, keepdims=True)
    for i in range(32):
        p = board.object_points[i]
        assert p.shape == (1, 3) and p.dtype == np.float32 and np.array_equal(p[0], grid[i])
    assert len(board.marker_squares()) == 22 and board.marker_squares()[:5] == [(1, 0), (3, 0), (5, 0), (7, 0), (0, 1)]
    with pytest.raises(ValueError, match="marker_bits_from_bytes_list.*make_marker_dictionary"):
        boards.CharucoBoard()
    with pytest.raises(NotImplementedError):
        boards.CharucoBoard(dictionary=d, using_marker_corner=True)
    for kw in (dict(square_xy=(2, 5)), dict(square_xy=(17, 5)), dict(first_id=1), dict(dictionary=d[:, :3, :3]),
               dict(marker_size_mm=44.95), dict(dictionary=d * 2)):
        with pytest.raises(ValueError):
            boards.CharucoBoard(**dict(dict(dictionary=d), **kw))
    for sq in ((5, 4), (9, 5), (4, 3), (16, 16)):
        for rank in range(-1, sq[0] * sq[1] // 2 + 1):
            want = ([(x, y) for y in range(sq[1]) for x in range(sq[0]) if x % 2 != y % 2] + [None])[rank] if rank >= 0 else None
            assert ref.marker_square(rank, *sq) == want


def test_build_with_calibration_img_detects_itself():
    board = boards.CharucoBoard.build_with_calibration_img(hw=(330, 440), n=8, ppi=100, seed=4)
    img = board.calibration_img
    assert img.shape == (330, 440) and img.dtype == np.uint8 and board.square_xy == (8, 6) and board.marker_ratio == (3, 4)
    assert board.calibration_img_name == "charuco_square_x8y6_size13.97mm.png" and set(np.unique(img)) == {0, 255}
    exp = ref.find(img, board.square_xy, board.dictionary, board.marker_ratio, board.first_id)
    assert exp["found"][0] and not np.isnan(exp["corners"][0]).any()
    x, y = np.meshgrid(np.arange(1, 8), np.arange(1, 6))
    truth = np.stack([x.ravel() * 55 - 0.5, y.ravel() * 55 - 0.5], 1)  # (the corner between pixels 54 and 55 of a square)
    assert np.abs(exp["corners"][0] - truth).max() <= MAX_OFFSET
    assert (exp["marker_ids"][0] >= 0).sum() >= 12
    inverted = boards.CharucoBoard.build_with_calibration_img(hw=(330, 440), n=8, ppi=100, seed=4, invert_color=True)
    assert np.array_equal(inverted.calibration_img, 255 - img)
