"""The marker detector without a GPU: the NumPy restatement tests/markers_ref.py against rendered markers with analytic
corners, the argument refusals of ``imgproc.find_markers`` and of the library before the device is touched, and the host
side of ``boards.MarkerBoard`` / ``boards.ArucoGridBoard``."""
import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import _native, boards, imgproc

import markers_cases as mc
import markers_ref as ref


def test_every_rendered_marker_is_found_with_its_id_and_turn():
    worst = 0.0
    for name in mc.SCENES:
        s = mc.scene(name)
        out = ref.find(s["img"], s["dictionary"])
        off = mc.offsets(name, out["seen"][0], out["corners"][0])  # (the corners in the marker's own order: id AND turn)
        worst = max(worst, float(off.max()))
        assert out["status"][0] == 0 and out["counts"][0] >= len(s["truth"])
    images, truth, shown = mc.recording()
    out = ref.find(images, mc.REC_DICT)
    assert np.array_equal(out["seen"], shown) and not shown.all() and shown[0].all()
    worst = max(worst, float(np.abs(out["corners"] - truth)[shown].max()))
    print("MEASURED the greatest per-axis distance of a coarse corner from the analytic one: %.3f px" % worst)
    assert worst <= mc.MAX_COARSE_OFFSET <= 2.0 and mc.MAX_COARSE_OFFSET == np.ceil(2 * mc.MEASURED_COARSE) / 2
    assert abs(worst - mc.MEASURED_COARSE) < 0.005


def test_the_scenes_cover_what_they_claim():
    for name in mc.NO_MARKER:
        s = mc.scene(name)
        out = ref.find(s["img"], s["dictionary"])
        assert not out["seen"].any() and out["counts"][0] == 0, name  # cut by the edge, below min_side, nothing: no candidate
    assert ref.dark_mask(mc.scene("cut")["img"])[:, -1].any()         # (the cut marker's outline reaches the last column)
    two, twice = ref.find(mc.scene("two")["img"], mc.DICT4), ref.find(mc.scene("twice")["img"], mc.DICT4)
    assert two["seen"].sum() == 2 and twice["seen"].sum() == 1 and (twice["id_turn"][0] >= 0).sum() == 2
    first = twice["quads"][0, 0]  # of two copies with no wrong bit the lower candidate stands
    assert np.array_equal(np.sort(twice["corners"][0, 2], 0), np.sort(first.astype(np.float32), 0))
    assert {int(v) & 3 for name in ("frontal", "turn90", "turn180", "tilted", "two")
            for v in ref.find(mc.scene(name)["img"], mc.DICT4)["id_turn"][0] if v >= 0} == {0, 1, 2, 3}
    big = ref.find(mc.scene("big")["img"], mc.DICT4)
    x0, y0, x1, y1 = big["candidates"][0, 0, 1:5]
    assert x1 - x0 > 200 and y1 - y0 > 200
    black = mc.scene("big")["img"][y0:y1, x0:x1] < 60
    assert (black & (big["mask"][0, y0:y1, x0:x1] == 0)).sum() > 1000  # a hollow ring: black pixels that are not dark
    c = ref.find(mc.scene("tiles")["img"], mc.DICT4)["candidates"][0, 0]
    assert c[1] // 32 < c[3] // 32 - 1 and c[2] // 32 < c[4] // 32 - 1  # the outline crosses labelling tiles both ways
    over = ref.find(mc.overflow_frame(), mc.DICT4, min_side=4)
    assert over["counts"][0] > ref.CAPACITY and over["status"][0] == ref.OVERFLOW and not over["seen"].any()
    assert (over["id_turn"] == -1).all() and (over["candidates"][0, -1] >= 0).all()
    noisy = ref.find(mc.scene("noisy")["img"], mc.DICT4, max_errors=2)
    assert noisy["seen"][0, 7] and noisy["seen"].sum() == 1


def test_the_labels_of_the_stress_masks():
    masks, names = mc.label_masks()
    counts = {}
    for m, name in zip(masks, names):
        L = ref.label(m)
        assert L.dtype == np.int32 and np.array_equal(L >= 0, m != 0)
        roots = np.unique(L[L >= 0])
        counts[name] = len(roots)
        flat = L.ravel()
        assert np.array_equal(flat[roots], roots) and (flat[flat >= 0] <= np.flatnonzero(flat >= 0)).all()  # the least index
        for dy, dx in ((0, 1), (1, 0)):  # neighbours share a label
            a, b = L[:L.shape[0] - dy, :L.shape[1] - dx], L[dy:, dx:]
            both = (a >= 0) & (b >= 0)
            assert np.array_equal(a[both], b[both])
    assert counts == dict(serpentine=1, comb=1, spiral=1, all_dark=1, checker=3500, touch=6)


def test_the_mask_is_the_clipped_window_rule():
    rng = np.random.default_rng(2)
    g = rng.integers(0, 256, (23, 31), dtype=np.uint8)
    for r, offset in ((1, 0), (3, 7), (8, -5), (32, 7)):
        want = np.zeros(g.shape, np.uint8)
        for y in range(g.shape[0]):
            for x in range(g.shape[1]):
                win = g[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].astype(np.int64)
                want[y, x] = (int(g[y, x]) + offset) * win.size < win.sum()
        assert np.array_equal(ref.dark_mask(g, r, offset), want)


def test_refusals_come_before_the_device():
    img = mc.scene("frontal")["img"]
    for kw in (dict(block_radius=0), dict(block_radius=33), dict(offset=256), dict(min_side=3), dict(min_side=20, max_side=19),
               dict(max_side=1025), dict(max_bit_errors=-1), dict(max_bit_errors=17), dict(block_radius=2.5), dict(refine_win=(0, 3)),
               dict(refine_win=3)):
        with pytest.raises(ValueError):
            imgproc.find_markers(img, mc.DICT4, **kw)
        if "refine_win" not in kw:
            with pytest.raises(ValueError):
                ref.check_arguments(mc.DICT4, **{dict(max_bit_errors="max_errors").get(k, k): v for k, v in kw.items()})
    for bad_dictionary in (np.zeros((3, 3, 3), np.uint8), np.zeros((2, 4, 5), np.uint8), np.full((2, 4, 4), 2, np.uint8),
                           np.zeros((1025, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            imgproc.find_markers(img, bad_dictionary)
    for bad in (img.astype(np.float32), np.zeros((0, 5), np.uint8), np.zeros((2, 2, 2, 2, 2), np.uint8), np.zeros((2, 16385), np.uint8)):
        with pytest.raises(ValueError):
            imgproc.find_markers(bad, mc.DICT4)
        with pytest.raises(ValueError):
            imgproc.dark_mask(bad)
    with pytest.raises(TypeError):
        imgproc.find_markers(img.tolist(), mc.DICT4)
    for bad in (np.zeros((4, 4), np.int32), np.zeros((2, 2, 2, 2), np.uint8), np.zeros((0, 4), np.uint8), np.zeros((16385, 2), bool)):
        with pytest.raises(ValueError):
            imgproc.label_components(bad)
    with pytest.raises(ValueError):
        imgproc.dark_mask(img, block_radius=40)
    # the library's own checks: limits first, and nothing is dereferenced
    lib, U, p = _native.lib(), _native.CAMD_ERR_UNSUPPORTED, 4096
    assert lib.camd_dark_mask(p, 64, 48, 64, 64 * 48, 1, 33, 7, p, None) == U and "camd_dark_mask" in _native.last_error()
    assert lib.camd_dark_mask(p, 16385, 48, 16385, 16385 * 48, 1, 8, 7, p, None) == U
    assert lib.camd_label_components(p, 64, 16385, 1, p, None) == U
    assert lib.camd_marker_candidates(p, 64, 48, 1, 12, 1025, p, p, p, p, None) == U
    assert lib.camd_marker_candidates(p, 64, 48, 1, 3, 512, p, p, p, p, None) == U
    for s, n_ids, errors in ((9, 10, 0), (3, 10, 0), (4, 1025, 0), (4, 0, 0), (4, 10, 17)):
        assert lib.camd_marker_decode(p, 64, 48, 64, 64 * 48, 1, p, p, p, 12, p, n_ids, s, errors, p, p, p, p, p, None) == U
    assert lib.camd_marker_decode(None, 64, 48, 64, 64 * 48, 1, p, p, p, 12, p, 10, 4, 0, p, p, p, p, p, None) == _native.CAMD_ERR_BAD_ARG
    assert lib.camd_marker_candidates_workspace_bytes(64, 48, 2) >= 2 * 48 * 64 * 16 and lib.camd_marker_candidates_workspace_bytes(0, 1, 1) == 0


def test_the_grid_board_and_its_sheet():
    assert ca.ArucoGridBoard is boards.ArucoGridBoard and ca.MarkerBoard is boards.MarkerBoard
    assert {"ArucoGridBoard", "MarkerBoard"} <= set(ca.__all__)
    board = ca.ArucoGridBoard(mc.GRID, mc.GRID_LENGTH_MM, mc.GRID_SEPARATION_MM, mc.REC_DICT)
    want = mc.grid_points()
    assert sorted(board.object_points) == sorted(want) == list(range(12)) and list(board.ids) == list(range(12))
    for i, p in board.object_points.items():
        assert p.dtype == np.float32 and p.shape == (4, 3) and np.abs(p - want[i]).max() < 1e-7
    assert np.allclose(board.object_points[5][1] - board.object_points[5][0], (0.03, 0, 0))       # top-left -> top-right: x
    assert np.allclose(board.object_points[5][3] - board.object_points[5][0], (0, 0.03, 0))       # top-left -> bottom-left: y down
    assert np.allclose(board.object_points[4][0] - board.object_points[0][0], (0, 0.036, 0))      # the next row of the grid
    shifted = ca.ArucoGridBoard((2, 2), 50.0, 10.0, mc.REC_DICT, first_id=8)
    assert sorted(shifted.object_points) == [8, 9, 10, 11]
    for bad in (dict(grid_size=(4, 4)), dict(first_id=1), dict(dictionary=None), dict(grid_size=(0, 3))):
        with pytest.raises(ValueError):
            ca.ArucoGridBoard(**dict(dict(grid_size=mc.GRID, dictionary=mc.REC_DICT), **bad))
    with pytest.raises(ValueError):
        ca.MarkerBoard({0: np.zeros((4, 2))}, mc.REC_DICT)
    with pytest.raises(ValueError):
        ca.MarkerBoard({12: np.zeros((4, 3))}, mc.REC_DICT)
    # the sheet: the reference's bit arithmetic -- marker 6 units, separation 1, margin 1
    sheet = ca.ArucoGridBoard.build_with_calibration_img(hw=(600, 860), n=4, ppi=100)
    unit = 860 / 29
    assert sheet.grid_size == ((int(860 / unit + 1e-5) - 1) // 7, (int(600 / unit + 1e-5) - 1) // 7) == (4, 2)
    mm = round(unit / 100 * 25.4, 2)
    assert sheet.marker_length_mm == mm * 6 and sheet.marker_separation_mm == mm and sheet.dictionary.shape == (8, 4, 4)
    img, q, m = sheet.calibration_img, int(unit), int(round(unit))
    assert img.shape == (600, 860) and img.dtype == np.uint8 and set(np.unique(img)) == {0, 255}
    assert (img[:m] == 255).all() and (img[:, :m] == 255).all()
    for j in range(2):
        for i in range(4):
            cell = img[m + 7 * q * j:m + 7 * q * j + 6 * q, m + 7 * q * i:m + 7 * q * i + 6 * q]
            assert (cell[0] == 0).all() and (cell[-1] == 0).all() and (cell[:, 0] == 0).all() and (cell[:, -1] == 0).all()
            bits = cell[q + q // 2::q, q + q // 2::q][:4, :4] // 255  # 6 units over 4 + 2 cells: a cell is a unit
            assert np.array_equal(bits, sheet.dictionary[j * 4 + i])
            assert (img[m + 7 * q * j:m + 7 * q * j + 6 * q, m + 7 * q * i + 6 * q:m + 7 * q * i + 7 * q] == 255).all()  # separation
    # what the detector's restatement sees on the printed sheet is the board
    out = ref.find(img, sheet.dictionary)
    assert out["seen"].all()
    for i in range(8):
        x, y = m + 7 * q * (i % 4), m + 7 * q * (i // 4)
        assert np.abs(out["corners"][0, i] - [[x, y], [x + 6 * q - 1, y], [x + 6 * q - 1, y + 6 * q - 1], [x, y + 6 * q - 1]]).max() <= 1
    assert "aruco_grid_x4y2" in sheet.calibration_img_name and sheet.calibration_img_info["bit_px"] == q


def test_to_frames_rows():
    pts = {3: np.arange(12.0).reshape(4, 3), 1: np.ones((4, 3)), 6: np.zeros((4, 3))}
    board = ca.MarkerBoard(pts, mc.REC_DICT)
    strict = ca.MarkerBoard(pts, mc.REC_DICT, occlusion=False)
    assert list(board.ids) == [1, 3, 6] and board.object_points[3].dtype == np.float32
    seen = np.array([[True, True, True], [True, False, True], [False, False, False]])
    corners = np.arange(3 * 3 * 4 * 2, dtype=np.float32).reshape(3, 3, 4, 2)
    corners[~seen] = np.nan
    frames = board.to_frames(seen, corners, keys=["a", "b", "c"])
    assert list(frames) == ["a", "b"] and list(strict.to_frames(seen, corners)) == [0]
    assert list(frames["b"]["ids"]) == [1, 6] and sorted(frames["b"]["image_points"]) == [1, 6]
    assert np.array_equal(frames["b"]["image_points"][6], corners[1, 2]) and frames["b"]["object_points"][6] is board.object_points[6]
    from calibrating_amd import geometry
    rows = geometry.join_points(frames["a"]["image_points"])
    assert rows.shape == (12, 2) and np.array_equal(rows, corners[0].reshape(12, 2))  # id order, four rows per marker
    assert np.array_equal(geometry.join_points(frames["a"]["object_points"])[4:8], pts[3].astype(np.float32))
    with pytest.raises(ValueError):
        board.to_frames(seen, corners, keys=["a"])
    cam = ca.Cam.from_detections(frames, (320, 240))
    assert set(cam) == {"a", "b"}
