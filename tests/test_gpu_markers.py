"""Stand-alone ArUco markers on the MI355X (-m gpu): every stage of ``imgproc.find_markers`` against the NumPy restatement
tests/markers_ref.py bit for bit -- every value up to the coarse corners is an integer --, the refinement against
``corner_sub_pix``, and ``ArucoGridBoard`` / ``MarkerBoard`` end to end on a rendered recording."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import _native, imgproc  # noqa: E402

import markers_cases as mc  # noqa: E402
import markers_ref as ref  # noqa: E402
import subpix_cases as sc  # noqa: E402

# test_a_camera_from_a_recording_of_a_grid_board: the camera calibrated from the detected, refined corners against the one
# calibrated from the analytic corners of the same markers -- the largest relative difference of fx, fy, cx, cy.  Measured
# once on the MI355X: 2.86e-3 (retval 0.21 px; the refined corners lie up to 0.44 px from the analytic ones on markers of
# 40 .. 60 px); twice that (the yardstick of tests/test_gpu_multiboard.py).
K_MEASURED = 2.86e-3
K_DIFFERENCE = 2 * K_MEASURED


def host(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def same(got, exp, what=""):
    got, exp = np.ascontiguousarray(np.atleast_1d(host(got))), np.ascontiguousarray(np.atleast_1d(exp))
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape, exp.dtype, exp.shape)
    assert np.array_equal(got.view(np.uint8), exp.view(np.uint8)), (what, got, exp)


def check_all(images, dictionary, exp=None, **kw):
    """every stage of the GPU against the restatement; -> (seen, coarse corners, info, exp)"""
    r = {k.replace("max_bit_errors", "max_errors"): v for k, v in kw.items()}
    exp = ref.find(host(images), dictionary, **r) if exp is None else exp
    mask_kw = {k: v for k, v in kw.items() if k in ("block_radius", "offset")}
    mask = imgproc.dark_mask(images, **mask_kw)
    same(mask, exp["mask"] if host(images).ndim == 3 else exp["mask"][0], "mask")
    same(imgproc.label_components(mask), exp["labels"] if host(images).ndim == 3 else exp["labels"][0], "labels")
    seen, corners, info = imgproc.find_markers(images, dictionary, refine_win=None, return_info=True, **kw)
    lead = (lambda a: a) if host(images).ndim == 3 else (lambda a: a[0])
    n = exp["counts"].clip(0, ref.CAPACITY)
    got_cand = host(info["candidates"]).reshape((-1,) + exp["candidates"].shape[1:])
    for f in range(len(n)):  # (the entries beyond a frame's count are not the library's to write)
        same(got_cand[f, :n[f]], exp["candidates"][f, :n[f]], "candidates")
    for key in ("status", "counts", "quads", "id_turn"):
        same(info[key], lead(exp[key]), key)
    same(seen, lead(exp["seen"]), "seen")
    same(corners, lead(exp["corners"]), "corners")
    same(info["coarse"], lead(exp["corners"]), "coarse")
    return seen, corners, info, exp


@pytest.fixture(scope="module")
def mixed():
    images, names = mc.batch()
    exp = ref.find(images, mc.DICT4)
    for a in exp.values():
        a.setflags(write=False)
    return images, names, exp


def test_every_stage_in_one_mixed_batch_equals_the_restatement(mixed):
    images, names, exp = mixed
    seen, corners, info, _ = check_all(images, mc.DICT4, exp)
    worst = 0.0
    for k, name in enumerate(names):
        if name in mc.SCENES:
            worst = max(worst, float(mc.offsets(name, seen[k], corners[k]).max()))
        else:
            assert not seen[k].any() and info["counts"][k] == 0, name
    assert worst <= mc.MAX_COARSE_OFFSET
    # the other sizes and the other dictionary: odd widths, 6 x 6 bits, the hollow ring of a marker over 200 px
    odd, odd_names = mc.batch(mc.ODD_HW)
    assert odd.shape == (2, 93, 157)
    seen, corners, _, _ = check_all(odd, mc.DICT4)
    for k, name in enumerate(odd_names):
        assert mc.offsets(name, seen[k], corners[k]).max() <= mc.MAX_COARSE_OFFSET
    for name in ("six", "big"):
        s = mc.scene(name)
        seen, corners, info, _ = check_all(s["img"], s["dictionary"])
        assert seen.shape == (len(s["dictionary"]),) and corners.shape == (len(s["dictionary"]), 4, 2) and info["counts"].shape == ()
        assert mc.offsets(name, seen, corners).max() <= mc.MAX_COARSE_OFFSET
    # other thresholds, a wrong bit allowed
    check_all(images[:6], mc.DICT4, block_radius=5, offset=12, min_side=20, max_side=60, max_bit_errors=2)
    check_all(images[:3], mc.DICT4, block_radius=32, offset=0)


def test_the_labelling_alone_on_masks_that_stress_the_union_find():
    masks, names = mc.label_masks()
    exp = np.stack([ref.label(m) for m in masks])
    same(imgproc.label_components(masks), exp)
    t = torch.from_numpy(masks).cuda()
    got = imgproc.label_components(t)
    assert got.is_cuda and got.dtype == torch.int32
    same(got, exp)
    same(imgproc.label_components(t.bool()), exp)
    for k in (0, 3, 5):
        same(imgproc.label_components(masks[k]), exp[k], names[k])
    order = [4, 1, 1, 5, 0]
    same(imgproc.label_components(masks[order]), exp[order])
    assert len(np.unique(exp[5][exp[5] >= 0])) == 6  # the blocks that touch at the tiles' corners stay apart
    # sizes about the 32 x 32 tile: one pixel, one tile exactly, one more
    rng = np.random.default_rng(9)
    for h, w in ((1, 1), (1, 70), (70, 1), (32, 32), (33, 33), (31, 65)):
        m = (rng.random((h, w)) < 0.62).astype(np.uint8)
        same(imgproc.label_components(m), ref.label(m), (h, w))


def test_a_frame_alone_and_at_any_place_of_a_batch(mixed):
    images, names, exp = mixed
    for k in (0, names.index("twice"), names.index("noise")):
        alone = imgproc.find_markers(images[k], mc.DICT4, refine_win=None, return_info=True)
        same(alone[0], exp["seen"][k]), same(alone[1], exp["corners"][k])
        for key in ("status", "counts", "quads", "id_turn"):
            same(alone[2][key], exp[key][k], (names[k], key))
    order = np.array([5, 0, 7, 3, 3, 1, 6, 4, 2])
    got = imgproc.find_markers(images[order], mc.DICT4, refine_win=None, return_info=True)
    same(got[0], exp["seen"][order]), same(got[1], exp["corners"][order])
    for key in ("status", "counts", "quads", "id_turn"):
        same(got[2][key], exp[key][order], key)


def test_numpy_cuda_colour_pitches_and_strides_agree(mixed, monkeypatch):
    images, names, exp = mixed
    t = torch.from_numpy(images).cuda()
    seen, corners, info = imgproc.find_markers(t, mc.DICT4, refine_win=None, return_info=True)
    assert seen.is_cuda and seen.dtype == torch.bool and corners.is_cuda and all(v.is_cuda for v in info.values())
    same(seen, exp["seen"]), same(corners, exp["corners"])
    rgb = np.stack([sc.colour(i) for i in images[:3]])
    want = imgproc.find_markers(imgproc.cvt_gray(rgb, "bgr"), mc.DICT4, refine_win=None)
    assert want[0].any(1).all()
    for rgb_in in (rgb, torch.from_numpy(rgb).cuda(), rgb[0]):
        got = imgproc.find_markers(rgb_in, mc.DICT4, refine_win=None)
        for g, w in zip(got, want):
            same(g, w if rgb_in.ndim == 4 else w[0])
    # 157 x 93 out of a wider tensor: odd width, pitch and stride, rows and frames apart
    odd, _ = mc.batch(mc.ODD_HW)
    big = np.random.default_rng(7).integers(0, 256, (3, 101, 171), dtype=np.uint8)
    big[:2, 5:98, 9:166] = odd
    big[2, 5:98, 9:166] = odd[0]
    view = torch.from_numpy(big).cuda()[:, 5:98, 9:166]
    assert not view.is_contiguous() and view.shape == (3, 93, 157)
    e = ref.find(np.ascontiguousarray(big[:, 5:98, 9:166]), mc.DICT4)
    for v, pick in ((view, slice(None)), (view[::2], slice(None, None, 2)), (view[1], 1)):
        got = imgproc.find_markers(v, mc.DICT4, refine_win=None, return_info=True)
        same(got[0], e["seen"][pick]), same(got[1], e["corners"][pick]), same(got[2]["quads"], e["quads"][pick])
        same(imgproc.dark_mask(v), e["mask"][pick])
    # a label plane beyond the budget goes in chunks of frames: the same bits
    monkeypatch.setattr(imgproc, "MARKER_PLANE_BUDGET", 20 * 120 * 160 * 4)
    got = imgproc.find_markers(images, mc.DICT4, refine_win=None, return_info=True)
    same(got[0], exp["seen"]), same(got[1], exp["corners"])
    for key in ("status", "counts", "quads", "id_turn"):
        same(got[2][key], exp[key], key)


def test_more_candidates_than_the_capacity_report_overflow():
    img = mc.overflow_frame()
    seen, corners, info, exp = check_all(img, mc.DICT4, min_side=4)
    assert info["counts"] > imgproc.MARKER_CAPACITY and info["status"] == imgproc.MARKER_OVERFLOW == ref.OVERFLOW
    assert not seen.any() and np.isnan(corners).all() and (info["id_turn"] == -1).all()
    both = np.stack([img, mc.scene("big")["img"]])  # beside a frame that overflows, a frame is what it is alone
    seen, corners, info, _ = check_all(both, mc.DICT4, min_side=4)
    assert list(info["status"]) == [2, 0] and seen[1, 5]


def test_limits_are_refused():
    img = torch.from_numpy(mc.scene("frontal")["img"]).cuda()
    for kw in (dict(block_radius=33), dict(min_side=3), dict(max_side=1025), dict(max_bit_errors=17), dict(offset=300)):
        with pytest.raises(ValueError):
            imgproc.find_markers(img, mc.DICT4, **kw)
    with pytest.raises(ValueError):
        imgproc.find_markers(torch.zeros((2, 16385), dtype=torch.uint8, device="cuda"), mc.DICT4)
    with pytest.raises(ValueError):
        imgproc.label_components(torch.zeros((4, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        imgproc.find_markers(torch.zeros((2, 2), dtype=torch.uint8).cuda(), mc.DICT4)
    one = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = one.data_ptr()
    lib, U = _native.lib(), _native.CAMD_ERR_UNSUPPORTED
    assert lib.camd_dark_mask(p, 64, 48, 64, 64 * 48, 1, 0, 7, p, None) == U
    assert lib.camd_label_components(p, 16385, 4, 1, p, None) == U
    assert lib.camd_marker_candidates(p, 64, 48, 1, 12, 2000, p, p, p, p, None) == U
    assert lib.camd_marker_decode(p, 64, 48, 64, 64 * 48, 1, p, p, p, 12, p, 10, 9, 0, p, p, p, p, p, None) == U
    assert "camd_marker_decode" in _native.last_error()


def test_refined_corners_are_corner_sub_pix_of_the_coarse_ones(mixed):
    images, names, exp = mixed
    seen, corners, info = imgproc.find_markers(images, mc.DICT4, return_info=True)
    same(seen, exp["seen"]), same(info["coarse"], exp["corners"])
    want = imgproc.corner_sub_pix(images, exp["corners"][exp["seen"]].reshape(-1, 2), (3, 3), (-1, -1), (30, 0.01),
                                  counts=4 * exp["seen"].sum(1))
    same(corners[seen], want.reshape(-1, 4, 2))
    assert np.isnan(corners[~seen]).all()
    same(imgproc.find_markers(images, mc.DICT4, refine_win=(5, 5))[1][seen],
         imgproc.corner_sub_pix(images, exp["corners"][exp["seen"]].reshape(-1, 2), (5, 5), counts=4 * exp["seen"].sum(1)).reshape(-1, 4, 2))
    worst = max(float(mc.offsets(name, seen[k], corners[k]).max()) for k, name in enumerate(names) if name in mc.SCENES)
    rec, truth, shown = mc.recording()
    rs, rc = imgproc.find_markers(rec, mc.REC_DICT)
    same(rs, shown)
    worst = max(worst, float(np.abs(rc - truth)[shown].max()))
    print("MEASURED the greatest per-axis distance of a refined corner from the analytic one: %.3f px" % worst)
    assert worst <= mc.MAX_REFINED_OFFSET <= mc.MAX_COARSE_OFFSET
    assert mc.MEASURED_REFINED is not None and mc.MAX_REFINED_OFFSET == max(np.ceil(2 * mc.MEASURED_REFINED) / 2, 0.5)


def pick(K):
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])


def test_a_camera_from_a_recording_of_a_grid_board():
    images, truth, shown = mc.recording()
    board = ca.ArucoGridBoard(mc.GRID, mc.GRID_LENGTH_MM, mc.GRID_SEPARATION_MM, mc.REC_DICT)
    seen, corners = board.find_image_points_batch(images)
    same(seen, shown)
    assert corners.shape == (12, 12, 4, 2) and np.isnan(corners[~seen]).all()
    on_device = board.find_image_points_batch(torch.from_numpy(images).cuda())
    assert all(v.is_cuda for v in on_device)
    same(on_device[0], seen), same(on_device[1], corners)
    frames = board.to_frames(seen, corners)
    assert list(frames) == list(range(12)) and len(frames[2]["ids"]) == 11 and 0 not in frames[2]["image_points"]
    strict = ca.ArucoGridBoard(mc.GRID, mc.GRID_LENGTH_MM, mc.GRID_SEPARATION_MM, mc.REC_DICT)
    strict.occlusion = False
    assert list(strict.to_frames(seen, corners)) == [k for k in range(12) if shown[k].all()]
    d = dict(img=images[4])
    board.find_image_points(d)
    assert d["valid"] and list(d["ids"]) == [i for i in range(12) if shown[4, i]]
    same(d["image_points"][7], corners[4, 7])
    d = dict(img=mc.scene("blank")["img"])
    board.find_image_points(d)
    assert set(d) == {"img", "valid"} and not d["valid"]
    cam = ca.Cam.from_detections(frames, (mc.REC_HW[1], mc.REC_HW[0]), undistorted=True)
    cam.calibrate()
    exact_frames = {k: dict(ids=f["ids"], object_points=f["object_points"],
                            image_points={int(i): truth[k, i].astype(np.float32) for i in f["ids"]}) for k, f in frames.items()}
    exact = ca.Cam.from_detections(exact_frames, (mc.REC_HW[1], mc.REC_HW[0]), undistorted=True)
    exact.calibrate()
    k_diff = float(np.abs(pick(cam.K) / pick(exact.K) - 1).max())
    print("MEASURED K %.3g (against the camera: %.3g; the analytic corners against the camera: %.3g); retval %.3g"
          % (k_diff, float(np.abs(pick(cam.K) / pick(mc.REC_K) - 1).max()), float(np.abs(pick(exact.K) / pick(mc.REC_K) - 1).max()),
             cam.retval))
    assert np.abs(pick(exact.K) / pick(mc.REC_K) - 1).max() < 1e-3  # (the analytic corners, rounded to float32, give the camera)
    assert k_diff <= K_DIFFERENCE


def test_poses_of_a_marker_board_with_an_irregular_layout():
    images, truth, shown = mc.recording()
    grid = mc.grid_points()
    layout = {i: grid[i] for i in (0, 2, 5, 7, 9, 10)}  # any subset of markers, in any places, is a board
    board = ca.MarkerBoard(layout, mc.REC_DICT)
    seen, corners = board.find_image_points_batch(images)
    same(seen, shown[:, board.ids])
    whole = np.flatnonzero(seen.all(1))
    assert len(whole) >= 6
    cam = ca.Cam(mc.REC_K, None, (mc.REC_HW[1], mc.REC_HW[0]))
    obj = np.concatenate([board.object_points[int(i)] for i in board.ids])
    res = cam.perspective_n_point_batch(corners[whole].reshape(len(whole), -1, 2), np.broadcast_to(obj, (len(whole),) + obj.shape).copy())
    assert (host(res["status"]) == 0).all()
    # a pose fitted to corners that lie within e of their true places (per axis) leaves no greater residual than the true
    # pose does, so the board's corners projected by it stay within about 2 e of the true ones
    for k, T in zip(whole, host(res["T"])):
        p = (obj.astype(np.float64) @ T[:3, :3].T + T[:3, 3]) @ mc.REC_K.T
        assert np.abs(p[:, :2] / p[:, 2:] - truth[k][board.ids].reshape(-1, 2)).max() <= 2 * mc.MAX_REFINED_OFFSET, k
