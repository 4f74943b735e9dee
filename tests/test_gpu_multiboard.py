"""Several ChArUco boards per frame on the MI355X (-m gpu): ``imgproc.find_charuco_boards`` against the NumPy restatement
tests/multiboard_ref.py -- corners, marker ids, status and counts bit for bit: every value is an integer --, against
``find_charuco_corners`` with one board, ``boards.MultiBoards`` / ``MultiBoardsCam`` end to end on a rendered recording of
three boards, ``imgproc.sharpness`` against exact integer sums and ``convert_cam_to_nerf_json``."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import boards, geometry, imgproc  # noqa: E402
from calibrating_amd.reconstruction_with_board import convert_cam_to_nerf_json, get_sharpness  # noqa: E402

import charuco_cases as cc  # noqa: E402
import multiboard_cases as mc  # noqa: E402
import multiboard_ref as ref  # noqa: E402
import subpix_cases as sc  # noqa: E402
from chessboard_cases import MAX_OFFSET  # noqa: E402

KEYS = ("seen", "corners", "marker_ids", "status", "counts")
# test_a_camera_from_a_recording_of_three_boards: the camera calibrated from the detected, refined corners against the one
# calibrated from the analytic corners of the same ids -- the largest relative difference of fx, fy, cx, cy, and the largest
# difference of the boards' poses in board 0 (rotation matrix entries; translation in metres).  Measured once on the
# MI355X: K 4.04e-3, R 3.54e-3, t 5.53e-4 m (the refinement's own bias on these renders, tests/subpix_cases.py: up to
# 0.23 px, on squares of 36 px and smaller); twice that.
K_DIFFERENCE, R_DIFFERENCE, T_DIFFERENCE = 8.08e-3, 7.08e-3, 1.106e-3


def host(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def same(got, exp, what=""):
    got, exp = np.ascontiguousarray(np.atleast_1d(host(got))), np.ascontiguousarray(np.atleast_1d(exp))
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape, exp.dtype, exp.shape)
    assert np.array_equal(got.view(np.uint8), exp.view(np.uint8)), (what, got, exp)


def args(first_ids=mc.SET3):
    return (mc.SQUARES, mc.DICTIONARY, tuple(first_ids), mc.RATIO)


def detect(images, first_ids=mc.SET3, **kw):
    return imgproc.find_charuco_boards(images, *args(first_ids), return_info=True, **kw)


@pytest.fixture(scope="module")
def scenes():
    images, names = mc.batch()
    exp = ref.find(images, **mc.kwargs())
    for a in exp.values():
        a.setflags(write=False)
    return images, names, exp


def test_every_scene_in_one_batch_equals_the_restatement(scenes):
    images, names, exp = scenes
    got = detect(images)
    for key, g in zip(KEYS, got):
        same(g, exp[key], key)
    for k, name in enumerate(names):
        mc.check_against_truth(name, got[0][k], got[1][k], MAX_OFFSET)
        assert ((got[3][k] == 0) == mc.scene(name)["present"]).all(), name
    assert {ref.FOUND, ref.FEW, ref.NO_LATTICE} <= set(got[3].ravel().tolist())


def test_four_boards_two_by_two():
    s = mc.scene("grid")
    exp = ref.find(s["img"], **mc.kwargs(mc.FIRST_IDS))
    got = detect(s["img"], mc.FIRST_IDS)
    assert got[0].shape == (4, 12) and got[1].shape == (4, 12, 2) and got[2].shape == (4, 20) and got[3].shape == (4,)
    for key, g in zip(KEYS, got):
        same(g, exp[key][0], key)
    mc.check_against_truth("grid", got[0], got[1], MAX_OFFSET)
    assert got[0].all()


def test_one_board_is_find_charuco_corners_bit_for_bit():
    for setup, images in ((cc.SMALL, cc.mixed_batch()[0]), (cc.WIDE, np.stack([cc.view("wide")["img"], cc.view("wide_cut")["img"]]))):
        for kw in ({}, dict(min_markers=3, max_bit_errors=1)):
            found, corners, marker_ids, status, counts = imgproc.find_charuco_corners(
                images, setup.squares, setup.dictionary, setup.ratio, setup.first_id, return_info=True, **kw)
            got = imgproc.find_charuco_boards(images, setup.squares, setup.dictionary, (setup.first_id,), setup.ratio,
                                              return_info=True, **kw)
            assert got[1].shape == (len(images), 1) + corners.shape[1:]
            same(got[1][:, 0], corners, "corners")
            same(got[2][:, 0], marker_ids, "marker_ids")
            same(got[3][:, 0], status, "status")
            same(got[4], counts, "counts")
            same(got[0][:, 0], ~np.isnan(corners[..., 0]), "seen")
            assert found.any() and (setup is cc.WIDE or not found.all())


def test_a_frame_alone_and_at_any_place_of_a_batch(scenes):
    images, names, exp = scenes
    for k in (0, names.index("foreign"), names.index("few")):
        alone = detect(images[k])
        assert alone[0].shape == (3, 12) and alone[4].shape == ()
        for key, a in zip(KEYS, alone):
            same(a, exp[key][k], (names[k], key))
    order = np.array([5, 0, 7, 3, 3, 1, 6, 4, 2])  # nine frames: two workgroups of four and one more
    for key, g in zip(KEYS, detect(images[order])):
        same(g, exp[key][order], key)


def test_numpy_cuda_colour_and_inverted_inputs_agree(scenes):
    images, names, exp = scenes
    t = torch.from_numpy(images).cuda()
    got = detect(t)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got) and got[0].dtype == torch.bool
    for key, g in zip(KEYS, got):
        same(g, exp[key], key)
    one = imgproc.find_charuco_boards(t[0], *args())
    assert len(one) == 2 and one[0].shape == (3, 12)
    same(one[1], exp["corners"][0])
    # colour: the detector sees cvt_gray's image
    rgb = np.stack([sc.colour(i) for i in images[:2]])
    want = detect(imgproc.cvt_gray(rgb, "bgr"))
    assert (want[3] == 0).all()
    for rgb_in in (rgb, torch.from_numpy(rgb).cuda(), rgb[0]):
        for key, g, w in zip(KEYS, detect(rgb_in), want):
            same(g, w if rgb_in.ndim == 4 else w[0], key)
    # boards printed inverted: MultiBoards inverts the image back
    inverted = ca.MultiBoards([ca.CharucoBoard(mc.SQUARES, 30.0, 20.0, mc.DICTIONARY, k, invert_color=True) for k in mc.SET3])
    plain = ca.MultiBoards([ca.CharucoBoard(mc.SQUARES, 30.0, 20.0, mc.DICTIONARY, k) for k in mc.SET3])
    a, b = inverted.find_image_points_batch(255 - images[:3], return_info=True), plain.find_image_points_batch(t[:3], return_info=True)
    for k in (0, 2, 3, 4):
        same(a[k], host(b[k]))
    assert np.abs(a[1][a[0]] - host(b[1])[a[0]]).max() < 1e-3  # (the refinement reads the picture as it came, inverted)
    same(a[2], exp["marker_ids"][:3])
    assert not detect(255 - images[:2])[0].any()


def test_odd_sizes_pitches_and_strides(scenes):
    # 631 x 471 out of 645 x 485: width, pitch and stride no multiples of 4, 8 or 16; a view whose rows and frames lie apart
    rng = np.random.default_rng(7)
    images, names, _ = scenes
    big = rng.integers(0, 256, (3, 485, 645), dtype=np.uint8)
    for k, name in enumerate(("row", "cut_covered", "margin")):
        big[k, 2:482, 3:643] = images[names.index(name)]
    view = torch.from_numpy(big).cuda()[:, 5:476, 8:639]
    assert not view.is_contiguous() and view.shape == (3, 471, 631)
    tight = np.ascontiguousarray(big[:, 5:476, 8:639])
    exp = ref.find(tight[:2], relative=6, nms_radius=2, **mc.kwargs())
    assert (exp["status"][0] == 0).all()
    want = detect(tight, relative=6, nms_radius=2)
    for key, g in zip(KEYS, want):
        same(g[:2], exp[key], key)
    for key, g, w in zip(KEYS, detect(view, relative=6, nms_radius=2), want):
        same(g, w, key)
    for key, g, w in zip(KEYS, detect(view[::2], relative=6, nms_radius=2), want):
        same(g, w[::2], key)


def test_limits_are_refused():
    img = mc.scene("paper")["img"]
    base = dict(squares_xy=mc.SQUARES, dictionary=mc.DICTIONARY, marker_ratio=mc.RATIO)
    for first_ids in ((), tuple(range(0, 54, 6)), (1, 5), (1, 10), (49,), (-1,)):  # B = 0, B = 9, overlaps, past the dictionary
        with pytest.raises(ValueError):
            imgproc.find_charuco_boards(img, first_ids=first_ids, **base)
    # the library's own checks: the set arrives by value
    from calibrating_amd import _native
    import ctypes
    one = torch.zeros(8, dtype=torch.int64, device="cuda")
    for n, ids in ((0, ()), (9, ()), (2, (1, 5)), (1, (49,)), (1, (-1,))):
        s = _native.CharucoBoards(n, (ctypes.c_int * 8)(*ids))
        rc = _native.lib().camd_charuco_detect_multi(one.data_ptr(), one.data_ptr(), one.data_ptr(), 64, 48, 64, 64 * 48, 1, 5, 4, 2, 3,
                                                     one.data_ptr(), 58, 4, ctypes.byref(s), 2, 0, one.data_ptr(), one.data_ptr(),
                                                     one.data_ptr(), None)
        assert rc == _native.CAMD_ERR_UNSUPPORTED and "camd_charuco_detect_multi" in _native.last_error()
    rc = _native.lib().camd_charuco_detect_multi(one.data_ptr(), one.data_ptr(), one.data_ptr(), 64, 48, 64, 64 * 48, 1, 5, 4, 2, 3,
                                                 one.data_ptr(), 58, 4, None, 2, 0, one.data_ptr(), one.data_ptr(), one.data_ptr(), None)
    assert rc == _native.CAMD_ERR_BAD_ARG


# ---- the classes -----------------------------------------------------------------------------------------------------------
def make_boards():
    return {"b%d" % k: ca.CharucoBoard(mc.SQUARES, 30.0, 20.0, mc.DICTIONARY, first) for k, first in enumerate(mc.SET3)}


def test_multi_boards_as_one_target():
    images, truth = mc.recording()
    cam = ca.Cam(mc.FRAME.K, None, (mc.HW[1], mc.HW[0]))
    bs = make_boards()
    multi = ca.MultiBoards(bs, [images[0]], cam)
    assert multi.first_ids == list(mc.SET3) and len(multi.Ts) == 3 and np.allclose(multi.Ts[0], np.eye(4), atol=1e-6)
    assert set(multi.object_points) == {(b, i) for b in range(3) for i in range(12)}
    centre = np.concatenate(list(multi.object_points.values())).mean(0)
    assert np.abs(centre).max() < 1e-6
    seen, corners = multi.find_image_points_batch(images)
    coarse = imgproc.find_charuco_boards(images, *args())[1]
    same(seen, ~np.isnan(coarse[..., 0]))
    same(corners[seen], imgproc.corner_sub_pix(images, coarse[seen], boards.SUBPIX_WIN, boards.SUBPIX_ZERO_ZONE,
                                               boards.SUBPIX_CRITERIA, counts=seen.sum((1, 2))))
    assert np.abs(corners[seen] - truth[seen]).max() <= 0.5
    on_device = multi.find_image_points_batch(torch.from_numpy(images).cuda())
    assert all(v.is_cuda for v in on_device)
    same(on_device[0], seen)
    same(on_device[1], corners)
    # one record at a time, as the reference's loop
    k = 3
    d = dict(img=images[k])
    multi.find_image_points(d)
    shown = [b for b in range(3) if seen[k, b].sum() >= 11]
    assert shown and set(d) == {"img", "image_points", "object_points"}
    assert sorted(d["image_points"]) == [(b, int(i)) for b in shown for i in np.flatnonzero(seen[k, b])]
    for (b, i), p in d["image_points"].items():
        same(p, corners[k, b, i][None])
        assert d["object_points"][(b, i)] is multi.object_points[(b, i)]
    d = dict(img=mc.scene("plain")["img"])
    multi.find_image_points(d)
    assert set(d) == {"img"}
    # to_frames and back
    frames = multi.to_frames(seen, corners, keys=["f%d" % i for i in range(len(images))])
    assert list(frames) == ["f%d" % i for i in range(len(images)) if (seen[i].sum(1) >= 11).any()] and len(frames) >= 8
    for key, fr in frames.items():
        i = int(key[1:])
        assert fr["ids"] == sorted(fr["image_points"]) == sorted(fr["object_points"])
        back = np.full((3, 12, 2), np.nan, np.float32)
        for (b, j), p in fr["image_points"].items():
            back[b, j] = p[0]
        full = seen[i].sum(1) >= 11
        same(back[full], corners[i][full])
        assert np.isnan(back[~full]).all()
    # the whole target's pose in a view that shows all boards: the camera of that view
    rec = cam.get_calibration_board_T(images[1], multi)
    print("the three boards as one target, placed from view 0, seen in view 1: reprojection error %.3g px" % rec["reprojection_error"])
    assert rec["reprojection_error"] < 1.0  # (corners within 0.5 px of their places in either view)


def pick(K):
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])


def test_a_camera_from_a_recording_of_three_boards(tmp_path):
    images, truth = mc.recording()
    bs = make_boards()
    names = list(bs)
    keys = ["v%d" % k for k in range(len(images))]
    with pytest.raises(ValueError):
        ca.MultiBoardsCam(["v0.png"], bs)
    cam = ca.MultiBoardsCam(dict(zip(keys, images)), bs, undistorted=True)
    assert cam.boards is bs and cam.xy == (640, 480)
    seen, corners = ca.MultiBoards(bs).find_image_points_batch(images)
    want_keys = {"%s~%s" % (keys[k], names[b]) for k in range(len(images)) for b in range(3) if seen[k, b].sum() >= 11}
    print("corners seen per view and board:", seen.sum(2).tolist())
    assert set(cam) == want_keys and len(want_keys) >= 2 * len(images)
    assert not seen.all((1, 2)).all()  # (no view has to show every board whole)
    for key, d in cam.items():
        k, b = keys.index(key.split("~")[0]), names.index(key.split("~")[1])
        assert d["board"] is bs[names[b]] and d["img"] is not None and "T" in d
        same(np.concatenate([d["image_points"][i] for i in d["ids"]]), corners[k, b][seen[k, b]])
    # the plumbing: the boards in board 0 and the cameras in the world, recomputed from the cam's own poses
    T_of = lambda k, b: cam["%s~%s" % (keys[k], names[b])]["T"]  # noqa: E731
    has = lambda k, b: "%s~%s" % (keys[k], names[b]) in cam      # noqa: E731
    in_board0 = {names[b]: geometry.mean_Ts([np.linalg.inv(T_of(k, 0)) @ T_of(k, b) for k in range(len(images)) if has(k, 0) and has(k, b)])
                 for b in range(3)}
    got = cam.get_board_name_to_T_world()
    assert list(got) == names
    for n in names:
        assert np.abs(got[n] - in_board0[n]).max() <= 1e-12
    to_world = np.linalg.inv(geometry.mean_Ts(list(in_board0.values())))
    world = cam.get_board_name_to_T_world(True)
    for n in names:
        assert np.abs(world[n] - to_world @ in_board0[n]).max() <= 1e-12
    out = cam.convert_to_nerf_json(coordinate_type="opencv", sharpness=False)
    assert set(f["file_path"] for f in out["frames"]) == {k.split("~")[0] for k in cam}
    for f in out["frames"]:
        k = keys.index(f["file_path"])
        want = geometry.mean_Ts([to_world @ in_board0[names[b]] @ np.linalg.inv(T_of(k, b)) for b in range(3) if has(k, b)])
        assert np.abs(f["transform_matrix"] - want).max() <= 1e-12
    assert not any("T_cam_in_world" in d for d in cam.values())  # (the cam's own records are left as they were)
    path = cam.convert_to_nerf_json(str(tmp_path / "transforms.json"), target_scale=2.0)
    written = json.load(open(path))
    assert len(written["frames"]) == len(out["frames"]) and all("sharpness" in f for f in written["frames"])
    assert abs(np.mean([np.linalg.norm(np.array(f["transform_matrix"])[:3, 3]) for f in written["frames"]]) - 2.0) < 1e-12
    # the accuracy: the same pipeline fed the analytic corners of the same ids
    exact = ca.MultiBoardsCam()
    exact.xy, exact.name, exact.undistorted, exact.calibrate_flags = cam.xy, None, True, 0
    for key, d in cam.items():
        k, b = keys.index(key.split("~")[0]), names.index(key.split("~")[1])
        exact[key] = dict(ids=d["ids"], object_points=d["object_points"],
                          image_points={int(i): truth[k, b, i][None].astype(np.float32) for i in d["ids"]})
    exact.calibrate()
    exact.boards = bs
    k_diff = float(np.abs(pick(cam.K) / pick(exact.K) - 1).max())
    a, b = cam.get_board_name_to_T_world(), exact.get_board_name_to_T_world()
    r_diff = max(float(np.abs(a[n][:3, :3] - b[n][:3, :3]).max()) for n in names)
    t_diff = max(float(np.abs(a[n][:3, 3] - b[n][:3, 3]).max()) for n in names)
    print("MEASURED K %.3g (against the camera: %.3g), R %.3g, t %.3g m; retval %.3g"
          % (k_diff, float(np.abs(pick(cam.K) / pick(mc.FRAME.K) - 1).max()), r_diff, t_diff, cam.retval))
    assert np.abs(pick(exact.K) / pick(mc.FRAME.K) - 1).max() < 1e-3  # (the analytic corners, rounded to float32, give the camera)
    for n, (rvec, t) in zip(names, mc.WORLD_BOARDS):  # ... and the boards where the world has them
        T0 = geometry.R_t_to_T(sc.rodrigues(mc.WORLD_BOARDS[0][0]), mc.WORLD_BOARDS[0][1])
        assert np.abs(b[n] - np.linalg.inv(T0) @ geometry.R_t_to_T(sc.rodrigues(rvec), t)).max() < 1e-3
    assert k_diff <= K_DIFFERENCE and r_diff <= R_DIFFERENCE and t_diff <= T_DIFFERENCE


# ---- sharpness ---------------------------------------------------------------------------------------------------------------
def test_laplacian_sums_are_exact():
    rng = np.random.default_rng(3)
    checker = ((np.add.outer(np.arange(64), np.arange(48)) % 2) * 255).astype(np.uint8)
    cases = [rng.integers(0, 256, (2, 2), dtype=np.uint8), rng.integers(0, 256, (3, 5), dtype=np.uint8),
             np.full((33, 20), 77, np.uint8), checker]
    for g in cases:
        want = ref.laplacian_sums(g)
        for img in (g, torch.from_numpy(g).cuda()):
            got = imgproc.laplacian_sums(img)
            assert got.dtype in (np.int64, torch.int64) and tuple(host(got).tolist()) == want, g.shape
        var = imgproc.sharpness(g)
        exact = ref.laplacian(g).var()
        assert isinstance(var, float) and abs(var - exact) <= 1e-12 * exact
    assert imgproc.sharpness(cases[2]) == 0.0 and ref.laplacian_sums(cases[2]) == (0, 0)
    assert ref.laplacian_sums(checker)[1] > 0.9 * checker.size * 2040 ** 2 / 4  # (the largest magnitudes: |L| = 1020 inside)
    # 257 x 131 with an odd pitch, out of a wider tensor; a batch of different frames and one of them alone
    big = torch.from_numpy(rng.integers(0, 256, (3, 140, 263), dtype=np.uint8)).cuda()
    view = big[:, 4:135, 3:260]
    assert view.shape == (3, 131, 257) and not view.is_contiguous()
    want = np.array([ref.laplacian_sums(g) for g in host(view)], np.int64)
    same(imgproc.laplacian_sums(view), want)
    same(imgproc.laplacian_sums(view[1]), want[1])
    same(imgproc.laplacian_sums(host(view)), want)
    var = imgproc.sharpness(view)
    exact = np.array([ref.laplacian(g).var() for g in host(view)])
    assert var.dtype == np.float64 and var.shape == (3,) and (np.abs(var - exact) <= 1e-12 * exact).all()
    # colour goes through cvt_gray
    rgb = rng.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    same(imgproc.laplacian_sums(rgb), imgproc.laplacian_sums(imgproc.cvt_gray(rgb, "bgr")))
    assert get_sharpness(rgb[0]) == imgproc.sharpness(imgproc.cvt_gray(rgb[0], "bgr"))


def test_convert_cam_to_nerf_json(tmp_path):
    rng = np.random.default_rng(5)
    cam = ca.Cam([[500.0, 0, 310.0], [0, 510.0, 250.0], [0, 0, 1]], [[0.1, -0.2, 0.001, 0.002, 0.05]], (640, 480))
    img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    poses = [geometry.R_t_to_T(sc.rodrigues(rng.normal(0, 0.3, 3)), rng.normal(0, 1, 3) + (0, 0, 3)) for _ in range(3)]
    cam["a"] = dict(T=poses[0], path="/data/a.png", img=img)
    cam["b"] = dict(T=poses[1], path="/data/b.png")
    cam["c"] = dict(T=poses[2], T_cam_in_world=poses[0], path="/data/c.png", img=torch.from_numpy(img[..., 0].copy()).cuda())
    cam["d"] = dict(path="/data/d.png", img=img)  # no pose: no frame
    out = convert_cam_to_nerf_json(cam)
    assert list(out) == ["fl_x", "fl_y", "cx", "cy", "w", "h", "camera_angle_x", "camera_angle_y", "coordinate_type", "k1", "k2", "p1",
                         "p2", "frames"]
    assert (out["fl_x"], out["fl_y"], out["cx"], out["cy"], out["w"], out["h"]) == (500.0, 510.0, 310.0, 250.0, 640, 480)
    assert abs(out["camera_angle_x"] - 2 * np.arctan(320 / 500)) < 1e-12 and abs(out["camera_angle_y"] - 2 * np.arctan(240 / 510)) < 1e-12
    assert (out["k1"], out["k2"], out["p1"], out["p2"]) == (0.1, -0.2, 0.001, 0.002) and out["coordinate_type"] == "nerf"
    assert [f["file_path"] for f in out["frames"]] == ["/data/a.png", "/data/b.png", "/data/c.png"]
    assert ["sharpness" in f for f in out["frames"]] == [True, False, True]
    assert out["frames"][0]["sharpness"] == imgproc.sharpness(img) and out["frames"][2]["sharpness"] == imgproc.sharpness(img[..., 0])
    flip = np.diag([1.0, -1, -1, 1])
    up = geometry.R_t_to_T([np.pi, 0, 0])
    in_world = [np.linalg.inv(poses[0]), np.linalg.inv(poses[1]), poses[0]]
    for f, T in zip(out["frames"], in_world):
        assert np.array_equal(f["transform_matrix"], up @ (T @ flip))
    for kw, make in ((dict(coordinate_type="opencv"), lambda T: T), (dict(coordinate_type="opencv", rotate_z_as_up=False), lambda T: T),
                     (dict(rotate_z_as_up=False), lambda T: T @ flip)):
        got = convert_cam_to_nerf_json(cam, sharpness=False, basename=True, **kw)
        assert [f["file_path"] for f in got["frames"]] == ["a.png", "b.png", "c.png"] and not any("sharpness" in f for f in got["frames"])
        for f, T in zip(got["frames"], in_world):
            assert np.array_equal(f["transform_matrix"], make(T))
    with pytest.raises(AssertionError):
        convert_cam_to_nerf_json(cam, coordinate_type="blender")
    scaled = convert_cam_to_nerf_json(cam, target_scale=2.5, sharpness=False)
    norms = [np.linalg.norm(f["transform_matrix"][:3, 3]) for f in scaled["frames"]]
    plain = [np.linalg.norm(f["transform_matrix"][:3, 3]) for f in out["frames"]]
    assert abs(np.mean(norms) - 2.5) < 1e-12 and np.allclose(np.array(norms) / plain, 2.5 / np.mean(plain), rtol=1e-12)
    for f, g in zip(scaled["frames"], out["frames"]):
        assert np.array_equal(f["transform_matrix"][:3, :3], g["transform_matrix"][:3, :3])
    path = convert_cam_to_nerf_json(cam, str(tmp_path / "t.json"))
    written = json.load(open(path))
    assert isinstance(written["frames"][0]["transform_matrix"], list) and written["fl_x"] == 500.0
    assert np.array_equal(np.array(written["frames"][1]["transform_matrix"]), out["frames"][1]["transform_matrix"])
