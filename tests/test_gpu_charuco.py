"""The ChArUco detector on the MI355X (-m gpu): ``imgproc.find_charuco_corners`` and ``boards.CharucoBoard`` against the
NumPy restatement tests/charuco_ref.py -- corners, marker ids, status and counts bit for bit: every value is an integer --
and, end to end, a camera and a rig calibrated from recordings in which no frame shows the whole board."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import boards, imgproc  # noqa: E402

import charuco_cases as cc  # noqa: E402
import charuco_ref as ref  # noqa: E402
import subpix_cases as sc  # noqa: E402
import subpix_ref  # noqa: E402
from chessboard_cases import MAX_OFFSET  # noqa: E402

KEYS = ("found", "corners", "marker_ids", "status", "counts")
# test_a_camera_from_a_recording_of_partial_views: the largest relative difference of fx, fy, cx, cy between the camera
# calibrated from the detected, refined corners and the one calibrated from the analytic corners of the same ids.
# Measured once on the MI355X: 2.26e-3 (the refinement's own bias on these renders, tests/subpix_cases.py: up to 0.23 px);
# twice that.
K_DIFFERENCE = 4.6e-3


def host(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def same(got, exp, what=""):
    got, exp = np.ascontiguousarray(np.atleast_1d(host(got))), np.ascontiguousarray(np.atleast_1d(exp))
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape, exp.dtype, exp.shape)
    assert np.array_equal(got.view(np.uint8), exp.view(np.uint8)), (what, got, exp)


def args(setup):
    return (setup.squares, setup.dictionary, setup.ratio, setup.first_id)


def check(images, setup, exp=None, **kw):
    exp = ref.find(images, **dict(setup.kwargs(), **kw)) if exp is None else exp
    got = imgproc.find_charuco_corners(images, *args(setup), return_info=True, **kw)
    for key, g in zip(KEYS, got):
        same(g, exp[key], key)
    return exp


@pytest.fixture(scope="module")
def mixed():
    images, names = cc.mixed_batch()
    exp = ref.find(images, **cc.SMALL.kwargs())
    for a in exp.values():
        a.setflags(write=False)
    return images, names, exp


def test_every_fixture_in_one_batch_equals_the_restatement(mixed):
    images, names, exp = mixed
    check(images, cc.SMALL, exp)
    assert exp["found"].tolist() == [cc.expected(k) is not None for k in names]
    got = imgproc.find_charuco_corners(images, *args(cc.SMALL))[1]
    for k, name in enumerate(names):
        v = cc.expected(name)
        if v is not None:
            seen = ~np.isnan(got[k, :, 0])
            assert not (v["required"] & ~seen).any() and np.abs(got[k][seen] - v["truth"][seen]).max() <= MAX_OFFSET, name


def test_the_wide_board_with_6x6_bits():
    images = np.stack([cc.view("wide")["img"], cc.view("wide_cut")["img"]])
    exp = check(images, cc.WIDE)
    assert exp["found"].all() and np.isnan(exp["corners"][1]).any() and not np.isnan(exp["corners"][0]).any()
    for k, name in enumerate(("wide", "wide_cut")):
        seen = ~np.isnan(exp["corners"][k, :, 0])
        assert np.abs(exp["corners"][k][seen] - cc.view(name)["truth"][seen]).max() <= MAX_OFFSET


def test_a_frame_alone_and_at_any_place_of_a_batch(mixed):
    images, names, exp = mixed
    for k in (1, names.index("covered"), names.index("blank"), len(names) - 1):
        alone = imgproc.find_charuco_corners(images[k], *args(cc.SMALL), return_info=True)
        assert isinstance(alone[0], bool) and alone[1].shape == (12, 2) and alone[2].shape == (20,)
        for key, a in zip(KEYS, alone):
            same(np.asarray(a), exp[key][k], (names[k], key))
    order = np.array([9, 0, 14, 5, 13, 8, 3, 11, 1, 12, 2])
    got = imgproc.find_charuco_corners(images[order], *args(cc.SMALL), return_info=True)
    for key, g in zip(KEYS, got):
        same(g, exp[key][order], key)


def test_numpy_cuda_colour_and_inverted_inputs_agree(mixed):
    images, names, exp = mixed
    t = torch.from_numpy(images).cuda()
    got = imgproc.find_charuco_corners(t, *args(cc.SMALL), return_info=True)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got) and got[0].dtype == torch.bool
    for key, g in zip(KEYS, got):
        same(g, exp[key], key)
    one = imgproc.find_charuco_corners(t[1], *args(cc.SMALL))
    assert one[0].shape == () and bool(one[0]) and np.array_equal(host(one[1]), exp["corners"][1])
    # colour: the detector sees cvt_gray's image
    rgb = np.stack([sc.colour(i) for i in images[:3]])
    want = ref.find(subpix_ref.gray(rgb, "bgr"), **cc.SMALL.kwargs())
    assert want["found"].all()
    for rgb_in in (rgb, torch.from_numpy(rgb).cuda()):
        for key, g in zip(KEYS, imgproc.find_charuco_corners(rgb_in, *args(cc.SMALL), return_info=True)):
            same(g, want[key], key)
    # a board printed inverted: the board inverts the image back
    board = ca.CharucoBoard(cc.SMALL.squares, 30.0, 20.0, cc.SMALL.dictionary, cc.SMALL.first_id, invert_color=True)
    assert board.marker_ratio == cc.SMALL.ratio
    for inverted in (255 - images, 255 - t):
        for key, g in zip(KEYS, board._detect(inverted, return_info=True)):
            same(g, exp[key], key)
    assert not imgproc.find_charuco_corners(255 - images[:3], *args(cc.SMALL))[0].any()


def test_odd_sizes_pitches_and_strides(mixed):
    # 317 x 237 out of 331 x 245: width, pitch and stride no multiples of 4, 8 or 16; a view whose rows and frames lie apart
    rng = np.random.default_rng(7)
    images, names, _ = mixed
    big = rng.integers(0, 256, (4, 245, 331), dtype=np.uint8)
    for k, name in enumerate(("tilted", "turn90", "cut_left", "covered")):
        big[k, 2:242, 5:325] = images[names.index(name)]
    view = torch.from_numpy(big).cuda()[:, 3:240, 7:324]
    assert not view.is_contiguous() and view.shape == (4, 237, 317)
    tight = np.ascontiguousarray(big[:, 3:240, 7:324])
    exp = ref.find(tight, relative=6, nms_radius=2, **cc.SMALL.kwargs())
    assert exp["found"].all()
    check(tight, cc.SMALL, exp, relative=6, nms_radius=2)
    for key, g in zip(KEYS, imgproc.find_charuco_corners(view, *args(cc.SMALL), relative=6, nms_radius=2, return_info=True)):
        same(g, exp[key], key)
    for key, g in zip(KEYS, imgproc.find_charuco_corners(view[1::2], *args(cc.SMALL), relative=6, nms_radius=2, return_info=True)):
        same(g, exp[key][1::2], key)
    # five frames: a workgroup of four and one more; min_markers and max_bit_errors take part
    five = np.ascontiguousarray(images[[0, 3, 9, 12, 14]])
    exp3 = ref.find(five, min_markers=3, max_errors=1, **cc.SMALL.kwargs())
    got = imgproc.find_charuco_corners(five, *args(cc.SMALL), min_markers=3, max_bit_errors=1, return_info=True)
    for key, g in zip(KEYS, got):
        same(g, exp3[key], key)
    assert exp3["status"].tolist().count(ref.NO_CONSENSUS) >= 1  # (the covered view shows two markers only)


def test_limits_are_refused():
    img = cc.view("frontal")["img"]
    base = dict(squares_xy=cc.SMALL.squares, dictionary=cc.SMALL.dictionary, marker_ratio=cc.SMALL.ratio, first_id=cc.SMALL.first_id)
    for kw in (dict(squares_xy=(2, 4)), dict(squares_xy=(17, 4)), dict(squares_xy=(5.5, 4)), dict(marker_ratio=(3, 3)),
               dict(marker_ratio=(1, 65)), dict(first_id=4), dict(first_id=-1), dict(dictionary=cc.SMALL.dictionary[:, :3, :3]),
               dict(dictionary=cc.SMALL.dictionary.astype(np.float32)), dict(relative=65), dict(nms_radius=0), dict(min_markers=0),
               dict(max_bit_errors=17)):
        with pytest.raises(ValueError):
            imgproc.find_charuco_corners(img, **dict(base, **kw))
    with pytest.raises(ValueError):
        imgproc.find_charuco_corners(img[:2], **base)
    found, corners = imgproc.find_charuco_corners(img, (16, 16), boards.make_marker_dictionary(128, 4, 0, 2), (1, 2))
    assert found is False and corners.shape == (225, 2) and np.isnan(corners).all()  # the largest board: none here


def calibrated(frames, setup):
    return ca.Cam.from_detections(frames, (setup.hw[1], setup.hw[0]), undistorted=True).calibrate()


@pytest.fixture(scope="module")
def wide_board():
    return ca.CharucoBoard(cc.WIDE.squares, 30.0, 22.5, cc.WIDE.dictionary, cc.WIDE.first_id)


def test_a_camera_from_a_recording_of_partial_views(wide_board):
    images, truth = cc.recording()
    board = wide_board
    assert board.marker_ratio == cc.WIDE.ratio
    seen, corners, found, marker_ids, status, counts = board.find_image_points_batch(images, return_info=True)
    assert found.all() and not seen.all(1).any() and (seen.sum(1) >= 20).all()  # no frame shows the whole board
    assert np.isnan(corners[~seen]).all() and np.abs(corners[seen] - truth[seen]).max() <= 0.5
    coarse = imgproc.find_charuco_corners(images, *args(cc.WIDE))[1]
    same(np.isnan(coarse[..., 0]), ~seen)
    same(corners[seen], imgproc.corner_sub_pix(images, coarse[seen], boards.SUBPIX_WIN, boards.SUBPIX_ZERO_ZONE,
                                               boards.SUBPIX_CRITERIA, counts=seen.sum(1)))
    on_device = board.find_image_points_batch(torch.from_numpy(images).cuda())
    assert all(v.is_cuda for v in on_device)
    same(on_device[0], seen)
    same(on_device[1], corners)
    frames = board.to_frames(seen, corners, keys=["f%02d" % k for k in range(len(images))])
    assert len(frames) == len(images) and list(frames["f03"]["ids"]) == list(np.flatnonzero(seen[3]))
    analytic = board.to_frames(seen, np.where(seen[..., None], truth, np.nan).astype(np.float32), keys=list(frames))
    cam, want = calibrated(frames, cc.WIDE), calibrated(analytic, cc.WIDE)
    pick = lambda K: np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])  # noqa: E731
    difference = float(np.abs(pick(cam.K) / pick(want.K) - 1).max())
    print("K from detections against K from the analytic corners of the same ids: %.3g; against the camera: %.3g; retval %.3g"
          % (difference, float(np.abs(pick(cam.K) / pick(cc.WIDE.K) - 1).max()), cam.retval))
    assert difference <= K_DIFFERENCE
    assert np.abs(pick(want.K) / pick(cc.WIDE.K) - 1).max() < 1e-3  # (the analytic corners, rounded to float32, give the camera)
    # one record at a time, as the reference's loop
    d = dict(img=images[6])
    board.find_image_points(d)
    assert set(d) == {"img", "marker_ids", "ids", "image_points", "object_points", "corners"}
    assert list(d["ids"]) == list(np.flatnonzero(seen[6])) and d["corners"].shape == (len(d["ids"]), 1, 2)
    for i in d["ids"]:
        same(d["image_points"][i], corners[6, i][None])
        assert d["object_points"][i] is board.object_points[i]
    same(np.sort(d["marker_ids"]), np.sort(marker_ids[6][marker_ids[6] >= 0]))
    for img in (cc.blank(), torch.from_numpy(cc.view("plain")["img"]).cuda()):
        d = dict(img=img)
        ca.CharucoBoard(cc.SMALL.squares, 30.0, 20.0, cc.SMALL.dictionary, cc.SMALL.first_id).find_image_points(d)
        assert set(d) == {"img", "marker_ids"} and len(d["marker_ids"]) == 0


def test_a_rig_from_two_recordings_whose_ids_partly_overlap(wide_board):
    board = wide_board
    cams, seen_by = [], []
    for second in (False, True):
        images = cc.recording(second)[0][:cc.RIG_FRAMES]
        seen, corners = board.find_image_points_batch(images)
        cam = ca.Cam.from_detections(board.to_frames(seen, corners), (cc.WIDE.hw[1], cc.WIDE.hw[0]), undistorted=True)
        cam.K, cam.D = cc.WIDE.K.copy(), np.zeros((1, 5))
        cams.append(cam)
        seen_by.append(seen)
    common = seen_by[0] & seen_by[1]
    assert (common.sum(1) >= 11).all() and (common != seen_by[0]).any() and (common != seen_by[1]).any()
    rig = ca.Stereo(cams[0], cams[1])
    uvs1, uvs2, xyzs = rig.get_conjoint_points()
    assert [len(a) for a in uvs1] == common.sum(1).tolist() == [len(a) for a in xyzs]
    # the corners are within 0.5 px at 300 px focal length and 0.2 m: half a millimetre across, and a rotation of 0.5 / 300 rad
    print("rig: |t - truth| = %.3g m, |R - truth| = %.3g, retval %.3g" % (np.abs(rig.t[:, 0] - cc.RIG_T).max(),
                                                                          np.abs(rig.R - cc.RIG_R).max(), rig.retval))
    assert np.abs(rig.t[:, 0] - cc.RIG_T).max() < 5e-4 and np.abs(rig.R - cc.RIG_R).max() < 0.5 / 300 and rig.retval < 0.5
