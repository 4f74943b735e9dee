"""The host side of the intrinsic calibration without a GPU: the NumPy restatement tests/calibrate_ref.py against the truth,
its start, the measured summation-order tolerance of tests/golden/calibrate_tolerance.json, every refusal of
``calibrate_camera`` before the device, the check order of the new entry points, the exports, and the wiring of
``Cam.from_detections(...).calibrate()``."""
import ctypes

import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import _native, calibrate

import calibrate_cases as cc
import calibrate_ref as ref
import calibrate_tolerance as tolerance
import pnp_cases as pc


@pytest.fixture()
def no_device(monkeypatch):
    """any step towards the device fails the test"""
    def touched(*a, **k):
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(_native, "require_device", touched)
    monkeypatch.setattr(_native, "call", touched)
    monkeypatch.setattr(_native, "lib", touched)


@pytest.mark.parametrize("name", cc.NAMES)
def test_restatement_recovers_the_truth(name):
    """noise-free: the true K, D and poses within the distance the tolerance file records, well below the cap"""
    rec = tolerance.load()
    c, r = tolerance.solved(name, False)
    assert r["camera_status"] == 0 and r["evaluations"] < ref.MAX_EVALUATIONS / 2
    assert [int(s) for s in np.flatnonzero(r["status"])] == sorted(c["bad"]) and all(r["status"][f] == w for f, w in c["bad"].items())
    d = tolerance.truth_distance(c, r)
    assert all(d[k] <= rec["truth_distance"][k] for k in tolerance.KEYS), d
    assert max(d["K"], d["D"], d["T"]) < 1e-9


@pytest.mark.parametrize("noisy", [False, True])
def test_the_start_is_within_three_percent_of_the_focal_lengths(noisy):
    worst = 0.0
    for name in cc.NAMES:
        c, r = tolerance.solved(name, noisy)
        if c["K_guess"] is None:
            worst = max(worst, abs(r["K0"][0, 0] / c["K"][0, 0] - 1), abs(r["K0"][1, 1] / c["K"][1, 1] - 1))
            assert r["K0"][0, 2] == (cc.W - 1) / 2 and r["K0"][1, 2] == (cc.H - 1) / 2
    print("largest relative error of the start's focal lengths: %.4f" % worst)
    assert worst < 0.03


def test_the_package_starts_where_the_restatement_starts():
    c = cc.case("f5-n70", seed=cc.SEED)
    Hs = [ref.homography(o, u, np.eye(3)) for o, u in zip(c["obj"], c["uv"])]
    assert np.array_equal(calibrate.initial_camera_matrix(np.stack(Hs + [np.full((3, 3), np.nan)]), c["xy"]),
                          ref.initial_camera_matrix(Hs, c["xy"]))
    for flags in (0, ref.FIX_K3, cc.cal.UNDISTORTED_FLAGS, ref.FIX_PRINCIPAL_POINT, ref.FIX_FOCAL_LENGTH | ref.FIX_K1 | ref.FIX_K2):
        assert np.array_equal(calibrate.free_mask(flags) != 0, ref.free_mask(flags))
    assert calibrate.UNDISTORTED_FLAGS == cc.cal.UNDISTORTED_FLAGS


def test_noisy_cases_converge_to_the_noise_level():
    for name in cc.NAMES:
        c, r = tolerance.solved(name, True)
        assert r["camera_status"] == 0 and 0.3 < r["retval"] < 0.5, (name, r["retval"])  # sigma 0.3 px per component: ~0.42 px per point


def test_tolerance_file_is_the_measurement():
    """the bounds come from the restatement's own disagreement under a change of summation order, times 8 -- never from
    what the kernels give; every case ends below half the cap"""
    rec, now = tolerance.load(), tolerance.measure()
    assert rec["factor"] == 8 and all(rec["bound"][k] == 8 * rec["disagreement"][k] for k in tolerance.KEYS)
    assert all(0 < now["disagreement"][k] <= rec["bound"][k] for k in tolerance.KEYS)
    assert all(now["truth_distance"][k] <= 2 * rec["truth_distance"][k] for k in tolerance.KEYS)
    assert now["evaluations"] == rec["evaluations"] and sorted(rec["evaluations"]) == sorted(cc.NAMES)
    assert rec["evaluation_cap"] == ref.MAX_EVALUATIONS and max(rec["evaluations"].values()) < rec["evaluation_cap"] / 2


def test_refusals_come_before_the_device(no_device):
    obj, uv = np.zeros((3, 70, 3)), np.zeros((3, 70, 2))
    obj[:] = pc.board_points(70)
    xy = (cc.W, cc.H)
    K = pc.camera(0)[0]
    bad = [
        (dict(object_points=obj[..., :2], image_points=uv), ValueError, "object_points must be"),
        (dict(object_points=obj, image_points=uv[:, :60]), ValueError, "object_points must be"),
        (dict(object_points=obj.astype(np.float16), image_points=uv), ValueError, "float32 or float64"),
        (dict(object_points=obj, image_points=uv.astype(np.int32)), ValueError, "float32 or float64"),
        (dict(object_points=list(obj), image_points=uv), TypeError, "NumPy array or a torch CUDA tensor"),
        (dict(object_points=obj[0], image_points=uv[0]), ValueError, "unless counts is given"),
        (dict(object_points=obj.reshape(-1, 3), image_points=uv.reshape(-1, 2), counts=[70, 60, 70]), ValueError, "counts sum"),
        (dict(object_points=obj, image_points=uv, xy=(0, 720)), ValueError, "xy must be"),
        (dict(object_points=obj, image_points=uv, flags=0x2), ValueError, "flags 0x2 are not implemented"),       # aspect ratio
        (dict(object_points=obj, image_points=uv, flags=0x4000), ValueError, "not implemented"),                  # rational
        (dict(object_points=obj, image_points=uv, flags=0x8000), ValueError, "not implemented"),                  # thin prism
        (dict(object_points=obj, image_points=uv, flags=0x40000), ValueError, "not implemented"),                 # tilted
        (dict(object_points=obj, image_points=uv, flags=ca.CALIB_USE_INTRINSIC_GUESS), ValueError, "needs K"),
        (dict(object_points=obj, image_points=uv, flags=ca.CALIB_USE_INTRINSIC_GUESS, K=np.eye(4)), ValueError, "K must be"),
        (dict(object_points=obj, image_points=uv, flags=ca.CALIB_USE_INTRINSIC_GUESS, K=K, D=np.zeros(8)), ValueError, "D must hold"),
        (dict(object_points=obj[:, :3], image_points=uv[:, :3]), ValueError, "fewer than 4 points"),
        (dict(object_points=pc.cloud_points(70), image_points=uv), ValueError, "a target with depth needs"),
        (dict(object_points=obj[:, :4], image_points=uv[:, :4]), ValueError, "singular: 24 equations for 27 free unknowns"),
    ]
    for kw, exc, text in bad:
        kw.setdefault("xy", xy)
        with pytest.raises(exc, match=text):
            calibrate.calibrate_camera(**kw)
    cam = ca.Cam.from_detections({i: dict(image_points=uv[i, :4], object_points=obj[i, :4]) for i in range(3)}, xy)
    with pytest.raises(ValueError, match="singular"):
        cam.calibrate()
    assert not hasattr(cam, "K")
    with pytest.raises(ValueError, match="No any valid image"):
        ca.Cam.from_detections({}, xy).calibrate()


def test_the_new_entry_points_check_before_they_probe():
    """status and message of a null call and of a formed call (made-up device addresses, never read): every argument check
    comes before the device probe, and an empty batch launches nothing"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the formed calls must not reach a kernel")
    lib = _native.lib()
    A = lambda k: 0x7000000000 + (k << 20)  # noqa: E731
    plane = np.eye(3).ravel()
    out = np.zeros(_native.CALIB_STATE_DOUBLES)
    pts = _native.PnpPoints(A(0), A(1), A(2), 10, 10, _native.VALUE_F64, _native.VALUE_F32, 3, 2, 0, 2)
    none = _native.PnpPoints(A(0), A(1), A(2), 10, 10, _native.VALUE_F64, _native.VALUE_F32, 3, 2, 0, 0)
    p, e = ctypes.byref(pts), ctypes.byref(none)
    null = {"camd_calib_homography": (None, None, None, None), "camd_calib_linearise": (None, None, 0, None, None, None, None),
            "camd_calib_step": (None, None, 0, None, None, None, None, None),
            "camd_calib_finish": (None, None, 0, None, None, None, None), "camd_calib_read": (None, 1, None, None)}
    for name, args in null.items():
        assert getattr(lib, name)(*args) == _native.CAMD_ERR_BAD_ARG, name
        assert _native.last_error().startswith(name + ": bad arguments"), name
    NO, BAD, OK = _native.CAMD_ERR_NO_DEVICE, _native.CAMD_ERR_BAD_ARG, _native.CAMD_OK
    assert lib.camd_calib_homography(p, plane.ctypes.data, A(3), None) == NO
    assert lib.camd_calib_homography(p, None, A(3), None) == BAD and lib.camd_calib_homography(p, plane.ctypes.data, None, None) == BAD
    assert lib.camd_calib_homography(e, plane.ctypes.data, None, None) == OK
    assert lib.camd_calib_linearise(p, A(3), 2, A(4), A(5), A(6), None) == NO
    assert lib.camd_calib_linearise(p, A(3), 2, A(4), None, A(6), None) == BAD and lib.camd_calib_linearise(p, A(3), -1, A(4), A(5), A(6), None) == BAD
    assert lib.camd_calib_linearise(p, A(3) + 2, 2, A(4), A(5), A(6), None) == BAD
    assert lib.camd_calib_linearise(p, None, 0, None, None, None, None) == OK
    assert lib.camd_calib_step(p, A(3), 2, A(4), A(5), A(6), A(7), None) == NO
    assert lib.camd_calib_step(p, A(3), 2, A(4), A(5), None, A(7), None) == BAD and lib.camd_calib_step(p, A(3), 2, None, A(5), A(6), A(7), None) == BAD
    assert lib.camd_calib_step(e, A(3), 2, A(4), A(5), A(6), A(7), None) == BAD  # frames to use, and no frames
    assert lib.camd_calib_step(p, None, 0, None, None, None, None, None) == OK
    assert lib.camd_calib_finish(p, A(3), 2, A(4), A(5), A(6), None) == NO
    assert lib.camd_calib_finish(p, A(3), 2, A(4), A(5), None, None) == BAD
    assert lib.camd_calib_finish(p, None, 0, None, None, None, None) == OK
    assert lib.camd_calib_read(A(0), 2, out.ctypes.data, None) == NO
    assert lib.camd_calib_read(A(0), _native.CALIB_STATE_DOUBLES + 1, out.ctypes.data, None) == BAD
    assert lib.camd_calib_read(A(0), 2, None, None) == BAD and lib.camd_calib_read(None, 0, None, None) == OK


def test_the_header_and_the_binding_agree_on_the_state():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "calibrating_amd.h")).read()
    values = {k: int(v) for k, v in re.findall(r"(CAMD_CALIB_[A-Z_]+)\s*=?\s+(\d+)", src)}
    for name, value in values.items():
        assert getattr(_native, name[len("CAMD_"):]) == value, name
    assert len(values) == 16
    assert not re.search(r"camd_calib_\w+\([^;]*void\*\s*stream\)", src)  # the stream is spelt `queue`, as in camd_pnp_*


def test_exports():
    names = ["calibrate_camera", "CALIB_USE_INTRINSIC_GUESS", "CALIB_FIX_PRINCIPAL_POINT", "CALIB_FIX_FOCAL_LENGTH",
             "CALIB_ZERO_TANGENT_DIST", "CALIB_FIX_K1", "CALIB_FIX_K2", "CALIB_FIX_K3", "CALIB_FIX_K4", "CALIB_FIX_K5", "CALIB_FIX_K6"]
    assert all(n in ca.__all__ and hasattr(ca, n) for n in names)
    assert ca.calibrate_camera is calibrate.calibrate_camera
    # cv2's values
    assert [getattr(ca, n) for n in names[1:]] == [1, 4, 16, 8, 32, 64, 128, 2048, 4096, 8192]


def test_cam_calibrate_is_wired_to_the_solver(monkeypatch):
    board = pc.centred(pc.board_points(70))
    seen = {}

    def solver(object_points, image_points, xy, counts=None, flags=0, K=None, D=None):
        seen.update(obj=object_points, uv=image_points, xy=xy, counts=list(counts), flags=flags)
        f = len(counts)
        T = np.tile(np.eye(4), (f, 1, 1))
        T[:, 2, 3] = np.arange(f) + 1.0
        T[1, :3] = np.nan
        return dict(retval=0.25, K=np.array([[900.0, 0, 640], [0, 910, 360], [0, 0, 1]]), D=np.array([[0.1, 0, 0, 0, 0.0]]), T=T,
                    reprojection_error=np.array([0.1, np.nan, 0.3]), iterations=7, status=np.array([0, 2, 0], np.int32), evaluations=9)
    monkeypatch.setattr(calibrate, "calibrate_camera", solver)
    uv = np.arange(140.0).reshape(70, 2)
    frames = {"b": dict(image_points=uv + 1, object_points=board, T=np.eye(4)),
              "a": dict(image_points={9: uv[35:], 5: uv[:35]}, object_points={5: board[:35], 9: board[35:]}),
              "c": dict(image_points=uv[:12] + 2, object_points=board[:12]),
              "empty": dict(image_points=np.zeros((0, 2)), object_points=board), "seen_only": dict(image_points=uv[:4])}
    cam = ca.Cam.from_detections(frames, (1280, 720), name="left", undistorted=True, calibrate_flags=ca.CALIB_FIX_K3)
    assert not hasattr(cam, "K") and cam.name == "left" and cam.xy == (1280, 720)
    assert cam.calibrate() is cam
    assert seen["counts"] == [70, 70, 12] and seen["xy"] == (1280, 720) and seen["flags"] == calibrate.UNDISTORTED_FLAGS
    assert np.array_equal(seen["uv"], np.concatenate([uv, uv + 1, uv[:12] + 2])) and np.array_equal(seen["obj"][:70], board)
    assert cam.retval == 0.25 and cam.K[0, 0] == 900 and cam.D.shape == (1, 5)
    assert cam["a"]["T"][2, 3] == 1 and cam["c"]["T"][2, 3] == 3 and cam["c"]["reprojection_error"] == 0.3
    assert "T" not in cam["b"] and "T" not in cam["seen_only"] and "T" not in cam["empty"]  # the bad frame lost its earlier pose
    rec = cam.dump(return_dict=True)
    assert rec["retval"] == 0.25 and rec["fx"] == 900.0 and ca.Cam.load(rec).K[1, 1] == 910
    plain = ca.Cam.from_detections(frames, (1280, 720), calibrate_flags=ca.CALIB_FIX_K3)
    plain.calibrate()
    assert seen["flags"] == ca.CALIB_FIX_K3
    assert ca.Cam(cam.K, cam.D, cam.xy).xy == (1280, 720)  # the constructor keeps its signature
