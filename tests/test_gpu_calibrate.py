"""Intrinsic calibration on the MI355X (-m gpu): ``calibrate_camera`` and ``Cam.from_detections(...).calibrate()`` against the
NumPy restatement tests/calibrate_ref.py within the measured summation-order bounds of
tests/golden/calibrate_tolerance.json, against the truth of the noise-free cases, and against themselves bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import geometry  # noqa: E402

import calibrate_cases as cc  # noqa: E402
import calibrate_tolerance as tolerance  # noqa: E402
import pnp_cases as pc  # noqa: E402

KEYS = ("retval", "K", "D", "T", "reprojection_error", "iterations", "status", "evaluations")


def host(r):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def same_bits(a, b):
    a, b = host(a), host(b)
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def run(c, **kw):
    obj, uv, counts = cc.rows(c)
    return ca.calibrate_camera(obj, uv, c["xy"], counts=counts, flags=c["flags"], K=c["K_guess"], **kw)


@pytest.fixture(scope="module")
def tol():
    return tolerance.load()


@pytest.mark.parametrize("noisy", [False, True], ids=["noise-free", "noisy"])
@pytest.mark.parametrize("name", cc.NAMES)
def test_every_case_agrees_with_the_restatement(name, noisy, tol):
    """K, D, T, retval and the per-frame errors within 8 x the restatement's own forward / reversed disagreement; status and
    the set of used frames equal; noise-free cases also against the truth, within the restatement's recorded distance from
    it plus that bound."""
    c, want = tolerance.solved(name, noisy)
    got = run(c)
    assert sorted(got) == sorted(KEYS) and all(isinstance(got[k], np.ndarray) for k in ("K", "D", "T", "reprojection_error", "status"))
    assert got["K"].shape == (3, 3) and got["D"].shape == (1, 5) and got["T"].shape == (len(c["counts"]), 4, 4)
    assert got["K"].dtype == got["D"].dtype == got["T"].dtype == np.float64 and isinstance(got["retval"], float)
    assert np.array_equal(got["status"], want["status"]) and got["evaluations"] <= 100
    used = got["status"] == 0
    assert np.isnan(got["T"][~used, :3]).all() and np.isnan(got["reprojection_error"][~used]).all()
    d = tolerance.difference(dict(got, status=want["status"]), want)
    print("%s: |gpu - restatement| %s; evaluations %d (restatement %d)" % (name, d, got["evaluations"], want["evaluations"]))
    assert all(d[k] <= tol["bound"][k] for k in tolerance.KEYS), d
    if not noisy:
        t = tolerance.truth_distance(c, dict(got, status=want["status"]))
        print("%s: |gpu - truth| %s" % (name, t))
        assert all(t[k] <= tol["truth_distance"][k] + tol["bound"][k] for k in tolerance.KEYS), t


def test_the_same_call_twice_gives_the_same_bits():
    for name in ("f5-n70", "f65-n12"):
        c, _ = tolerance.solved(name, True)
        assert same_bits(run(c), run(c)), name


def test_ndarray_cuda_and_float32_rows_give_the_same_result(tol):
    """the 9-frame case on pixels that are exact in float32: (f, n, .) ndarrays, CUDA tensors, ragged rows and float32
    image rows are the same numbers, so the same bits come back; and they are the truth"""
    p = cc.case_from_pixels(9, 70)
    assert p["uv"].dtype == np.float32
    uv64 = p["uv"].astype(np.float64)
    a = ca.calibrate_camera(p["obj"], uv64, p["xy"])
    b = ca.calibrate_camera(torch.from_numpy(p["obj"]).cuda(), torch.from_numpy(uv64).cuda(), p["xy"])
    assert all(isinstance(b[k], torch.Tensor) and b[k].is_cuda for k in ("T", "reprojection_error", "status"))
    assert isinstance(b["K"], np.ndarray) and isinstance(b["D"], np.ndarray) and isinstance(b["retval"], float)
    assert same_bits(a, b)
    assert same_bits(a, ca.calibrate_camera(p["obj"], p["uv"], p["xy"]))
    assert same_bits(a, ca.calibrate_camera(torch.from_numpy(p["obj"]).cuda(), torch.from_numpy(p["uv"]).cuda(), p["xy"]))
    assert same_bits(a, ca.calibrate_camera(p["obj"].reshape(-1, 3), p["uv"].reshape(-1, 2), p["xy"], counts=[70] * 9))
    t = tolerance.truth_distance(dict(p, D=p["D"]), a)
    print("float32 pixels: |gpu - truth| %s" % t)
    assert all(t[k] <= tol["truth_distance"][k] + tol["bound"][k] for k in ("K", "D", "T"))


def test_a_bad_frame_in_the_middle_changes_nothing_else():
    c, _ = tolerance.solved("bad-frames", True)
    whole = run(c)
    good = [f for f in range(len(c["counts"])) if f not in c["bad"]]
    without = ca.calibrate_camera(np.concatenate([c["obj"][f] for f in good]), np.concatenate([c["uv"][f] for f in good]), c["xy"],
                                  counts=[c["counts"][f] for f in good])
    assert [int(s) for s in whole["status"]] == [c["bad"].get(f, 0) for f in range(len(c["counts"]))]
    for k in ("retval", "K", "D", "iterations", "evaluations"):
        assert np.array_equal(whole[k], without[k]), k
    assert np.array_equal(whole["T"][good], without["T"]) and np.array_equal(whole["reprojection_error"][good], without["reprojection_error"])
    for f in c["bad"]:
        assert np.isnan(whole["T"][f, :3]).all() and np.isnan(whole["reprojection_error"][f])


def test_too_few_equations_are_singular_and_leave_the_camera_alone():
    c, _ = tolerance.solved("f3-n70", False)
    frames = {i: dict(image_points=u[:4], object_points=o[:4])
              for i, (o, u) in enumerate(zip(c["obj"], c["uv"]))}
    cam = ca.Cam.from_detections(frames, c["xy"])
    with pytest.raises(ValueError, match="singular"):
        cam.calibrate()
    assert not hasattr(cam, "K")
    with pytest.raises(ValueError, match="singular"):  # CUDA points: refused before a launch
        ca.calibrate_camera(torch.from_numpy(np.stack([o[:4] for o in c["obj"]])).cuda(),
                            torch.from_numpy(np.stack([u[:4] for u in c["uv"]])).cuda(), c["xy"])


def test_two_calibrated_cameras_make_the_rig(tol):
    """detections -> K, D and every frame's pose -> get_T_cam2_in_self -> Stereo.load, noise-free: the true rig pose within
    what the poses' bound (the restatement's distance from the truth plus the summation-order bound) becomes in
    T1 inv(T2): |d(T1 T2^-1)| <= |dT1| |T2^-1| + |T1| |T2^-1|^2 |dT2| in the row-sum norm, which bounds every entry"""
    xy = (cc.W, cc.H)
    K1, D1 = cc.true_camera("lens", 0)
    K2, D2 = cc.true_camera("lens", 1)
    rig = np.eye(4)  # camera 2 in camera 1
    rig[:3, :3] = geometry.rodrigues(np.array([0.02, -0.15, 0.01]))
    rig[:3, 3] = [-0.06, 0.004, 0.01]
    board = pc.centred(pc.board_points(70))
    frames1, frames2, T1s, T2s = {}, {}, [], []
    for i, T2 in enumerate(cc.poses(6, seed=3)):
        T1 = rig @ T2
        frames1["f%d" % i] = dict(image_points=pc.observe(board, T1, K1, D1), object_points=board)
        uv2 = pc.observe(board, T2, K2, D2)
        frames2["f%d" % i] = dict(image_points={5: uv2[:35], 9: uv2[35:]}, object_points={5: board[:35], 9: board[35:]})
        T1s.append(T1), T2s.append(T2)
    cam1 = ca.Cam.from_detections(frames1, xy, name="a").calibrate()
    cam2 = ca.Cam.from_detections(frames2, xy, name="b").calibrate()
    e = tol["truth_distance"]["T"] + tol["bound"]["T"]
    for cam, K, D in ((cam1, K1, D1), (cam2, K2, D2)):
        assert np.abs(cam.K - K).max() <= tol["truth_distance"]["K"] + tol["bound"]["K"]
        assert np.abs(cam.D.ravel() - D).max() <= tol["truth_distance"]["D"] + tol["bound"]["D"]
        assert cam.retval < 1e-9
    norm = lambda M: np.abs(M).sum(1).max()  # noqa: E731
    bound = max(4 * e * norm(np.linalg.inv(b)) + norm(a) * norm(np.linalg.inv(b)) ** 2 * 4 * e for a, b in zip(T1s, T2s))
    T = cam1.get_T_cam2_in_self(cam2)
    want = geometry.R_t_to_T(rig[:3, :3], rig[:3, 3])  # both through R_t_to_T's float32 rotation
    print("rig: |T - truth| %.3e rotation, %.3e translation (bound %.3e)" % (np.abs(T - want)[:3, :3].max(), np.abs(T - want)[:3, 3].max(), bound))
    assert np.abs(T - want)[:3, 3].max() <= bound
    assert np.abs(T - want)[:3, :3].max() <= bound + 2.0 ** -24  # one float32 rounding of an entry below 1
    R, t = np.linalg.inv(T)[:3, :3], np.linalg.inv(T)[:3, 3]
    stereo = ca.Stereo.load(dict(R=R.tolist(), t=t.tolist(), cam1=cam1.dump(return_dict=True), cam2=cam2.dump(return_dict=True)))
    assert tuple(stereo.xy) == xy and np.isfinite(stereo.K).all()
    depth2 = np.full(xy[::-1], 0.9)
    assert np.array_equal(cam1.project_cam2_depth(cam2, depth2), cam1.project_cam2_depth(cam2, depth2, T=T))
