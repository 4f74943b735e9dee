"""Stereo calibration on the MI355X (-m gpu): ``stereo_calibrate`` and ``Stereo(cam1, cam2)`` against the NumPy restatement
tests/stereo_calibrate_ref.py within the measured summation-order bounds of tests/golden/stereo_calibrate_tolerance.json,
against the truth of the noise-free cases, and against themselves bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402

import stereo_calibrate_cases as sc  # noqa: E402
import stereo_calibrate_tolerance as tolerance  # noqa: E402

KEYS = ("retval", "R", "t", "T", "reprojection_error", "iterations", "status", "evaluations")


def host(r):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def same_bits(a, b):
    a, b = host(a), host(b)
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def run(c, **kw):
    obj, uv1, uv2, counts = sc.rows(c)
    return ca.stereo_calibrate(obj, uv1, uv2, c["K1"], c["D1"], c["K2"], c["D2"], counts=counts, **kw)


@pytest.fixture(scope="module")
def tol():
    return tolerance.load()


@pytest.mark.parametrize("noisy", [False, True], ids=["noise-free", "noisy"])
@pytest.mark.parametrize("name", sc.NAMES)
def test_every_case_agrees_with_the_restatement(name, noisy, tol):
    """R, t, T, retval and the per-frame errors within 8 x the restatement's own forward / reversed disagreement; status
    equal; NaN exactly where the status is not 0; noise-free cases also against the truth, within the restatement's recorded
    distance from it plus that bound."""
    c, want = tolerance.solved(name, noisy)
    got = run(c)
    assert sorted(got) == sorted(KEYS) and all(isinstance(got[k], np.ndarray) for k in ("R", "t", "T", "reprojection_error", "status"))
    assert got["R"].shape == (3, 3) and got["t"].shape == (3, 1) and got["T"].shape == (len(c["counts"]), 4, 4)
    assert got["R"].dtype == got["t"].dtype == got["T"].dtype == np.float64 and isinstance(got["retval"], float)
    assert np.array_equal(got["status"], want["status"]) and got["evaluations"] <= 100
    used = got["status"] == 0
    assert np.isnan(got["T"][~used, :3]).all() and np.isnan(got["reprojection_error"][~used]).all()
    assert np.isfinite(got["T"][used]).all() and np.isfinite(got["reprojection_error"][used]).all()
    d = tolerance.difference(dict(got, status=want["status"]), want)
    print("%s: |gpu - restatement| %s; evaluations %d (restatement %d)" % (name, d, got["evaluations"], want["evaluations"]))
    assert all(d[k] <= tol["bound"][k] for k in tolerance.KEYS), d
    if not noisy:
        t = tolerance.truth_distance(c, dict(got, status=want["status"]))
        print("%s: |gpu - truth| %s" % (name, t))
        assert all(t[k] <= tol["truth_distance"][k] + tol["bound"][k] for k in tolerance.KEYS), t


def test_the_same_call_twice_gives_the_same_bits():
    for name in ("f5-n70", "f130-n12"):
        c, _ = tolerance.solved(name, True)
        assert same_bits(run(c), run(c)), name


def test_ndarray_cuda_ragged_and_float32_rows_give_the_same_bits():
    """pixels that are exact in float32: (f, n, .) ndarrays with a shared board, CUDA tensors, ragged rows with counts and
    float32 image rows are the same numbers, so the same bits come back"""
    p = sc.case_from_pixels()
    assert p["uv1"].dtype == p["uv2"].dtype == np.float32
    f, n = p["uv1"].shape[:2]
    cams = (p["K1"], p["D1"], p["K2"], p["D2"])
    a64, b64 = p["uv1"].astype(np.float64), p["uv2"].astype(np.float64)
    cuda = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    a = ca.stereo_calibrate(p["obj"], a64, b64, *cams)
    b = ca.stereo_calibrate(cuda(p["obj"]), cuda(a64), cuda(b64), *cams)
    assert all(isinstance(b[k], torch.Tensor) and b[k].is_cuda for k in ("T", "reprojection_error", "status"))
    assert isinstance(b["R"], np.ndarray) and isinstance(b["t"], np.ndarray) and isinstance(b["retval"], float)
    assert same_bits(a, b)
    assert same_bits(a, ca.stereo_calibrate(p["obj"], p["uv1"], p["uv2"], *cams))
    assert same_bits(a, ca.stereo_calibrate(cuda(p["obj"]), cuda(p["uv1"]), cuda(p["uv2"]), *cams))
    assert same_bits(a, ca.stereo_calibrate(np.tile(p["obj"], (f, 1, 1)), a64, b64, *cams))
    assert same_bits(a, ca.stereo_calibrate(np.tile(p["obj"], (f, 1)), a64.reshape(-1, 2), b64.reshape(-1, 2), *cams, counts=[n] * f))
    assert a["retval"] < 1e-4 and np.abs(a["R"] - p["R"]).max() < 1e-6 and np.abs(a["t"].ravel() - p["t"]).max() < 1e-6


def test_bad_frames_change_nothing_else():
    c, _ = tolerance.solved("bad-frames", True)
    whole = run(c)
    assert [int(s) for s in whole["status"]] == [c["bad"].get(f, 0) for f in range(len(c["counts"]))]
    good = [f for f in range(len(c["counts"])) if whole["status"][f] == 0]
    assert good == [0, 2, 4, 5]
    without = ca.stereo_calibrate(np.concatenate([c["obj"][f] for f in good]), np.concatenate([c["uv1"][f] for f in good]),
                                  np.concatenate([c["uv2"][f] for f in good]), c["K1"], c["D1"], c["K2"], c["D2"],
                                  counts=[c["counts"][f] for f in good])
    for k in ("retval", "R", "t", "iterations", "evaluations"):
        assert np.array_equal(whole[k], without[k]), k
    assert np.array_equal(whole["T"][good], without["T"]) and np.array_equal(whole["reprojection_error"][good], without["reprojection_error"])
    for f in range(len(c["counts"])):
        if f not in good:
            assert np.isnan(whole["T"][f, :3]).all() and np.isnan(whole["reprojection_error"][f])


def test_an_extrinsic_guess_reaches_the_same_minimum(tol):
    c, _ = tolerance.solved("f5-n70", True)
    a = run(c)
    R0, t0 = sc.perturbed_rig(c["R"], c["t"])
    b = run(c, flags=ca.CALIB_FIX_INTRINSIC | ca.CALIB_USE_EXTRINSIC_GUESS, R=R0, t=t0)
    d = tolerance.difference(a, b)
    print("guess: |median start - guess start| %s; evaluations %d and %d" % (d, a["evaluations"], b["evaluations"]))
    assert all(d[k] <= tol["bound"][k] for k in tolerance.KEYS), d


def test_a_rig_that_cannot_be_solved_raises_status_3():
    """one frame whose points are collinear in both cameras: no pose, no rig"""
    c, _ = tolerance.solved("f1-n70", False)
    line = np.zeros((6, 3))
    line[:, 0] = np.linspace(-0.1, 0.1, 6)
    import pnp_cases as pc
    T12 = np.eye(4)
    T12[:3, :3], T12[:3, 3] = c["R"], c["t"]
    uv1 = pc.observe(line, c["T"][0], c["K1"], c["D1"])
    uv2 = pc.observe(line, T12 @ c["T"][0], c["K2"], c["D2"])
    with pytest.raises(ValueError, match="status 3"):
        ca.stereo_calibrate(line[None], uv1[None], uv2[None], c["K1"], c["D1"], c["K2"], c["D2"])


def _calibrated_cameras(frames1, frames2, xy):
    cam1 = ca.Cam.from_detections(frames1, xy, name="left").calibrate()
    cam2 = ca.Cam.from_detections(frames2, xy, name="right").calibrate()
    return cam1, cam2


def test_detections_to_the_rig_end_to_end():
    """Cam.from_detections x 2, each calibrated, then Stereo(cam1, cam2): R, t, retval are the array call's on
    get_conjoint_points(); dump -> load round-trips; the R=, t= path builds the same device tables"""
    c, _ = tolerance.solved("f5-n70", True)
    xy = (sc.W, sc.H)
    frames1 = {"f%d" % i: dict(image_points=u, object_points=o) for i, (o, u) in enumerate(zip(c["obj"], c["uv1"]))}
    frames2 = {"f%d" % i: dict(image_points=u, object_points=o) for i, (o, u) in enumerate(zip(c["obj"], c["uv2"]))}
    frames2["only_right"] = dict(image_points=c["uv2"][0], object_points=c["obj"][0])
    cam1, cam2 = _calibrated_cameras(frames1, frames2, xy)
    s = ca.Stereo(cam1, cam2)
    uvs1, uvs2, xyzs = s.get_conjoint_points()
    assert len(uvs1) == 5 and all(np.array_equal(a, b) for a, b in zip(uvs1, c["uv1"]))
    want = ca.stereo_calibrate(np.concatenate(xyzs), np.concatenate(uvs1), np.concatenate(uvs2), cam1.K, cam1.D, cam2.K, cam2.D,
                               counts=[len(a) for a in uvs1])
    assert np.array_equal(s.R, want["R"]) and np.array_equal(s.t, want["t"]) and s.retval == want["retval"]
    assert s.t.shape == (3, 1) and 0.3 < s.retval < 0.5 and abs(np.linalg.norm(s.t) - np.linalg.norm(c["t"])) < 5e-3
    again = ca.Stereo.load(s.dump(return_dict=True))
    assert np.array_equal(again.R, s.R) and np.array_equal(again.t, s.t) and again.retval == s.retval
    other = ca.Stereo(cam1, cam2, R=s.R, t=s.t)
    ta, tb = s._tables("cuda"), other._tables("cuda")
    assert all(torch.equal(ta[k], tb[k]) for k in ta)


def test_marker_detections_where_camera_2_misses_ids(tol):
    c, want = tolerance.solved("markers", True)
    full = sc.case("f5-n70", sigma=sc.NOISE_SIGMA, seed=sc.NOISY_SEED)
    frames1, frames2 = sc.marker_frames(full["obj"], full["uv1"], full["uv2"])
    xy = (sc.W, sc.H)
    cam1 = ca.Cam.from_detections(frames1, xy, name="left")
    cam2 = ca.Cam.from_detections(frames2, xy, name="right")
    cam1.K, cam1.D, cam2.K, cam2.D = c["K1"], c["D1"].reshape(1, -1), c["K2"], c["D2"].reshape(1, -1)
    s = ca.Stereo(cam1, cam2)
    uvs1, uvs2, xyzs = s.get_conjoint_points()
    assert [len(a) for a in uvs1] == c["counts"] and all(np.array_equal(a, b) for a, b in zip(uvs2, c["uv2"]))
    got = run(c)
    assert np.array_equal(s.R, got["R"]) and np.array_equal(s.t, got["t"]) and s.retval == got["retval"]
    d = tolerance.difference(dict(got, status=want["status"]), want)
    assert all(d[k] <= tol["bound"][k] for k in tolerance.KEYS), d
