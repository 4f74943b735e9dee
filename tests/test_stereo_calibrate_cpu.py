"""The host side of the stereo calibration without a GPU: the NumPy restatement tests/stereo_calibrate_ref.py -- its
Jacobian blocks against finite differences, the noise-free cases against the truth, one noisy case against SciPy --, the
measured summation-order tolerance of tests/golden/stereo_calibrate_tolerance.json, every refusal of ``stereo_calibrate``
before the device, the kept ``NotImplementedError`` of ``Stereo(cam1, cam2)``, and ``get_conjoint_points`` against the
reference's own method (tests/golden/reference_conjoint.npz)."""
import importlib
import os

import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import _native

import pnp_cases as pc
import stereo_calibrate_cases as sc
import stereo_calibrate_ref as ref
import stereo_calibrate_tolerance as tolerance

module = importlib.import_module("calibrating_amd.stereo_calibrate")  # (the package's attribute of that name is the function)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_conjoint.npz")


@pytest.fixture()
def no_device(monkeypatch):
    """any step towards the device fails the test"""
    def touched(*a, **k):
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(_native, "require_device", touched)
    monkeypatch.setattr(_native, "call", touched)
    monkeypatch.setattr(_native, "lib", touched)


def test_the_jacobian_blocks_match_central_differences():
    """the frame's and the rig's block of both cameras on a handful of points, lenses of 5 / 5 and of 0 / 12 coefficients;
    step and bound: the restatement's FD_STEP, FD_BOUND (from the size of the third derivative)"""
    for name in ("f5-n70", "lens-0-12"):
        c = sc.case(name, sigma=sc.NOISE_SIGMA, seed=sc.NOISY_SEED)
        cams = (c["K1"], c["D1"], c["K2"], c["D2"])
        for f in (0, 3):
            at = slice(0, 70, 10)
            obj, u1, u2, T = c["obj"][f][at], c["uv1"][f][at], c["uv2"][f][at], c["T"][f]
            R0, t0 = sc.perturbed_rig(c["R"], c["t"], seed=f)  # off the minimum: the blocks do not rely on small residuals
            r1, J1, r2, Jf, Jr = ref.frame_terms(T[:3, :3], T[:3, 3], R0, t0, obj, u1, u2, cams)
            Ff, Fr = ref.finite_difference_blocks(T[:3, :3], T[:3, 3], R0, t0, obj, u1, u2, cams)
            n = len(r1)
            d = [np.abs(Ff[:n] - J1).max(), np.abs(Ff[n:] - Jf).max(), np.abs(Fr[:n]).max(), np.abs(Fr[n:] - Jr).max()]
            print("%s frame %d: |analytic - central difference| %s (entries up to %.0f)" % (name, f, d, np.abs(Jr).max()))
            assert max(d) <= ref.FD_BOUND and np.abs(Jr).max() > 100


@pytest.mark.parametrize("name", sc.NAMES)
def test_restatement_recovers_the_truth(name):
    """noise-free: the true R, t and poses within the distance the tolerance file records, below half the cap"""
    rec = tolerance.load()
    c, r = tolerance.solved(name, False)
    assert r["rig_status"] == 0 and r["evaluations"] < ref.MAX_EVALUATIONS / 2
    assert [int(s) for s in r["status"]] == [c["bad"].get(f, 0) for f in range(len(c["counts"]))]
    d = tolerance.truth_distance(c, r)
    assert all(d[k] <= rec["truth_distance"][k] for k in tolerance.KEYS), d
    assert max(d["R"], d["t"], d["T"]) < 1e-12


def test_noisy_cases_converge_to_the_noise_level():
    for name in sc.NAMES:
        c, r = tolerance.solved(name, True)
        # sigma 0.3 px per component: retval is the RMS over the components; four points leave few degrees of freedom
        assert r["rig_status"] == 0 and (0.2 if name == "f5-n4" else 0.27) < r["retval"] < 0.33 * np.sqrt(2), (name, r["retval"])


def test_tolerance_file_is_the_measurement():
    """the bounds come from the restatement's own disagreement under a change of summation order, times 8 -- never from
    what the kernels give; every case ends below half the cap"""
    rec, now = tolerance.load(), tolerance.measure()
    assert rec["factor"] == 8 and all(rec["bound"][k] == 8 * rec["disagreement"][k] for k in tolerance.KEYS)
    assert all(0 < now["disagreement"][k] <= rec["bound"][k] for k in tolerance.KEYS)
    assert all(now["truth_distance"][k] <= 2 * rec["truth_distance"][k] for k in tolerance.KEYS)
    assert now["evaluations"] == rec["evaluations"] and sorted(rec["evaluations"]) == sorted(sc.NAMES)
    assert rec["evaluation_cap"] == ref.MAX_EVALUATIONS and max(rec["evaluations"].values()) < rec["evaluation_cap"] / 2


def test_scipy_reaches_the_same_minimum():
    """a dense least_squares over the rig and the five poses of one noisy case, started at the restatement's start, ends
    where the restatement ends, within the measured bound"""
    optimize = pytest.importorskip("scipy.optimize")
    rec = tolerance.load()
    c, want = tolerance.solved("f5-n70", True)
    cams = (c["K1"], c["D1"], c["K2"], c["D2"])
    _, T1s, _ = ref.start(c["obj"], c["uv1"], c["uv2"], cams)
    base = [(want["R0"], want["t0"])] + [(T[:3, :3], T[:3, 3]) for T in T1s]

    def poses(x):
        return [(pc_rotate(x[6 * i:6 * i + 3], R), t + x[6 * i + 3:6 * i + 6]) for i, (R, t) in enumerate(base)]

    def fun(x):
        (R, t), frames = poses(x)[0], poses(x)[1:]
        return np.concatenate([ref.residuals(Ri, ti, R, t, o, a, b, cams) for (Ri, ti), o, a, b in zip(frames, c["obj"], c["uv1"], c["uv2"])])

    from pnp_ref import rotate_left as pc_rotate
    x = np.zeros(6 * len(base))
    for _ in range(3):  # re-centred twice: the last rounds start next to the minimum, where 3-point differences are exact enough
        x = optimize.least_squares(fun, x, jac="3-point", method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0).x
        base, x = poses(x), np.zeros_like(x)
    got = dict(R=base[0][0], t=base[0][1].reshape(3, 1), T=np.stack([np.vstack([np.c_[R, t], [0, 0, 0, 1]]) for R, t in base[1:]]),
               status=want["status"])
    rr = fun(x).reshape(len(c["obj"]), -1)
    got["retval"] = float(np.sqrt((rr * rr).sum() / (2 * sum(c["counts"]))))
    got["reprojection_error"] = np.sqrt((rr * rr).sum(1) / (2 * np.array(c["counts"])))
    d = tolerance.difference(got, want)
    print("|scipy - restatement| %s" % d)
    assert all(d[k] <= rec["bound"][k] for k in tolerance.KEYS), d


def test_refusals_come_before_the_device(no_device):
    obj, uv = np.zeros((3, 70, 3)), np.zeros((3, 70, 2))
    obj[:] = pc.board_points(70)
    K = pc.camera(0)[0]
    fix, guess = ca.CALIB_FIX_INTRINSIC, ca.CALIB_FIX_INTRINSIC | ca.CALIB_USE_EXTRINSIC_GUESS
    ok = dict(object_points=obj, image_points1=uv, image_points2=uv, K1=K, D1=None, K2=K, D2=np.zeros(5))
    bad = [
        (dict(object_points=obj[..., :2]), ValueError, "object_points must be"),
        (dict(image_points1=uv[:, :60], image_points2=uv[:, :60]), ValueError, "object_points must be"),
        (dict(object_points=obj.astype(np.float16)), ValueError, "float32 or float64"),
        (dict(image_points2=uv.astype(np.int32)), ValueError, "float32 or float64"),
        (dict(image_points1=list(uv)), TypeError, "NumPy array or a torch CUDA tensor"),
        (dict(image_points2=uv[:, :60]), ValueError, "must agree in shape, dtype and kind"),
        (dict(image_points2=uv.astype(np.float32)), ValueError, "must agree in shape, dtype and kind"),
        (dict(object_points=obj[0], image_points1=uv[0], image_points2=uv[0]), ValueError, "unless counts is given"),
        (dict(object_points=obj.reshape(-1, 3), image_points1=uv.reshape(-1, 2), image_points2=uv.reshape(-1, 2), counts=[70, 60, 70]),
         ValueError, "counts sum"),
        (dict(flags=0), ValueError, "CALIB_FIX_INTRINSIC is required"),
        (dict(flags=ca.CALIB_USE_EXTRINSIC_GUESS), ValueError, "CALIB_FIX_INTRINSIC is required"),
        (dict(flags=fix | ca.CALIB_USE_INTRINSIC_GUESS), ValueError, "flags 0x1 are not implemented"),
        (dict(flags=fix | 0x200), ValueError, "not implemented"),  # CALIB_SAME_FOCAL_LENGTH
        (dict(flags=guess), ValueError, "needs R and t"),
        (dict(flags=guess, R=np.eye(3)), ValueError, "needs R and t"),
        (dict(flags=guess, R=np.eye(4), t=np.zeros(3)), ValueError, "R must be"),
        (dict(flags=guess, R=np.eye(3), t=np.full(3, np.nan)), ValueError, "R must be"),
        (dict(K1=np.eye(4)), ValueError, "K1 must be"),
        (dict(K2=np.full((3, 3), np.inf)), ValueError, "K2 must be"),
        (dict(D1=np.zeros(6)), ValueError, "D1 must hold"),
        (dict(D2=np.r_[np.zeros(12), 0.1, 0.0]), ValueError, "tilted"),
        (dict(object_points=obj[:, :3], image_points1=uv[:, :3], image_points2=uv[:, :3]), ValueError, "fewer than 4 points"),
        (dict(object_points=pc.cloud_points(5), image_points1=uv[:, :5], image_points2=uv[:, :5]), ValueError, "fewer than 6 points"),
    ]
    for change, exc, text in bad:
        with pytest.raises(exc, match=text):
            module.stereo_calibrate(**dict(ok, **change))


def test_stereo_without_common_detections_still_raises(no_device):
    """cameras without detections, and cameras that share no key: the NotImplementedError this package has always raised,
    before anything touches the device or the library; R=, t= still builds the rig"""
    K = pc.camera(0)[0]
    xy = (pc.W, pc.H)
    plain1, plain2 = ca.Cam(K, None, xy), ca.Cam(K, None, xy)
    with pytest.raises(NotImplementedError, match="R= and t="):
        ca.Stereo(plain1, plain2)
    board, uv = pc.board_points(12), np.arange(24.0).reshape(12, 2)
    cam1 = ca.Cam.from_detections({"a": dict(image_points=uv, object_points=board)}, xy)
    cam2 = ca.Cam.from_detections({"b": dict(image_points=uv, object_points=board),
                                   "a": dict(image_points=np.zeros((0, 2)), object_points=board)}, xy)
    cam1.K = cam2.K = K
    cam1.D = cam2.D = np.zeros((1, 5))
    for pair in ((cam1, cam2), (cam1, plain2), (plain1, cam2)):
        with pytest.raises(NotImplementedError, match="carry detections"):
            ca.Stereo(*pair)
    m1 = ca.Cam.from_detections({"a": dict(image_points={1: uv[:4]}, object_points={1: board[:4]})}, xy)
    m2 = ca.Cam.from_detections({"a": dict(image_points={2: uv[:4]}, object_points={2: board[:4]})}, xy)
    with pytest.raises(NotImplementedError):
        ca.Stereo(m1, m2)  # a common key without a common id
    s = ca.Stereo(plain1, plain2, R=np.eye(3), t=[-0.1, 0, 0])
    assert s.t.shape == (3, 1) and s.get_conjoint_points() == ([], [], [])


def _frames(fx, prefix):
    out = {}
    for key in fx[prefix + "/keys"]:
        d = {}
        for what in ("image_points", "object_points"):
            base = "%s/%s/%s" % (prefix, key, what)
            if base in fx:
                d[what] = fx[base]
            elif base + "/ids" in fx:
                d[what] = {int(i): fx["%s/%d" % (base, i)] for i in fx[base + "/ids"]}
        out[str(key)] = d
    return out


@pytest.mark.parametrize("name", ["arrays", "markers"])
def test_conjoint_points_equal_the_references(name):
    fx = np.load(GOLDEN)
    s = ca.Stereo()
    s.cam1, s.cam2 = ca.Cam(), ca.Cam()
    s.cam1.update(_frames(fx, name + "/cam1")), s.cam2.update(_frames(fx, name + "/cam2"))
    got = s.get_conjoint_points()
    n = int(fx[name + "/frames"])
    assert n >= 2 and all(len(g) == n for g in got)
    for which, arrays in zip(("image_points1", "image_points2", "object_points"), got):
        for i, a in enumerate(arrays):
            assert np.array_equal(a, fx["%s/out/%s/%d" % (name, which, i)]), (which, i)


def test_the_rig_is_wired_to_the_solver(monkeypatch):
    seen = {}

    def solver(object_points, image_points1, image_points2, K1, D1, K2, D2, counts=None, flags=0, R=None, t=None):
        seen.update(obj=object_points, uv1=image_points1, uv2=image_points2, counts=list(counts), flags=flags, K2=K2)
        return dict(retval=0.25, R=np.eye(3), t=np.array([[-0.1], [0.0], [0.0]]))
    monkeypatch.setattr(module, "stereo_calibrate", solver)
    c = sc.case("markers", seed=sc.SEED)
    full = sc.case("f5-n70", seed=sc.SEED)
    frames1, frames2 = sc.marker_frames(full["obj"], full["uv1"], full["uv2"])
    xy = (sc.W, sc.H)
    cam1, cam2 = ca.Cam.from_detections(frames1, xy), ca.Cam.from_detections(frames2, xy)
    cam1.K, cam1.D, cam2.K, cam2.D = c["K1"], c["D1"].reshape(1, -1), c["K2"], c["D2"].reshape(1, -1)
    s = ca.Stereo(cam1, cam2)
    assert seen["counts"] == c["counts"] and seen["flags"] == ca.CALIB_FIX_INTRINSIC and seen["K2"] is cam2.K
    assert np.array_equal(seen["uv2"], np.concatenate(c["uv2"])) and np.array_equal(seen["obj"], np.concatenate(c["obj"]))
    assert s.retval == 0.25 and s.t.shape == (3, 1) and s.dump(return_dict=True)["retval"] == 0.25 and tuple(s.xy) == xy


def test_exports_and_the_binding():
    import re
    assert all(n in ca.__all__ for n in ("stereo_calibrate", "CALIB_FIX_INTRINSIC", "CALIB_USE_EXTRINSIC_GUESS"))
    assert ca.stereo_calibrate is module.stereo_calibrate
    assert (ca.CALIB_FIX_INTRINSIC, ca.CALIB_USE_EXTRINSIC_GUESS) == (256, 1 << 22)  # cv2's values
    assert (module.CALIB_FIX_INTRINSIC, module.CALIB_USE_EXTRINSIC_GUESS) == (ref.FIX_INTRINSIC, ref.USE_EXTRINSIC_GUESS)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "calibrating_amd.h")).read()
    values = {k: int(v) for k, v in re.findall(r"(CAMD_STEREO_[A-Z_]+)\s*=?\s+(\d+)", src)}
    assert len(values) == 17
    for name, value in values.items():
        assert getattr(_native, name[len("CAMD_"):]) == value, name
    assert _native.STEREO_STATE_DOUBLES <= _native.CALIB_STATE_DOUBLES  # camd_calib_read reads it


def test_the_entry_points_check_before_they_probe():
    """null and malformed problems are CAMD_ERR_BAD_ARG with a text; a formed one (made-up device addresses, never read)
    reaches the device probe; an empty one launches nothing"""
    import ctypes
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the formed calls must not reach a kernel")
    lib = _native.lib()
    A = lambda k: 0x7000000000 + (k << 20)  # noqa: E731
    K, D = np.eye(3).ravel(), np.zeros(5)
    p1 = _native.PnpPoints(A(0), A(1), A(2), 10, 10, _native.VALUE_F64, _native.VALUE_F32, 3, 2, 0, 2)
    p2 = _native.PnpPoints(A(0), A(8), A(2), 10, 10, _native.VALUE_F64, _native.VALUE_F32, 3, 2, 0, 2)

    def rig(**change):
        kw = dict(points1=p1, points2=p2, K1=K.ctypes.data, dist1=D.ctypes.data, K2=K.ctypes.data, dist2=None, used=A(3), state=A(4),
                  poses=A(5), candidate=A(6), workspace=A(7), partials=A(9), frame_error=A(10), ndist1=5, ndist2=0, used_n=2, reserved=0)
        kw.update(change)
        return ctypes.byref(_native.StereoRig(**kw))
    NO, BAD, OK = _native.CAMD_ERR_NO_DEVICE, _native.CAMD_ERR_BAD_ARG, _native.CAMD_OK
    other = _native.PnpPoints(A(0), A(8), A(2), 10, 12, _native.VALUE_F64, _native.VALUE_F32, 3, 2, 0, 2)
    for name in ("camd_stereo_linearise", "camd_stereo_step", "camd_stereo_finish"):
        fn = getattr(lib, name)
        assert fn(None, None) == BAD and _native.last_error().startswith(name + ": bad arguments"), name
        assert fn(rig(), None) == NO, name
        assert fn(rig(used_n=0, used=None, state=None, workspace=None), None) == OK, name
        for change in (dict(used_n=-1), dict(used=None), dict(used=A(3) + 2), dict(state=None), dict(workspace=None), dict(points2=other),
                       dict(ndist1=6), dict(ndist2=5), dict(K1=None)):
            assert fn(rig(**change), None) == BAD, (name, change)
    assert lib.camd_stereo_linearise(rig(poses=None), None) == BAD and lib.camd_stereo_linearise(rig(partials=None), None) == NO
    assert lib.camd_stereo_step(rig(candidate=None), None) == BAD and lib.camd_stereo_step(rig(partials=None), None) == BAD
    assert lib.camd_stereo_finish(rig(frame_error=None), None) == BAD and lib.camd_stereo_finish(rig(poses=None), None) == NO
