"""The host side of the batched PnP without a GPU: refusals, the reference's pose bookkeeping (``mean_Ts``,
``get_T_cam2_in_self``, the key sets) bit for bit against tests/golden/reference_pose.npz, the NumPy restatement
tests/pnp_ref.py against the truth, and the measured summation-order tolerance of tests/golden/pnp_tolerance.json."""
import os

import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import _native, geometry, pnp

import pnp_cases as pc
import pnp_ref as ref
import pnp_tolerance

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_pose.npz")
K, _ = pc.camera(0)


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


@pytest.fixture()
def no_device(monkeypatch):
    """any step towards the device fails the test"""
    def touched(*a, **k):
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(_native, "require_device", touched)
    monkeypatch.setattr(_native, "call", touched)
    monkeypatch.setattr(_native, "lib", touched)


def test_refusals_come_before_the_device(no_device):
    obj, uv = np.zeros((2, 70, 3)), np.zeros((2, 70, 2))
    obj[:] = pc.board_points(70)
    bad = [
        (dict(object_points=obj[..., :2], image_points=uv), ValueError, "object_points must be"),
        (dict(object_points=obj, image_points=uv[:, :60]), ValueError, "object_points must be"),
        (dict(object_points=obj.astype(np.float16), image_points=uv), ValueError, "float32 or float64"),
        (dict(object_points=obj, image_points=uv.astype(np.int32)), ValueError, "float32 or float64"),
        (dict(object_points=list(obj), image_points=uv), TypeError, "NumPy array or a torch CUDA tensor"),
        (dict(object_points=obj[0], image_points=uv[0]), ValueError, "unless counts is given"),
        (dict(object_points=obj.reshape(-1, 3), image_points=uv.reshape(-1, 2), counts=[70, 60]), ValueError, "counts sum"),
        (dict(object_points=obj.reshape(-1, 3), image_points=uv.reshape(-1, 2), counts=[70.0, 70.0]), ValueError, "counts must be"),
        (dict(object_points=obj, image_points=uv, D=np.zeros(3)), ValueError, "coefficients"),
        (dict(object_points=obj, image_points=uv, D=np.r_[np.zeros(12), 0.01, 0.0]), ValueError, "tilted-sensor"),
        (dict(object_points=obj, image_points=uv, T0=np.eye(3)), ValueError, "T0 must be"),
        (dict(object_points=obj[:, :3], image_points=uv[:, :3]), ValueError, "fewer than 4 points"),
        (dict(object_points=pc.cloud_points(5)[None], image_points=uv[:1, :5]), ValueError, "fewer than 6 points"),
        (dict(object_points=pc.cloud_points(3)[None], image_points=uv[:1, :3], T0=np.eye(4)), ValueError, "fewer than 4 points"),
    ]
    for kw, exc, text in bad:
        with pytest.raises(exc, match=text):
            pnp.solve_pnp_batch(K=K, **kw)
    cam = ca.Cam(K, None, (pc.W, pc.H))
    with pytest.raises(ValueError, match="fewer than 4 points"):
        cam.perspective_n_point(uv[0, :3], obj[0, :3])


def test_planarity_rule():
    assert pnp.plane_of(pc.board_points(70))[0] and not pnp.plane_of(pc.cloud_points(6))[0]
    bent = pc.board_points(70)
    bent[:, 2] = 2e-3 * np.sin(40 * bent[:, 0])  # 2 mm off a 15 cm board: above 1e-3 of the middle singular value
    assert not pnp.plane_of(bent)[0]
    planar, plane = pnp.plane_of(pc.board_points(70) @ geometry.rodrigues(np.array([0.3, -0.5, 0.2])).T + 1.0)
    z = (pc.board_points(70) @ geometry.rodrigues(np.array([0.3, -0.5, 0.2])).T + 1.0) @ plane.T
    assert planar and np.ptp(z[:, 2]) < 1e-12 and abs(np.linalg.det(plane) - 1) < 1e-12


@pytest.mark.parametrize("name", ["one", "tight", "loose", "pair"])
def test_mean_Ts_is_the_references(fx, name):
    got = geometry.mean_Ts(list(fx["mean/%s/Ts" % name]))
    assert got.dtype == np.float64 and np.array_equal(got, fx["mean/%s/T" % name])
    assert np.array_equal(ca.mean_Ts(fx["mean/%s/Ts" % name]), got)
    assert np.array_equal(got[:3, :3], got[:3, :3].astype(np.float32))  # the rotation went through float32


def test_mean_Ts_accumulates_from_the_left(fx):
    """``R_acc = (R0.T @ R) @ R_acc``: for rotations that do not commute the order shows in the result"""
    Ts = fx["mean/loose/Ts"]
    assert not np.array_equal(geometry.mean_Ts(Ts), geometry.mean_Ts(np.concatenate([Ts[:1], Ts[:0:-1]])))


def _cameras(fx):
    cam1, cam2 = ca.Cam(K, None, (pc.W, pc.H), "a"), ca.Cam(K, None, (pc.W, pc.H), "b")
    pts = np.array([[10.0, 20.0], [30.0, 40.0]])
    for k, T in zip(fx["rig/keys1"], fx["rig/T1"]):
        cam1[str(k)] = dict(image_points=pts, T=T)
    for k, T in zip(fx["rig/keys2"], fx["rig/T2"]):
        cam2[str(k)] = dict(image_points={} if k == fx["rig/empty"] else {3: pts[:1], 1: pts[1:]}, T=T)
    return cam1, cam2


def test_key_sets_and_rig_pose_are_the_references(fx):
    cam1, cam2 = _cameras(fx)
    assert sorted(cam1.valid_keys) == list(fx["rig/valid1"]) and sorted(cam2.valid_keys) == list(fx["rig/valid2"])
    assert cam1.valid_keys_intersection(cam2) == list(fx["rig/intersection"])
    assert np.array_equal(cam1.get_T_cam2_in_self(cam2), fx["rig/T_cam2_in_cam1"])


def test_points_dicts_join_in_sorted_key_order(fx):
    joined = {int(k): fx["join/in_%d" % k] for k in fx["join/keys"][::-1]}
    assert np.array_equal(geometry.join_points(joined), fx["join/out"])
    assert geometry.join_points(fx["join/out"]) is not None


def test_T_none_is_still_refused_without_poses(fx, no_device):
    msg = "pass T \\(cam2 in cam1\\): board-based extrinsics are outside the MI355X path"
    cam1, cam2 = ca.Cam(K, None, (pc.W, pc.H)), ca.Cam(K, None, (pc.W, pc.H))
    depth, img = np.ones((pc.H, pc.W)), np.zeros((pc.H, pc.W, 3), np.uint8)
    for cams in ((cam1, cam2), _cameras(fx)[:1] + (cam2,)):  # no frames at all; poses in one camera only
        with pytest.raises(NotImplementedError, match=msg):
            cams[0].project_cam2_depth(cams[1], depth)
        with pytest.raises(NotImplementedError, match=msg):
            cams[0].reproject_img(cams[1], depth, img)
        with pytest.raises(NotImplementedError, match=msg):
            cams[0].vis_reproject_img_alignment(cams[1], depth, img, img)
    a, b = _cameras(fx)
    for d in b.values():
        d.pop("T")  # common keys, but camera 2 carries no pose
    with pytest.raises(NotImplementedError, match=msg):
        a.project_cam2_depth(b, depth)
    with pytest.raises(NotImplementedError):
        ca.Stereo(cam1, cam2)


def test_jacobian_of_the_restatement_against_differences():
    c = pc.case("cloud", 65, 1, 12)
    T = pc.perturbed(c["T"][0])
    _, g, _ = ref.normal_equations(T[:3, :3], T[:3, 3], c["obj"], c["uv"][0], c["K"], c["D"])

    def cost(d):
        r = ref.residuals(ref.rotate_left(d[:3], T[:3, :3]), T[:3, 3] + d[3:], c["obj"], c["uv"][0], c["K"], c["D"])
        return (r * r).sum()
    h = 1e-6
    num = np.array([(cost(np.eye(6)[i] * h) - cost(-np.eye(6)[i] * h)) / (2 * h) for i in range(6)])
    assert np.abs(num - 2 * g).max() <= 1e-7 * np.abs(g).max()


@pytest.mark.parametrize("kind,n,ndist", pc.GRID)
def test_restatement_recovers_the_truth(kind, n, ndist):
    """the reference's own bar (example/test_occlude_marker.py:53): 9 decimals, noise-free, with and without a start"""
    c = pc.case(kind, n, 3, ndist)
    for f, (uv, T) in enumerate(zip(c["uv"], c["T"])):
        for T0 in (None, pc.perturbed(T, f)):
            r = ref.solve(c["obj"], uv, c["K"], c["D"], T0=T0)
            assert r["status"] == ref.OK and r["iterations"] <= ref.MAX_ITERATIONS
            np.testing.assert_almost_equal(r["T"], T, 9)
            assert r["reprojection_error"] < 1e-9


@pytest.mark.parametrize("sigma", [0.0, pc.NOISE_SIGMA])
def test_the_kernels_null_vector_is_the_eigenvector(sigma):
    """The start pose rests on six rounds of inverse iteration with a fixed shift instead of an eigensolver.  Each round
    shrinks what is left of the other eigenvectors by (l1 + mu) / (l2 + mu), so six rounds leave nothing above rounding
    unless the two smallest eigenvalues nearly coincide; measured here on every case of the grid: the start pose it
    gives is the eigensolver's to 1e-9 (2.4e-12 measured), and without noise it is the truth to 1e-9 (3.9e-13 measured)."""
    for kind, n, ndist in pc.GRID:
        c = pc.case(kind, n, 3, ndist, sigma=sigma, seed=5)
        planar, plane = ref.plane_of(c["obj"])
        for uv, T in zip(c["uv"], c["T"]):
            a = ref.init_pose(c["obj"], uv, c["K"], c["D"], planar, plane)
            b = ref.init_pose(c["obj"], uv, c["K"], c["D"], planar, plane, null="kernel")
            assert np.abs(a - b).max() < 1e-9, (kind, n, ndist)
            if not sigma:
                assert np.abs(b - T).max() < 1e-9, (kind, n, ndist)


@pytest.mark.parametrize("kind", ["board", "cloud"])
def test_restatement_recovers_the_truth_from_float32_pixels(kind):
    """cases whose image rows ARE float32 and still noise-free: the object points were put on the pixels' rays"""
    c = pc.case_from_pixels(kind, 65, 3, 8)
    assert c["uv"].dtype == np.float32
    for obj, uv, T in zip(c["obj"], c["uv"], c["T"]):
        r = ref.solve(obj, uv.astype(np.float64), c["K"], c["D"])
        assert r["status"] == ref.OK and r["reprojection_error"] < 1e-9
        np.testing.assert_almost_equal(r["T"], T, 9)


def test_restatement_names_degenerate_frames():
    c = pc.case("board", 70, 1, 5)
    obj, uv, T = c["obj"], c["uv"][0], c["T"][0]
    line = obj[:10] * [1, 0, 0]
    assert ref.refine(line, pc.observe(line, T, c["K"], c["D"]), c["K"], c["D"], pc.perturbed(T))["status"] == ref.SINGULAR
    assert ref.refine(obj[:3], uv[:3], c["K"], c["D"], T)["status"] == ref.FEW
    bad = uv.copy()
    bad[7, 1] = np.nan
    assert ref.refine(obj, bad, c["K"], c["D"], T)["status"] == ref.NONFINITE


def test_tolerance_file_is_the_measurement():
    """the bound comes from the restatement's own disagreement under a change of summation order, times 8 -- never from
    what the kernel gives"""
    rec, now = pnp_tolerance.load(), pnp_tolerance.measure()
    assert rec["factor"] == 8 and rec["T_bound"] == 8 * rec["T_disagreement"] and rec["rms_bound"] == 8 * rec["rms_disagreement"]
    assert 0 < now["T_disagreement"] <= rec["T_bound"] and 0 < now["rms_disagreement"] <= rec["rms_bound"]


def test_the_new_entry_points_check_before_they_probe():
    """status and message of a null call and of a formed call (made-up device addresses, never read): every argument check
    comes before the device probe, and an empty batch launches nothing"""
    import ctypes
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the formed calls must not reach a kernel")
    lib = _native.lib()
    A = lambda k: 0x7000000000 + (k << 20)  # noqa: E731
    Kf, plane = np.ascontiguousarray(K.ravel()), np.eye(3).ravel()
    pts = _native.PnpPoints(A(0), A(1), A(2), 10, 10, _native.VALUE_F64, _native.VALUE_F32, 3, 2, 0, 2)
    none = _native.PnpPoints(A(0), A(1), A(2), 10, 10, _native.VALUE_F64, _native.VALUE_F32, 3, 2, 0, 0)
    assert lib.camd_pnp_init(None, None, None, 0, 0, None, None, None) == _native.CAMD_ERR_BAD_ARG
    assert _native.last_error().startswith("camd_pnp_init: bad arguments")
    assert lib.camd_pnp_refine(None, None, None, 0, 0, None, 0, None, None, None, None, None) == _native.CAMD_ERR_BAD_ARG
    assert _native.last_error().startswith("camd_pnp_refine: bad arguments")
    assert lib.camd_pnp_init(ctypes.byref(pts), Kf.ctypes.data, None, 0, 1, plane.ctypes.data, A(3), None) == _native.CAMD_ERR_NO_DEVICE
    assert lib.camd_pnp_init(ctypes.byref(pts), Kf.ctypes.data, None, 0, 1, None, A(3), None) == _native.CAMD_ERR_BAD_ARG
    assert lib.camd_pnp_init(ctypes.byref(none), Kf.ctypes.data, None, 0, 0, None, None, None) == _native.CAMD_OK
    refine = lambda p, minimum, stride: lib.camd_pnp_refine(ctypes.byref(p), Kf.ctypes.data, None, 0, minimum, A(3), stride, A(4),  # noqa: E731
                                                            A(5), A(6), A(7), None)
    assert refine(pts, 4, 12) == _native.CAMD_ERR_NO_DEVICE
    assert refine(pts, 2, 12) == _native.CAMD_ERR_BAD_ARG and refine(pts, 4, 7) == _native.CAMD_ERR_BAD_ARG
    assert refine(none, 4, 0) == _native.CAMD_OK
