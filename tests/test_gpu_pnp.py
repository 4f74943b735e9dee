"""Batched PnP on the MI355X (-m gpu): ``pnp.solve_pnp_batch`` and the ``Cam`` methods over it, against the truth of the
synthetic cases (tests/pnp_cases.py), against the NumPy restatement tests/pnp_ref.py within the measured summation-order
bound of tests/golden/pnp_tolerance.json, and against themselves bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import geometry, pnp  # noqa: E402

import pnp_cases as pc  # noqa: E402
import pnp_ref as ref  # noqa: E402
import pnp_tolerance  # noqa: E402

KEYS = ("T", "reprojection_error", "iterations", "status")


def host(r):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    a, b = host(a), host(b)
    return all(np.array_equal(a[k][rows_a], b[k][rows_b], equal_nan=True) for k in KEYS)


def starts(c):
    return np.stack([pc.perturbed(T, i) for i, T in enumerate(c["T"])])


@pytest.mark.parametrize("i", range(len(pc.GRID)))
def test_noise_free_poses_to_nine_decimals(i):
    kind, n, ndist = pc.GRID[i]
    frames = pc.FRAME_COUNTS[i % len(pc.FRAME_COUNTS)]
    c = pc.case(kind, n, frames, ndist)
    for T0 in (None, starts(c)):
        r = pnp.solve_pnp_batch(c["obj"], c["uv"], c["K"], c["D"], T0=T0)
        assert all(isinstance(r[k], np.ndarray) for k in KEYS) and r["T"].shape == (frames, 4, 4) and r["T"].dtype == np.float64
        assert (r["status"] == 0).all() and (r["iterations"] <= 100).all(), (r["status"], r["iterations"])
        np.testing.assert_almost_equal(r["T"], c["T"], 9)
        assert (r["reprojection_error"] < 1e-9).all()
        t = pnp.solve_pnp_batch(torch.from_numpy(c["obj"]).cuda(), torch.from_numpy(c["uv"]).cuda(), c["K"], c["D"], T0=T0)
        assert all(isinstance(t[k], torch.Tensor) and t[k].is_cuda for k in KEYS) and same_bits(t, r)


@pytest.mark.parametrize("frames", pc.FRAME_COUNTS)
@pytest.mark.parametrize("kind", ["board", "cloud"])
def test_every_frame_count_and_float32_rows(kind, frames):
    """float32 object rows are the data here: the truth is projected from their values.  float32 image rows are checked
    against the float64 copy of the same values (the same bits), and against the truth on cases built from float32 pixels
    (pnp_cases.case_from_pixels), as ndarrays and as CUDA tensors, with and without a start."""
    c = pc.case(kind, 65, frames, 8)
    obj32 = c["obj"].astype(np.float32)
    uv = np.stack([pc.observe(obj32.astype(np.float64), T, c["K"], c["D"]) for T in c["T"]])
    per_frame = np.repeat(obj32[None], frames, 0)
    for o in (obj32, per_frame, torch.from_numpy(per_frame).cuda()):
        u = torch.from_numpy(uv).cuda() if isinstance(o, torch.Tensor) else uv
        for T0 in (None, starts(c)):
            r = host(pnp.solve_pnp_batch(o, u, c["K"], c["D"], T0=T0))
            assert (r["status"] == 0).all()
            np.testing.assert_almost_equal(r["T"], c["T"], 9)
    p = pc.case_from_pixels(kind, 65, frames, 8)
    for T0 in (None, starts(p)):
        for o, u in ((p["obj"], p["uv"]), (torch.from_numpy(p["obj"]).cuda(), torch.from_numpy(p["uv"]).cuda())):
            r = host(pnp.solve_pnp_batch(o, u, p["K"], p["D"], T0=T0))
            assert (r["status"] == 0).all() and (r["reprojection_error"] < 1e-9).all()
            np.testing.assert_almost_equal(r["T"], p["T"], 9)
    uv32 = uv.astype(np.float32)
    for T0 in (None, starts(c)):
        assert same_bits(pnp.solve_pnp_batch(obj32, uv32, c["K"], c["D"], T0=T0),
                         pnp.solve_pnp_batch(obj32.astype(np.float64), uv32.astype(np.float64), c["K"], c["D"], T0=T0))


@pytest.fixture(scope="module")
def noisy():
    return pnp_tolerance.noisy_cases(), pnp_tolerance.load()


def test_noisy_poses_agree_with_the_restatement(noisy):
    """pose and RMS from the same start; the bound is 8 x the restatement's own forward / reversed disagreement"""
    cases, tol = noisy
    worst_T = worst_rms = 0.0
    for name, c, T0 in cases:
        r = pnp.solve_pnp_batch(c["obj"], c["uv"], c["K"], c["D"], T0=T0)
        assert (r["status"] == 0).all(), name
        for f, uv in enumerate(c["uv"]):
            w = ref.refine(c["obj"], uv, c["K"], c["D"], T0[f])
            worst_T = max(worst_T, np.abs(r["T"][f] - w["T"]).max())
            worst_rms = max(worst_rms, abs(r["reprojection_error"][f] - w["reprojection_error"]))
    print("largest |T - restatement| %.3e (bound %.3e), RMS %.3e (bound %.3e)" % (worst_T, tol["T_bound"], worst_rms, tol["rms_bound"]))
    assert worst_T <= tol["T_bound"] and worst_rms <= tol["rms_bound"]


def test_scipy_cannot_lower_the_cost(noisy):
    optimize = pytest.importorskip("scipy.optimize")
    cases, tol = noisy
    worst = 0.0
    for name, c, T0 in cases:
        r = pnp.solve_pnp_batch(c["obj"], c["uv"], c["K"], c["D"], T0=T0)
        for f, uv in enumerate(c["uv"]):
            T = r["T"][f]
            fun = lambda d: ref.residuals(ref.rotate_left(d[:3], T[:3, :3]), T[:3, 3] + d[3:], c["obj"], uv, c["K"], c["D"]).reshape(-1)  # noqa: E731
            cost = (fun(np.zeros(6)) ** 2).sum()
            best = optimize.least_squares(fun, np.zeros(6), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
            margin = 2 * tol["rms_bound"] / r["reprojection_error"][f]  # cost = 2n rms^2: twice the RMS bound's relative size
            worst = max(worst, (cost - 2 * best.cost) / cost / margin)
            assert 2 * best.cost >= cost * (1 - margin), (name, f, cost, 2 * best.cost)
    print("largest share of the margin SciPy gained: %.3f" % worst)


def test_a_frame_gets_the_same_bits_alone_and_anywhere_in_a_batch():
    c = pc.case("board", 70, 5, 5, sigma=pc.NOISE_SIGMA, seed=3)
    whole = pnp.solve_pnp_batch(c["obj"], c["uv"], c["K"], c["D"])
    assert same_bits(whole, pnp.solve_pnp_batch(c["obj"], c["uv"], c["K"], c["D"]))      # two runs
    for f in range(5):                                                                    # a loop of single calls
        assert same_bits(pnp.solve_pnp_batch(c["obj"], c["uv"][f:f + 1], c["K"], c["D"]), whole, rows_b=slice(f, f + 1)), f
    order = [3, 0, 4, 2, 1, 3, 3, 0, 1]                                                   # other places, other workgroups
    moved = pnp.solve_pnp_batch(c["obj"], c["uv"][order], c["K"], c["D"])
    for at, f in enumerate(order):
        assert same_bits(moved, whole, slice(at, at + 1), slice(f, f + 1)), (at, f)
    cloud = pc.case("cloud", 130, 4, 12, sigma=pc.NOISE_SIGMA, seed=4)
    T0 = starts(cloud)
    whole = pnp.solve_pnp_batch(cloud["obj"], cloud["uv"], cloud["K"], cloud["D"], T0=T0)
    for f in range(4):
        alone = pnp.solve_pnp_batch(cloud["obj"], cloud["uv"][f:f + 1], cloud["K"], cloud["D"], T0=T0[f])
        assert same_bits(alone, whole, rows_b=slice(f, f + 1)), f


def ragged(frames, K, D, **kw):
    """[(obj (n, 3), uv (n, 2))] -> one call with counts"""
    return pnp.solve_pnp_batch(np.concatenate([o for o, _ in frames]), np.concatenate([u for _, u in frames]), K, D,
                               counts=[len(o) for o, _ in frames], **kw)


def test_a_ragged_batch_of_4_and_130_point_frames():
    K, D = pc.camera(5)
    small, large = pc.centred(pc.board_points(4)), pc.centred(pc.board_points(130))
    Ts = pc.poses(4, seed=9)
    frames = [(o, pc.observe(o, T, K, D, pc.NOISE_SIGMA, seed=i)) for i, (o, T) in enumerate(zip((small, large, large, small), Ts))]
    whole = ragged(frames, K, D)
    assert (whole["status"] == 0).all() and (whole["reprojection_error"] < 3 * pc.NOISE_SIGMA).all()
    for f, fr in enumerate(frames):
        assert same_bits(ragged([fr], K, D), whole, rows_b=slice(f, f + 1)), f


def test_degenerate_frames_inside_a_good_batch():
    c = pc.case("board", 70, 2, 5, sigma=pc.NOISE_SIGMA, seed=6)
    K, D, obj = c["K"], c["D"], c["obj"]
    line = obj[:10] * [1, 0, 0]
    nan_uv = c["uv"][1].copy()
    nan_uv[33, 0] = np.nan
    frames = [(obj, c["uv"][0]), (line, pc.observe(line, c["T"][0], K, D)), (obj[:3], c["uv"][0][:3]), (obj, nan_uv), (obj, c["uv"][1])]
    for T0 in (None, np.stack([c["T"][0]] * 4 + [c["T"][1]])):
        r = ragged(frames, K, D, T0=T0)
        assert list(r["status"]) == [0, pnp.STATUS_SINGULAR, pnp.STATUS_FEW_POINTS, pnp.STATUS_NONFINITE, 0]
        assert (r["iterations"] <= 100).all() and r["iterations"][2] == 0 and r["iterations"][3] == 0
        assert np.isnan(r["T"][1:4, :3]).all() and np.isnan(r["reprojection_error"][1:4]).all()  # R and t: the rows above 0 0 0 1
        for f in (0, 4):
            alone = ragged([frames[f]], K, D, T0=None if T0 is None else T0[f])
            assert same_bits(alone, r, rows_b=slice(f, f + 1)), f
    cam = ca.Cam(K, D, (pc.W, pc.H))
    with pytest.raises(ValueError, match="status 3"):
        cam.perspective_n_point(frames[1][1], frames[1][0])
    with pytest.raises(ValueError, match="status 2"):
        cam.perspective_n_point(nan_uv, obj)


def test_cuda_points_are_refused_before_a_launch():
    few = torch.zeros((2, 3, 3), dtype=torch.float64).cuda()
    with pytest.raises(ValueError, match="fewer than 4 points"):
        pnp.solve_pnp_batch(few, few[..., :2], pc.camera(0)[0])
    cloud = torch.from_numpy(pc.cloud_points(5)).cuda()
    with pytest.raises(ValueError, match="fewer than 6 points"):
        pnp.solve_pnp_batch(cloud, torch.zeros((2, 5, 2), dtype=torch.float64).cuda(), pc.camera(0)[0])


def test_perspective_n_point_takes_arrays_and_id_dicts():
    c = pc.case("board", 70, 1, 5)
    cam = ca.Cam(c["K"], c["D"], (pc.W, pc.H))
    got = cam.perspective_n_point(c["uv"][0], c["obj"])
    assert sorted(got) == ["T", "reprojection_error", "retval"] and got["retval"] == 1
    np.testing.assert_almost_equal(got["T"], c["T"][0], 9)
    ids = {7: slice(0, 30), 2: slice(30, 50), 40: slice(50, 70)}  # joined in sorted-key order: 2, 7, 40
    by_id = cam.perspective_n_point({k: c["uv"][0][s] for k, s in ids.items()}, {k: c["obj"][s] for k, s in ids.items()})
    order = np.r_[30:50, 0:30, 50:70]
    want = cam.perspective_n_point(c["uv"][0][order][:, None], c["obj"][order])
    assert np.array_equal(by_id["T"], want["T"]) and by_id["reprojection_error"] == want["reprojection_error"]
    batch = cam.perspective_n_point_batch(c["uv"], c["obj"])
    assert np.array_equal(batch["T"][0], got["T"])


def test_solve_poses_makes_the_rig_and_T_none_resolves_through_it():
    xy = (320, 180)
    K1 = np.array([[250.0, 0, 161.5], [0, 251.0, 88.0], [0, 0, 1]])
    K2 = np.array([[240.0, 0, 158.0], [0, 242.0, 91.5], [0, 0, 1]])
    cam1, cam2 = ca.Cam(K1, np.array([[0.05, -0.02, 1e-3, -1e-3, 0.0]]), xy, "a"), ca.Cam(K2, None, xy, "b")
    rig = np.eye(4)  # camera 2 in camera 1
    rig[:3, :3] = geometry.rodrigues(np.array([0.02, -0.15, 0.01]))
    rig[:3, 3] = [-0.06, 0.004, 0.01]
    board = pc.centred(pc.board_points(70))
    rng = np.random.default_rng(77)
    for i in range(5):
        T2 = np.eye(4)
        T2[:3, :3] = geometry.rodrigues(rng.uniform(-0.3, 0.3, 3))
        T2[:3, 3] = [rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02), rng.uniform(0.4, 0.7)]
        T1 = rig @ T2
        cam1["f%d" % i] = dict(image_points=pc.observe(board, T1, cam1.K, cam1.D), object_points=board)
        # camera 2 stores the reference's id -> points dicts
        uv2 = pc.observe(board, T2, cam2.K, None)
        cam2["f%d" % i] = dict(image_points={5: uv2[:35], 9: uv2[35:]}, object_points={5: board[:35], 9: board[35:]})
    cam1["only_here"] = dict(image_points=np.zeros((0, 2)), object_points=board)  # not a valid key: no points
    cam1["seen_only"] = dict(image_points=np.ones((4, 2)))                       # valid, but nothing to solve it with
    with pytest.raises(NotImplementedError):
        cam1.project_cam2_depth(cam2, np.ones(xy[::-1]))
    assert cam1.solve_poses() == {"f%d" % i: 0 for i in range(5)} and set(cam2.solve_poses().values()) == {0}
    assert cam1.valid_keys_intersection(cam2) == ["f%d" % i for i in range(5)] and "T" not in cam1["seen_only"]
    assert all(cam1[k]["reprojection_error"] < 1e-9 for k in cam1.valid_keys_intersection(cam2))
    T = cam1.get_T_cam2_in_self(cam2)
    np.testing.assert_almost_equal(T, geometry.R_t_to_T(rig[:3, :3], rig[:3, 3]), 9)  # both through R_t_to_T's float32 rotation
    depth2 = 0.8 + 0.3 * np.random.default_rng(78).random(xy[::-1])
    a, b = cam1.project_cam2_depth(cam2, depth2), cam1.project_cam2_depth(cam2, depth2, T=T)
    assert (a > 0).any() and np.array_equal(a, b)
    img2 = np.random.default_rng(79).integers(0, 255, xy[::-1] + (3,), dtype=np.uint8)
    assert np.array_equal(cam1.reproject_img(cam2, depth2, img2), cam1.reproject_img(cam2, depth2, img2, T=T))
