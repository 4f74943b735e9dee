"""The exact fixture of the start stage and its bounds, without a GPU: tests/golden/pnp_start_exact.npz is what
tests/pnp_start_cases.py generates, every case is conditioned well enough to test a kernel, the lens cases would notice an
undistortion that stops early, and tests/golden/pnp_start_tolerance.json is the restatement's own error against the
fixture -- nothing a kernel gave."""
import numpy as np
import pytest

import calibrate_ref
import pnp_ref as ref
import pnp_start_cases as cases
import pnp_start_tolerance as tolerance
import points_ref


@pytest.fixture(scope="module")
def fixture():
    return tolerance.fixture()


def test_fixture_holds_the_cases_of_the_generator(fixture):
    """the rows in the file are the generator's (to the rounding of another machine's libm: the exact answers belong to the
    STORED rows, which is why they are stored), within the limits of the issue: at most 9 frames and 130 points"""
    assert list(fixture) == cases.NAMES
    for name, c in fixture.items():
        g = cases.case(name)
        frames, n = c["uv"].shape[:2]
        assert frames <= 9 and n <= 130 and c["obj"].shape == (n, 3), name
        for k in cases.INPUT_KEYS:
            assert c[k].shape == g[k].shape, (name, k)
            np.testing.assert_allclose(c[k], g[k], rtol=1e-6, atol=1e-9, err_msg="%s %s" % (name, k))
        assert np.isfinite(c["G"]).all() and np.isfinite(c["eigen"]).all(), name
        assert np.isfinite(c["pose"]).all() == (c["kind"] != "homography"), name
        np.testing.assert_allclose((c["G"] ** 2).sum(1), 1, rtol=1e-15)
        assert (np.take_along_axis(c["G"], np.abs(c["G"]).argmax(1)[:, None], 1) > 0).all(), name
    counts = {kind: sorted({c["uv"].shape[1] for c in fixture.values() if c["kind"] == kind}) for kind in ("planar", "cloud", "homography")}
    assert set(counts["planar"]) >= {4, 5, 63, 64, 65, 128, 129} and set(counts["cloud"]) >= {6, 7, 63, 64, 65, 128, 129}
    assert set(counts["homography"]) >= {4, 5, 63, 64, 65, 128, 129}
    for kind in ("planar", "cloud"):
        assert {c["uv"].shape[0] for c in fixture.values() if c["kind"] == kind} >= {1, 3, 4, 5, 9}
        assert {len(c["D"]) for c in fixture.values() if c["kind"] == kind} == {0, 4, 5, 8, 12, 14}


def test_the_exact_pose_of_noise_free_pinhole_frames_is_the_truth(fixture):
    """without a lens and without noise the null vector is the true H or P: the exact reference against the generator"""
    for name in ("planar-n4-f9-d0", "planar-behind-n12-f4-d0", "cloud-n6-f9-d0", "cloud-behind-n16-f4-d0"):
        T = cases.case(name)["T"]
        want = np.concatenate([T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]], 1)
        np.testing.assert_allclose(fixture[name]["pose"], want, rtol=0, atol=1e-9, err_msg=name)


def test_the_off_origin_cases_need_the_centre_term(fixture):
    """the object origin is behind the camera (t_z < 0) while every point is in front of it: the sign of H[8] or P[11]
    alone would turn the pose round"""
    for name in cases.OFF_ORIGIN:
        c = fixture[name]
        if c["kind"] == "homography":
            continue
        for pose in c["pose"]:
            R, t = pose[:9].reshape(3, 3), pose[9:]
            assert t[2] < -0.05 and ((c["obj"] @ R.T + t)[:, 2] > 0.3).all(), name
            assert abs(np.linalg.det(R) - 1) < 1e-14, name


def test_kappa_stays_under_the_cap(fixture):
    """kappa = trace M / (lambda2 - lambda1) from the exact fixture; under the cap every bound is below 1e-9 in absolute
    terms, and the restatement with the kernel's null vector is within 1e-9 of the exact pose"""
    rec = tolerance.load()
    assert rec["kappa_cap"] == tolerance.KAPPA_CAP
    assert all(b * tolerance.ULP * tolerance.KAPPA_CAP <= tolerance.POSE_ACCURACY for b in rec["bound"].values()), rec["bound"]
    for name, c in fixture.items():
        # (four points on a plane fit exactly: lambda1 is 0 to the 60 digits of the reference)
        assert (c["eigen"][:, 0] > -1e-50 * c["eigen"][:, 2]).all() and (c["eigen"][:, 1] > c["eigen"][:, 0]).all(), name
        assert (c["kappa"] < tolerance.KAPPA_CAP).all(), (name, c["kappa"])
        _, pose = tolerance.restated(c)
        if pose is not None:
            assert np.abs(pose - c["pose"]).max() < tolerance.POSE_ACCURACY, name


def test_the_tenth_undistortion_round_still_moves_the_points(fixture):
    """in every case with a lens the tenth round moves some point by more than 1 ulp of its coordinate, and the fifth
    (cv2's count) by far more than the bound: a kernel that stops early does not give the exact answer"""
    seen = set()
    for name, c in fixture.items():
        if len(c["D"]) == 0:
            continue
        seen.add(len(c["D"]))
        uv = c["uv"].reshape(-1, 2)
        x9, x10 = (points_ref.undistort_trace(uv, c["K"], c["D"], iters=i)[0] for i in (9, 10))
        moved = np.abs(x10 - x9) / np.spacing(np.abs(x10))
        print("%-34s the tenth round moves a point by up to %.3g ulp" % (name, moved.max()))
        assert moved.max() > 1, name
        x5 = points_ref.undistort_trace(uv, c["K"], c["D"], iters=5)[0]
        assert np.abs(x10 - x5).max() > 1e3 * tolerance.load()["bound"]["pose"] * tolerance.ULP * c["kappa"].max(), name
    assert seen == {4, 5, 8, 12, 14}


def test_tolerance_file_is_the_measurement():
    """the bounds are 8 x the restatement's own error against the exact fixture, in units of 2^-52 kappa, forward and
    reversed -- never what a kernel gives"""
    rec, now = tolerance.load(), tolerance.measure()
    assert rec["factor"] == 8 and rec["ulp"] == tolerance.ULP and set(rec["bound"]) == set(tolerance.QUANTITIES)
    for k in tolerance.QUANTITIES:
        assert rec["bound"][k] == 8 * rec["measured"][k] and 0 < now["measured"][k] <= rec["bound"][k], (k, now["measured"][k], rec["bound"][k])
    assert set(rec["cases"]) == set(cases.NAMES)


def test_the_restatement_lies_within_the_bound(fixture):
    """``pnp_ref.init_pose(..., null="kernel")`` and ``calibrate_ref.homography`` against the exact fixture"""
    bound = tolerance.load()["bound"]
    for name, c in fixture.items():
        D = c["D"] if len(c["D"]) else None
        if c["kind"] == "homography":
            G = np.stack([calibrate_ref.homography(c["obj"], uv, c["plane"]).reshape(-1) for uv in c["uv"]])
            e = tolerance.case_errors(c, G, K0=calibrate_ref.initial_camera_matrix(G.reshape(-1, 3, 3), tolerance.XY))
        else:
            T = [ref.init_pose(c["obj"], uv, c["K"], D, c["kind"] == "planar", c["plane"], null="kernel") for uv in c["uv"]]
            e = dict(pose=tolerance.pose_error(np.stack([np.concatenate([t[:3, :3].reshape(-1), t[:3, 3]]) for t in T]), c).max())
        for k, v in e.items():
            assert v <= bound[k], (name, k, v, bound[k])


def test_the_comparison_notices_each_defect_the_refinement_hides(fixture):
    """the restatement with one line changed lands outside the bound: five undistortion rounds, a transposed plane; and on
    the off-origin boards the sign of H[8] alone disagrees with the sign test that has its centre term"""
    bound = tolerance.load()["bound"]

    def worst(pose_of, names):
        return max(tolerance.pose_error(np.stack([pose_of(fixture[n], uv) for uv in fixture[n]["uv"]]), fixture[n]).max() for n in names)

    def flat(T):
        return np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]])

    def lens(c):
        return c["D"] if len(c["D"]) else None

    def early_stop(c, uv):
        xy = points_ref.undistort_trace(uv, c["K"], lens(c), iters=5)[0]
        return flat(ref.init_pose(c["obj"], xy, np.eye(3), None, c["kind"] == "planar", c["plane"], "kernel"))

    def transposed(c, uv):
        return flat(ref.init_pose(c["obj"], uv, c["K"], lens(c), True, c["plane"].T, "kernel"))

    assert worst(early_stop, ["planar-n65-f4-d12-noisy", "cloud-n7-f5-d4-noisy"]) > bound["pose"]
    assert worst(transposed, ["planar-tilted-n24-f3-d8-noisy"]) > bound["pose"]
    for name in ("planar-behind-n12-f4-d0", "planar-behind-n12-f4-d5-noisy"):
        c = fixture[name]
        for uv, pose in zip(c["uv"], c["pose"]):
            G = ref.normalised_dlt(c["obj"][:, :2], points_ref.undistort_trace(uv, c["K"], lens(c), iters=10)[0], "kernel")
            m = c["obj"].mean(0)
            assert (G[2, 2] < 0) != (G[2, 0] * m[0] + G[2, 1] * m[1] + G[2, 2] < 0), name
