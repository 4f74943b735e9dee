"""The host side of the bundle adjustment without a GPU: the NumPy restatement tests/bundle_ref.py -- its Jacobians against
finite differences, the noise-free cases against the truth, the noisy cases against their start --, the measured
summation-order tolerance of tests/golden/bundle_tolerance.json, and every refusal of ``bundle_adjust_pairs`` before the
device."""
import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import _native, bundle

import bundle_cases as bc
import bundle_ref as ref
import bundle_tolerance as tolerance


@pytest.fixture()
def no_device(monkeypatch):
    """any step towards the device fails the test"""
    def touched(*a, **k):
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(_native, "require_device", touched)
    monkeypatch.setattr(_native, "call", touched)
    monkeypatch.setattr(_native, "lib", touched)


def test_the_jacobians_match_central_differences():
    """a view's 2 x 6 block in (w, d), the point's 2 x 3 block, and the anchor's (w, e) block through M, off the minimum;
    step and bound: the restatement's FD_STEP, FD_BOUND"""
    c = bc.case("three", bc.NOISE_SIGMA, bc.NOISY_SEED)
    R, t = ref.poses_from_T(c["T0"])
    k = ref.k4(c["K"])
    X0, status = ref.start(c["K"], R, t, c["pairs"], c["uvs_a"], c["uvs_b"], c["counts"])
    at = np.flatnonzero(status[:300] == 0)[::40]
    X, uv, h = X0[at], c["uvs_a"][at], ref.FD_STEP
    v = 1
    z, r, J, G = ref.observe(R[v], t[v], k[v], X, uv)
    assert (z > 0).all()

    def residual(x, dX=np.zeros(3)):
        return ref.observe(ref.rotate_left(x[:3], R[v]), t[v] + x[3:], k[v], X + dX, uv, terms=False)[1]

    def anchored(yv):  # the anchor's own update: R' = exp([w]x) R, c' = c + e, t' = -R' c'
        R2 = ref.rotate_left(yv[:3], R[v])
        return ref.observe(R2, -(R2 @ (-(R[v].T @ t[v]) + yv[3:])), k[v], X, uv, terms=False)[1]

    M = ref.anchor_matrix(R[v], t[v])
    worst = 0.0
    for q in range(6):
        e = np.zeros(6)
        e[q] = h
        worst = max(worst, np.abs((residual(e) - residual(-e)) / (2 * h) - J[:, :, q]).max())
        worst = max(worst, np.abs((anchored(e) - anchored(-e)) / (2 * h) - (J @ M)[:, :, q]).max())
    for q in range(3):
        e = np.zeros(3)
        e[q] = h
        worst = max(worst, np.abs((residual(np.zeros(6), e) - residual(np.zeros(6), -e)) / (2 * h) - G[:, :, q]).max())
    print("|analytic - central difference| %.3g (entries up to %.0f)" % (worst, np.abs(J).max()))
    assert worst <= ref.FD_BOUND and np.abs(J).max() > 50


def test_the_anchor_keeps_its_coordinate_and_the_fixed_view_its_pose():
    c, r = tolerance.solved("five", True)
    anchor, axis = r["anchor"]
    assert (anchor, axis) == ref.gauge(c["T0"], 0) and anchor != 0
    assert np.array_equal(r["T"][0], c["T0"][0])
    assert abs(r["T"][anchor][axis, 3] - c["T0"][anchor][axis, 3]) < 1e-14
    far = np.linalg.norm(c["T0"][:, :3, 3] - c["T0"][0, :3, 3], axis=1)
    assert anchor == int(np.argmax(far)) and axis == int(np.argmax(np.abs(c["T0"][anchor, :3, 3] - c["T0"][0, :3, 3])))


@pytest.mark.parametrize("name", bc.NAMES)
def test_restatement_recovers_the_truth(name):
    """noise-free: the true poses (after the similarity the gauge leaves free) within the distance the tolerance file
    records, below half the cap"""
    rec = tolerance.load()
    c, r = tolerance.solved(name, False)
    assert r["rig_status"] == 0 and r["evaluations"] < ref.MAX_EVALUATIONS / 2
    rot, centre = ref.pose_errors(r["T"], c["T_true"])
    assert rot <= 2 * rec["truth_distance"]["rotation"] and centre <= 2 * rec["truth_distance"]["centre"], (rot, centre)
    assert rot < 1e-7 and centre < 1e-7 and r["retval"] < 1e-6


@pytest.mark.parametrize("name", bc.NAMES)
def test_noisy_cases_end_closer_to_the_truth_than_they_start(name):
    c, r = tolerance.solved(name, True)
    start, result = ref.pose_errors(c["T0"], c["T_true"]), ref.pose_errors(r["T"], c["T_true"])
    print("%s: rotation %.3g -> %.3g rad, centre %.3g -> %.3g" % (name, start[0], result[0], start[1], result[1]))
    assert r["rig_status"] == 0 and result[0] < start[0] and result[1] < start[1]
    # sigma per component: retval is the RMS distance of an observation, of which the points absorb a part
    assert 0.3 * bc.NOISE_SIGMA < r["retval"] < 1.5 * bc.NOISE_SIGMA * np.sqrt(2)


def test_the_cases_hold_what_they_are_there_for():
    c, r = tolerance.solved("borders", True)
    assert r["used_counts"] == [1, 63, 64, 65, 255, 256, 257, 100, 100, 100]
    c, r = tolerance.solved("bad_pair", True)
    rows = bc.single_pair(c, 2)
    assert r["used_counts"][2] == 0 and set(r["status"][rows]) == {1, 2} and np.isnan(r["pair_error"][2])
    assert len(bc.case("sixteen")["pairs"]) == 120
    c, _ = tolerance.solved("five", True)
    p, rows = bc.planted(c)
    got = ref.solve(p["K"], p["T0"], p["pairs"], p["uvs_a"], p["uvs_b"], p["counts"], threshold=bc.THRESHOLD)
    clean, keep = bc.without(p, rows)
    want = ref.solve(clean["K"], clean["T0"], clean["pairs"], clean["uvs_a"], clean["uvs_b"], clean["counts"], threshold=bc.THRESHOLD)
    assert len(rows) == 60 and (got["status"][rows] != 0).all()
    assert np.array_equal(got["status"][keep], want["status"]) and np.array_equal(got["T"], want["T"])


def test_tolerance_file_is_the_measurement():
    """the bounds come from the restatement's own disagreement under a change of summation order, times 8 -- never from
    what the kernels give; every case ends below half the cap"""
    rec, now = tolerance.load(), tolerance.measure()
    assert rec["factor"] == 8 and all(rec["bound"][k] == 8 * rec["disagreement"][k] for k in tolerance.KEYS)
    assert all(0 < now["disagreement"][k] <= rec["bound"][k] for k in tolerance.KEYS)
    assert all(now["truth_distance"][k] <= 2 * rec["truth_distance"][k] for k in rec["truth_distance"])
    assert now["evaluations"] == rec["evaluations"] and sorted(rec["evaluations"]) == sorted(bc.NAMES)
    assert rec["evaluation_cap"] == ref.MAX_EVALUATIONS and max(rec["evaluations"].values()) < rec["evaluation_cap"] / 2
    assert sorted(rec["pose_error"]) == sorted(bc.NAMES) and rec["noise_sigma"] == bc.NOISE_SIGMA
    for name in bc.NAMES:
        assert np.allclose(now["pose_error"][name]["result"], rec["pose_error"][name]["result"], rtol=1e-6, atol=0)
        assert rec["pose_error"][name]["result"][0] < rec["pose_error"][name]["start"][0]
        assert rec["pose_error"][name]["result"][1] < rec["pose_error"][name]["start"][1]


def test_refusals_come_before_the_device(no_device):
    c = bc.case("three")
    ok = dict(K=c["K"], T=c["T0"], pairs=c["pairs"], uvs_a=c["uvs_a"], uvs_b=c["uvs_b"], counts=c["counts"])
    nan_K, nan_T = c["K"].copy(), c["T0"].copy()
    nan_K[1, 0, 0], nan_T[2, 0, 3] = np.nan, np.inf
    wide = bc.case("sixteen")
    K17, T17 = np.concatenate([wide["K"], wide["K"][:1]]), np.concatenate([wide["T0"], wide["T0"][:1]])
    bad = [
        (dict(K=K17, T=T17), "3 .. 16 views, got 17"),
        (dict(K=c["K"][:2], T=c["T0"][:2]), "3 .. 16 views, got 2"),
        (dict(T=c["T0"][:2]), "K must be"),
        (dict(pairs=np.array([[0, 1], [0, 3], [1, 2]], np.int32)), "outside 0 .. 2"),
        (dict(pairs=np.array([[0, 1], [0, 1], [1, 2]], np.int32)), "more than once"),
        (dict(pairs=np.array([[0, 1], [2, 0], [1, 2]], np.int32)), "a < b"),
        (dict(pairs=np.array([[0, 1], [1, 1], [1, 2]], np.int32)), "a < b"),
        (dict(pairs=c["pairs"].astype(np.float64)), "pairs must be"),
        (dict(uvs_b=c["uvs_b"][:-1]), "must agree in shape, dtype and kind"),
        (dict(uvs_b=c["uvs_b"].astype(np.float32)), "must agree in shape, dtype and kind"),
        (dict(uvs_a=c["uvs_a"].astype(np.int32), uvs_b=c["uvs_b"].astype(np.int32)), "float32 or float64"),
        (dict(uvs_a=np.zeros((900, 3)), uvs_b=np.zeros((900, 3))), "(M, 2)"),
        (dict(counts=np.array([300, 300, 299])), "counts sum to 899"),
        (dict(counts=np.array([300, 600])), "counts must be (P,)"),
        (dict(K=nan_K), "finite"),
        (dict(T=nan_T), "finite"),
        (dict(pairs=np.array([[0, 1]], np.int32), counts=np.array([900])), "views [2] are touched by no pair"),
        (dict(fixed_view=3), "fixed_view must be a view"),
        (dict(fixed_view=-1), "fixed_view must be a view"),
        (dict(fixed_view=0.5), "fixed_view must be a view"),
        (dict(threshold=-1.0), "threshold must be"),
    ]
    for change, text in bad:
        if text is None:
            continue
        with pytest.raises(ValueError) as e:
            ca.bundle_adjust_pairs(**dict(ok, **change))
        assert text in str(e.value), (change.keys(), str(e.value))
    with pytest.raises(TypeError):
        ca.bundle_adjust_pairs(**dict(ok, uvs_a=list(c["uvs_a"])))
    with pytest.raises(ValueError) as e:
        ca.ReconstructionExtrinsics.refine(type("R", (), dict(viewds={0: {}, 1: {}}, set2ds={}))(), fixed_view=7)
    assert "fixed_view must be a key" in str(e.value)


def test_exports_and_the_binding():
    assert ca.bundle_adjust_pairs is bundle.bundle_adjust_pairs and "bundle_adjust_pairs" in ca.__all__
    assert hasattr(ca.ReconstructionExtrinsics, "refine")
    src = open(_native.LIB_PATH.replace("calibrating_amd/lib/libcalibrating_amd.so", "include/calibrating_amd.h")).read() \
        if "calibrating_amd/lib/" in _native.LIB_PATH else ""
    for name in ("MAX_VIEWS", "CHUNK", "SEGMENT", "PARTIAL_DOUBLES", "EVAL_DOUBLES", "STATE_DOUBLES"):
        assert not src or "#define CAMD_BUNDLE_%s %d" % (name, getattr(_native, "BUNDLE_" + name)) in src
    for name in ("DONE", "ACCEPT", "LAMBDA", "COST", "EVALUATIONS", "ITERATIONS", "STATUS", "CONVERGED", "SOLVED", "PIVOT", "FIXED",
                 "ANCHOR", "AXIS", "COST0", "LABEL", "POSES", "CANDIDATE", "STEP", "K"):
        assert not src or "CAMD_BUNDLE_%s = %d" % (name, getattr(_native, "BUNDLE_" + name)) in src
    assert _native.BUNDLE_K + 4 * _native.BUNDLE_MAX_VIEWS == _native.BUNDLE_STATE_DOUBLES
    assert _native.BUNDLE_DONE == _native.CALIB_DONE and _native.BUNDLE_ACCEPT == _native.CALIB_ACCEPT  # camd_calib_read's places
    table, ranges = bundle._chunks([1, 0, 257, 256])
    assert table.tolist() == [[0, 0, 1, 0], [2, 1, 256, 0], [2, 257, 1, 0], [3, 258, 256, 0]] and ranges.tolist() == [0, 1, 1, 3, 4]
    first, n = bundle._segments([1, 0, 1025])
    assert first.tolist() == [0, 1, 1025] and n.tolist() == [1, 1024, 1]
