"""The RANSAC 8-point estimator on the GPU (-m gpu): every stage of csrc/essential.hip against the NumPy restatement
(tests/essential_ref.py) bit for bit, then ``find_essential_matrix`` and ``EssentialMatrixStereo(robust=...)`` end to end on
the contaminated scenes of tests/essential_cases.py.  Plain imports: a missing feature fails."""
import numpy as np
import pytest
import torch

import calibrating_amd as ca
from calibrating_amd import epipolar_geometry as eg

import epipolar_ref
import essential_cases as es
import essential_ref as er

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _stages(uvs1, uvs2, K1, K2, hypotheses, seed=es.STAGE_SEED, threshold=es.THRESHOLD):
    """every stage alone through the private helpers -> host arrays"""
    rows = eg._EssentialRows(uvs1, uvs2, K1, K2)
    thr2 = er.ray_threshold2(K1, K2, threshold)
    samples, Es = eg._essential_hypotheses(rows, hypotheses, seed)
    counts, winner = eg._essential_score(rows, Es, thr2)
    mask, sums = eg._essential_moments(rows, winner[:9], thr2)
    return dict(rows=rows, samples=_host(samples), Es=_host(Es), counts=_host(counts), winner=_host(winner), mask=_host(mask) != 0,
                sums=_host(sums), thr2=thr2)


@pytest.mark.parametrize("n,hypotheses,dtype", es.STAGE_CASES)
def test_stages_against_the_restatement(n, hypotheses, dtype):
    """Samples as integers; the matrices BIT FOR BIT (every operation of stage 1 is an individually rounded product or sum,
    a correctly rounded division or square root, on both sides); then, with the DEVICE's matrices fed to both, counts,
    winner, mask, number of inliers and the 46 sums bit for bit.  ndarrays and CUDA tensors take turns."""
    uvs1, uvs2, K1, K2 = es.stage_inputs(n, dtype)
    ref = es.stage_reference(n, hypotheses, dtype)
    conv = _cuda if (n + hypotheses) % 2 else (lambda a: a)
    got = _stages(conv(uvs1), conv(uvs2), K1, K2, hypotheses)
    assert got["samples"].dtype == np.int32 and np.array_equal(got["samples"], ref["samples"])
    assert all(len(set(row)) == 8 and min(row) >= 0 and max(row) < n for row in got["samples"].tolist())
    angles = [er.angle9(g, r) for g, r in zip(got["Es"], ref["Es"]) if g.any() and r.any()]
    print("n=%d H=%d %s: %d of %d matrices differ in a bit, largest angle %.3g" % (
        n, hypotheses, dtype, int((got["Es"] != ref["Es"]).any(1).sum()), hypotheses, max(angles, default=0.0)))
    assert np.array_equal(got["Es"], ref["Es"])
    same = er.find(uvs1, uvs2, K1, K2, es.THRESHOLD, hypotheses, es.STAGE_SEED, Es=got["Es"])
    assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], same["counts"])
    assert int(got["winner"][9]) == same["hypothesis"] and int(got["winner"][10]) == same["hypothesis_inliers"]
    assert np.array_equal(got["winner"][:9], got["Es"][same["hypothesis"]])
    assert np.array_equal(got["mask"], same["hypothesis_mask"]) and int(got["sums"][45]) == int(got["mask"].sum())
    assert np.array_equal(got["sums"], same["hypothesis_sums"])
    # the whole call: the same winner, the same refit (the host's eigh of the same 81 numbers), the same answer
    info = eg.find_essential_matrix(conv(uvs1), conv(uvs2), K1, K2, es.THRESHOLD, hypotheses, es.STAGE_SEED, return_info=True)
    assert isinstance(info["inliers"], torch.Tensor if conv is _cuda else np.ndarray) and info["inliers"].dtype in (torch.bool, np.bool_)
    inl = _host(info["inliers"]) if conv is _cuda else info["inliers"]
    for key in ("hypothesis", "hypothesis_inliers", "refined", "status", "n_inliers"):
        assert info[key] == same[key], key
    assert np.array_equal(info["E"], same["E"]) and np.array_equal(inl, same["inliers"])
    assert info["E"].dtype == np.float64 and info["E"].shape == (3, 3) and np.linalg.matrix_rank(info["E"], tol=1e-12) == 2


def test_a_hypothesis_does_not_depend_on_how_many_there_are():
    uvs1, uvs2, K1, K2 = es.stage_inputs(1000, "float64")
    rows = eg._EssentialRows(uvs1, uvs2, K1, K2)
    few, many = eg._essential_hypotheses(rows, 5, 3), eg._essential_hypotheses(rows, 1024, 3)
    for a, b in zip(few, many):
        assert np.array_equal(_host(a), _host(b)[:5])
    assert not np.array_equal(_host(many[0]), _host(eg._essential_hypotheses(rows, 1024, 4)[0]))


def test_a_strided_view_is_read_in_place():
    uvs1, uvs2, K1, K2 = es.stage_inputs(257, "float64")
    rng = np.random.default_rng(9)
    wide1, wide2 = _cuda(rng.uniform(-1e6, 1e6, (257, 5))), _cuda(rng.uniform(-1e6, 1e6, (257, 3)))
    wide1[:, 1:3], wide2[:, 1:3] = _cuda(uvs1), _cuda(uvs2)
    v1, v2 = wide1[:, 1:3], wide2[:, 1:3]
    rows = eg._EssentialRows(v1, v2, K1, K2)
    assert (rows.stride1, rows.stride2) == (5, 3) and rows.uv1.data_ptr() == v1.data_ptr() and rows.uv2.data_ptr() == v2.data_ptr()
    got = eg.find_essential_matrix(v1, v2, K1, K2, hypotheses=65, seed=es.STAGE_SEED, return_info=True)
    want = eg.find_essential_matrix(uvs1, uvs2, K1, K2, hypotheses=65, seed=es.STAGE_SEED, return_info=True)
    assert np.array_equal(got["E"], want["E"]) and np.array_equal(_host(got["inliers"]), want["inliers"])
    assert got["hypothesis"] == want["hypothesis"] and got["n_inliers"] == want["n_inliers"]
    # a view whose columns do not lie side by side is copied, and gives the same
    turned = _cuda(np.ascontiguousarray(uvs1.T)).T
    assert np.array_equal(eg.find_essential_matrix(turned, _cuda(uvs2), K1, K2, hypotheses=65, seed=es.STAGE_SEED), want["E"])


def test_eight_copies_of_one_match_are_marked_and_nothing_leaks():
    uvs1, uvs2, K1, K2 = es.degenerate_inputs()
    got = _stages(uvs1, uvs2, K1, K2, 5)
    assert not got["Es"].any() and not got["counts"].any() and got["winner"][10] == 0 and np.isfinite(got["winner"]).all()
    assert not got["mask"].any() and not got["sums"].any()
    info = eg.find_essential_matrix(uvs1, uvs2, K1, K2, hypotheses=5, return_info=True)
    assert info["status"] == "degenerate" and not info["E"].any() and info["n_inliers"] == 0 and not info["inliers"].any()
    assert not eg.find_essential_matrix(_cuda(uvs1), _cuda(uvs2), K1, K2, hypotheses=5).any()
    with pytest.raises(ValueError, match="determine"):
        s = es.end_to_end("clean")
        ca.EssentialMatrixStereo(uvs1, uvs2, K1, K2, xy1=s["xy1"], xy2=s["xy2"], robust=dict(hypotheses=5))


def test_two_identical_calls_give_identical_bits():
    s = es.end_to_end("wrong_30")
    a = eg.find_essential_matrix(_cuda(s["uvs1"]), _cuda(s["uvs2"]), s["K1"], s["K2"], return_info=True)
    b = eg.find_essential_matrix(_cuda(s["uvs1"]), _cuda(s["uvs2"]), s["K1"], s["K2"], return_info=True)
    assert a["E"].tobytes() == b["E"].tobytes() and torch.equal(a["inliers"], b["inliers"])
    assert {k: a[k] for k in a if k not in ("E", "inliers")} == {k: b[k] for k in b if k not in ("E", "inliers")}
    got = [_stages(s["uvs1"], s["uvs2"], s["K1"], s["K2"], 1024, seed=0) for _ in range(2)]
    for key in ("samples", "Es", "counts", "winner", "mask", "sums"):
        assert got[0][key].tobytes() == got[1][key].tobytes(), key


def _today_on(s, rows):
    """the existing 8-point fit handed the matches ``rows`` (a mask)"""
    u1, u2 = s["uvs1"][rows], s["uvs2"][rows]
    return eg.compute_essential_matrix(eg.uvs_to_xyz_noramls(eg._host_subsample(u1, len(u1)), s["K1"]),
                                       eg.uvs_to_xyz_noramls(eg._host_subsample(u2, len(u2)), s["K2"]))


@pytest.mark.parametrize("name", list(es.END_TO_END))
def test_pose_error_and_mask_end_to_end(name):
    """Rotation angle and angle between the translation directions against the scene's truth: no more than twice what the
    existing ``compute_essential_matrix`` gets when handed the true inliers only; the mask differs from the true matrix'
    mask at the same threshold on at most 2 % of the rows.  Measured on an MI355X (radians, ours against the existing fit):
    wrong_30 (4.8e-4, 2.6e-3) against (1.2e-3, 2.7e-3), mask 0.2 %; clean (5.4e-4, 2.8e-3) against (2.9e-3, 3.6e-3), mask
    0 %; eight_exact 0 against 0 (both below the resolution of arccos), mask 0 %."""
    s = es.end_to_end(name)
    info = eg.find_essential_matrix(s["uvs1"], s["uvs2"], s["K1"], s["K2"], return_info=True)
    ours = er.pose_error(info["E"], s["R"], s["t"])
    base = er.pose_error(_today_on(s, ~s["wrong"]), s["R"], s["t"])
    differ = float((info["inliers"] != es.true_mask(s)).mean())
    print("%s: pose error %s, the existing fit on the true inliers %s; mask differs on %.4f; %d inliers, hypothesis %d (%d), refined %s"
          % (name, ours, base, differ, info["n_inliers"], info["hypothesis"], info["hypothesis_inliers"], info["refined"]))
    assert info["status"] == "ok" and np.isfinite(info["E"]).all()
    assert ours[0] <= 2 * base[0] and ours[1] <= 2 * base[1]
    assert differ <= es.MASK_LIMIT
    assert info["n_inliers"] == int(info["inliers"].sum()) and info["n_inliers"] >= info["hypothesis_inliers"]


@pytest.mark.parametrize("cuda", [False, True])
def test_the_whole_call_on_the_contaminated_scene(cuda):
    """``EssentialMatrixStereo(..., robust=True)`` on 30 % wrong pairs: the candidate with positive depths, n depths, the
    caller's kind of mask, and the rows of the true inliers aligned after rectification, camera 2 standing where it truly
    stood: max |v1 - v2| no more than twice what today's path gives on the uncontaminated scene.  Measured on an MI355X:
    1.04 px against 2.43 px (bound 4.86 px)."""
    s, clean = es.end_to_end("wrong_30"), es.end_to_end("clean")
    conv = _cuda if cuda else (lambda a: a)
    st = ca.EssentialMatrixStereo(conv(s["uvs1"]), conv(s["uvs2"]), s["K1"], s["K2"], baseline=0.3, xy1=s["xy1"], xy2=s["xy2"],
                                  robust=True)
    plain = ca.EssentialMatrixStereo(clean["uvs1"], clean["uvs2"], clean["K1"], clean["K2"], baseline=0.3, xy1=clean["xy1"],
                                     xy2=clean["xy2"])
    kind = torch.Tensor if cuda else np.ndarray
    inliers, zs1, zs2 = st.epipolar["inliers"], st.epipolar["zs1"], st.epipolar["zs2"]
    assert isinstance(inliers, kind) and isinstance(zs1, kind) and tuple(inliers.shape) == tuple(zs1.shape) == tuple(zs2.shape) == (1000,)
    inliers, zs1, zs2 = (_host(a) if cuda else a for a in (inliers, zs1, zs2))
    assert inliers.dtype == np.bool_ and st.epipolar["n_inliers"] == inliers.sum() == st.robust_info["n_inliers"]
    assert st.robust_info["status"] == "ok" and np.array_equal(st.epipolar["E"], st.robust_info["E"])
    assert st.epipolar["z1"] > 0 and st.epipolar["z2"] > 0 and (zs1[inliers] > 0).mean() > 0.99 and (zs2[inliers] > 0).mean() > 0.99
    good = ~s["wrong"]
    assert np.abs(zs1[good & inliers] / s["X1"][good & inliers, 2] * (np.linalg.norm(s["t"]) / 0.3) - 1).max() < 0.2
    v1, v2 = epipolar_ref.rectified_v(st, s["X1"][good], s["R"], s["t"])
    w1, w2 = epipolar_ref.rectified_v(plain, clean["X1"], clean["R"], clean["t"])
    worst, bound = float(np.abs(v1 - v2).max()), 2 * float(np.abs(w1 - w2).max())
    print("rows of the true inliers: max |v1 - v2| = %.3g px, today's path on the uncontaminated scene %.3g px" % (worst, bound / 2))
    assert worst <= bound
    # from_stereo passes the argument on and keeps the record
    again = ca.EssentialMatrixStereo.from_stereo(conv(s["uvs1"]), conv(s["uvs2"]), plain, robust=dict(seed=0))
    assert np.array_equal(again.R, st.R) and np.array_equal(again.epipolar["E"], st.epipolar["E"])


def test_no_change_at_the_default():
    """``robust=None``: R, t, E, zs1, zs2 bit-equal to a direct call of the helpers that made them before"""
    s = es.end_to_end("wrong_30")
    st = ca.EssentialMatrixStereo(s["uvs1"], s["uvs2"], s["K1"], s["K2"], baseline=0.3, xy1=s["xy1"], xy2=s["xy2"])
    assert "inliers" not in st.epipolar and not hasattr(st, "robust_info")
    n = s["n"]
    E = eg.compute_essential_matrix(eg.uvs_to_xyz_noramls(s["uvs1"][:: n // 100], s["K1"]),
                                    eg.uvs_to_xyz_noramls(s["uvs2"][:: n // 100], s["K2"]))
    Ts = eg.decompose_essential_matrix(E)
    for T in Ts:
        T[:3, 3] *= 0.3 / np.linalg.norm(T[:3, 3])
    a, b = _cuda(s["uvs1"]), _cuda(s["uvs2"])
    means = eg._candidate_means(a, b, s["K1"], s["K2"], Ts)
    T = Ts[next((c for c in range(4) if means[c, 0] > 0 and means[c, 1] > 0), 3)]
    zs = eg.matched_uvs_to_zs(a, b, s["K1"], s["K2"], T)
    assert np.array_equal(st.epipolar["E"], E) and np.array_equal(st.R, T[:3, :3]) and np.array_equal(np.ravel(st.t), T[:3, 3])
    assert np.array_equal(st.epipolar["zs1"], _host(zs["zs1"])) and np.array_equal(st.epipolar["zs2"], _host(zs["zs2"]))


def test_non_finite_tensors_are_refused():
    s = es.end_to_end("clean")
    bad = s["uvs2"].copy()
    bad[501, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        eg.find_essential_matrix(_cuda(s["uvs1"]), _cuda(bad), s["K1"], s["K2"])
    with pytest.raises(ValueError, match="finite"):
        eg.find_essential_matrix(s["uvs1"], bad, s["K1"], s["K2"])
