"""The epipolar path without a GPU: the NumPy restatements (tests/epipolar_ref.py) against the reference's own output
(tests/golden/reference_epipolar.npz, made by tests/golden/make_epipolar_golden.py) bit for bit, the inputs the fixture was
made from, the generator's conditions, the argument errors that are raised before the device is touched, and the host
pose path (compute_essential_matrix / decompose_essential_matrix) within the reference's recorded sensitivity."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import reference_cases as rc  # noqa: E402
import epipolar_cases as ec  # noqa: E402
import epipolar_ref as er  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    f = ec.load_fixture()
    assert f is not None, "tests/golden/reference_epipolar.npz is missing (python tests/golden/make_epipolar_golden.py)"
    return f


def same_as_fixture(fx, key, a):
    """dtype, shape and SHA-256 of the whole array; every element where the fixture keeps the array whole."""
    assert [a.dtype.str] + [str(s) for s in a.shape] == [str(s) for s in fx[key + "_dtype_shape"]], key
    assert rc.sha(a) == str(fx[key + "_sha"]), key
    if fx[key].shape == a.shape:
        assert np.array_equal(fx[key], a), key
    return True


def pose_case(fx, name):
    return ec.pose_case(name, int(fx[name + "/seed"]) if name + "/seed" in fx else None)


@pytest.mark.parametrize("name", list(ec.MATCH_CASES))
def test_matching_restatement_equals_the_reference(fx, name):
    uvs1, uvs2, d, k = ec.match_case(name)
    assert rc.sha(uvs1) + rc.sha(uvs2) == str(fx["match/%s/in_sha" % name])
    got = er.matching(uvs1, uvs2, d, k)
    assert sorted(got) == [str(s) for s in fx["match/%s/keys" % name]]
    for key, v in got.items():
        assert same_as_fixture(fx, "match/%s/%s" % (name, key), v)
    if name == "too_few":
        assert got == {}


def test_matching_cases_do_what_they_are_there_for():
    a, b = ec.match_case("half_and_negative")[:2]
    assert (a % 1 == 0.5).sum() > 1000 and (a < 0).sum() > 1000 and (b % 1 == 0.5).sum() > 1000
    a, b = ec.match_case("duplicates")[:2]
    assert len(np.unique(np.rint(a).astype(np.int64), axis=0)) < len(a) // 2  # most cells hold several rows
    assert ec.match_case("float32_100k")[0].dtype == np.float32


@pytest.mark.parametrize("name", ec.OVERLAP_CASES)
def test_overlap_restatement_equals_the_reference(fx, name):
    uvs1, uvs2 = ec.overlap_case(name)
    assert rc.sha(uvs1) + rc.sha(uvs2) == str(fx["overlap/%s/in_sha" % name])
    a, b = er.overlap_filter(uvs1, uvs2)
    assert same_as_fixture(fx, "overlap/%s/uvs1" % name, a) and same_as_fixture(fx, "overlap/%s/uvs2" % name, b)
    if name == "every_point_overlaps":
        assert a.shape == (0, 2) and a.dtype == np.float32
    if name == "no_overlap":
        assert len(a) == len(uvs1)


@pytest.mark.parametrize("name", list(ec.FLOW_CASES))
def test_flow_restatement_equals_the_reference(fx, name):
    flow, mask = ec.flow_case(name)
    assert rc.sha(flow) + rc.sha(mask) == str(fx["flow/%s/in_sha" % name])
    if not mask.any():
        assert int(fx["flow/%s/pairs" % name]) == 0  # <= 10 masked pixels: the direction, hence the pair, is skipped
        return
    a, b = er.flow_to_uvs(flow, mask)
    assert same_as_fixture(fx, "flow/%s/from" % name, a) and same_as_fixture(fx, "flow/%s/to" % name, b)


def check_set2ds(fx, name, got, host=lambda a: a):
    pairs = sorted(",".join(str(v) for v in sorted(k)) for k in got)
    assert pairs == [str(s) for s in fx["flowds/%s/pairs" % name]]
    for k, d in got.items():
        pair = ",".join(str(v) for v in sorted(k))
        assert list(d) == [str(s) for s in fx["flowds/%s/%s/keys" % (name, pair)]], "keys and their order"
        for key, v in d.items():
            assert same_as_fixture(fx, "flowds/%s/%s/%s" % (name, pair, key), host(v))


def test_set2ds_restatement_equals_the_reference(fx):
    check_set2ds(fx, "two_way", er.set2ds(*ec.flowds_case("two_way")))
    assert "1,2" not in [str(s) for s in fx["flowds/two_way/pairs"]]  # its only direction has 10 masked pixels
    # a flow_normal without a view mask: the reference hands flow_normal.shape (three numbers) to flow_normal_to_abs
    assert str(fx["flowds/normal_no_view_mask/raises"]).startswith("ValueError: too many values to unpack")


@pytest.mark.parametrize("name", list(ec.CONVERT_CASES))
def test_conversion_restatements_equal_the_reference(fx, name):
    seed, hw, target = ec.CONVERT_CASES[name]
    flow = ec.flow_abs(seed, hw)
    normal = er.abs_to_normal(flow)
    assert same_as_fixture(fx, "convert/%s/normal" % name, normal)
    assert same_as_fixture(fx, "convert/%s/abs" % name, er.normal_to_abs(normal, target))
    assert same_as_fixture(fx, "convert/%s/abs_of_f64" % name, er.normal_to_abs(normal.astype(np.float64), target))
    assert same_as_fixture(fx, "convert/%s/normal_of_f64" % name, er.abs_to_normal(flow.astype(np.float64)))
    assert [str(s) for s in fx["convert/%s/abs_dtype_shape" % name]][0] == np.dtype(np.float64).str  # NumPy's promotion


@pytest.mark.parametrize("name", ec.ALL_POSE_CASES)
def test_pose_inputs_and_generator_conditions(fx, name):
    c = pose_case(fx, name)
    assert rc.sha(c["uvs1"]) == str(fx[name + "/uvs1_sha"]) and rc.sha(c["uvs2"]) == str(fx[name + "/uvs2_sha"])
    means = fx[name + "/cand_means"]
    small = np.abs(means).min(1)
    assert small.min() >= ec.MEAN_FLOOR * small.max(), "a candidate's mean depth is too close to zero to pin its sign"
    w = int(fx[name + "/winner"])
    assert (means[w] > 0).all() and not any((means[i] > 0).all() for i in range(w))
    n = len(c["uvs1"])
    assert {"small_n60": n < 100, "mid_n150": 100 < n < 200, "later_winner": w != 0}.get(name, True)
    if name.startswith("scene_720p"):
        assert 15000 < n < 21000


@pytest.mark.parametrize("name", ec.ALL_POSE_CASES)
def test_host_pose_path_within_the_references_sensitivity(fx, name):
    from calibrating_amd import epipolar_geometry as eg
    c = pose_case(fx, name)
    K2 = c["K1"] if c["K2"] is None else c["K2"]
    E, Ts = eg._pose_candidates(c["uvs1"], c["uvs2"], c["K1"], K2, float(fx[name + "/baseline"]))
    f = ec.SENS_FACTOR
    dE = er.E_distance(E, fx[name + "/E"])
    print("%s: |E - reference| = %.3g (sens %.3g)" % (name, dE, fx[name + "/sens_E"]))
    assert dE <= f * fx[name + "/sens_E"]
    # all four candidates against the reference's four, both sets sorted (by their entries, rotation first).  The rotation
    # is allowed one float32 ulp where SENS_FACTOR x sens_R is smaller (sens_R is 0: epipolar_cases.R_ULP says why)
    key = lambda T: tuple(np.round(T[:3].reshape(-1), 6))  # noqa: E731
    mine, ref = sorted(Ts, key=key), sorted(fx[name + "/candidates"], key=key)
    allow_R, allow_t = max(f * fx[name + "/sens_R"], ec.R_ULP), f * fx[name + "/sens_t"]
    for T, want in zip(mine, ref):
        dR, dt = np.abs(T[:3, :3] - want[:3, :3]).max(), np.abs(T[:3, 3] - want[:3, 3]).max()
        print("%s: candidate |R - reference| %.3g (allowed %.3g), |t - reference| %.3g (allowed %.3g)" % (name, dR, allow_R, dt, allow_t))
        assert dR <= allow_R and dt <= allow_t
    w = int(fx[name + "/winner"])  # ... and unsorted, the reference's winner sits where the reference has it
    assert np.abs(Ts[w][:3, :3] - fx[name + "/R"]).max() <= allow_R and np.abs(Ts[w][:3, 3] - fx[name + "/t"]).max() <= allow_t


def test_argument_errors_need_no_device():
    import calibrating_amd as ca
    from calibrating_amd import epipolar_geometry as eg
    for name in ("EssentialMatrixStereo", "filter_overlap_uvs", "matching_uvs_in_one_img", "flow_abs_to_normal",
                 "flow_normal_to_abs", "flow_to_matched_uvs", "build_set2ds_by_flowds"):
        assert name in ca.__all__ and getattr(ca, name) is getattr(eg, name)
    assert eg.uvs_to_xyz_normals is eg.uvs_to_xyz_noramls and callable(eg.matched_uvs_to_zs)
    assert issubclass(ca.EssentialMatrixStereo, ca.Stereo)
    uvs = np.random.default_rng(0).uniform(0, 100, (20, 2))
    K = np.array([[100.0, 0, 50], [0, 100, 50], [0, 0, 1]])
    with pytest.raises(NotImplementedError, match="argpartition"):
        eg.matching_uvs_in_one_img(uvs, uvs, precise=True)
    with pytest.raises(ValueError, match="xy1"):
        eg.EssentialMatrixStereo(uvs, uvs, K)
    with pytest.raises(ValueError, match="different names"):
        eg.EssentialMatrixStereo(uvs, uvs, K, xy1=(100, 100), xy2=(100, 100), name1="a", name2="a")
    bad = uvs.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        eg.matching_uvs_in_one_img(bad, uvs)
    with pytest.raises(ValueError, match="finite"):
        eg.filter_overlap_uvs(uvs, np.where(np.isnan(bad), np.inf, bad))
    with pytest.raises(ValueError, match="MAX_DISTANCE"):
        eg.matching_uvs_in_one_img(uvs * 1e4, uvs, MAX_DISTANCE=0.01)
    with pytest.raises(ValueError, match="MAX_DISTANCE"):
        eg.matching_uvs_in_one_img(uvs, uvs, MAX_DISTANCE=0)
    with pytest.raises(ValueError, match="float32 or float64"):
        eg.flow_abs_to_normal(np.zeros((4, 4, 2), np.int32))
    with pytest.raises(ValueError, match=r"\(2, h, w\)"):
        eg.flow_normal_to_abs(np.zeros((4, 4, 2), np.float32))
    with pytest.raises(ValueError, match="does not match"):
        eg.flow_to_matched_uvs(np.zeros((4, 4, 2), np.float32), np.ones((4, 5), bool))
    x = eg.uvs_to_xyz_noramls(uvs, K)
    assert x.shape == (20, 3) and np.allclose(x[:, :2], (uvs - 50) / 100) and np.all(x[:, 2] == 1)
