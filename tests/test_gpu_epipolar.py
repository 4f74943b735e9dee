"""The epipolar path on the GPU (-m gpu): calibrating_amd.epipolar_geometry against the reference's own output
(tests/golden/reference_epipolar.npz) and the NumPy restatements (tests/epipolar_ref.py).  Every integer, compacted or
converted array is compared bit for bit (values, dtype, shape, order); the pose within SENS_FACTOR x the reference's
recorded one-ulp sensitivity; depths against an exact fractions.Fraction solve; means against the error bound of the
documented reduction shape.  Plain imports: a missing feature fails."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import calibrating_amd as ca
from calibrating_amd import _native, epipolar_geometry as eg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import reference_cases as rc  # noqa: E402
import epipolar_cases as ec  # noqa: E402
import epipolar_ref as er  # noqa: E402
from test_epipolar_cpu import check_set2ds, pose_case, same_as_fixture  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def fx():
    f = ec.load_fixture()
    assert f is not None, "tests/golden/reference_epipolar.npz is missing"
    return f


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    assert isinstance(t, torch.Tensor) and t.is_cuda, type(t)
    return t.cpu().numpy()


# ---- matching, overlap, flow: bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.MATCH_CASES))
def test_matching_equals_the_reference(fx, name):
    uvs1, uvs2, d, k = ec.match_case(name)
    got = eg.matching_uvs_in_one_img(uvs1, uvs2, d, k)
    dev = eg.matching_uvs_in_one_img(_cuda(uvs1), _cuda(uvs2), d, k)
    assert sorted(got) == sorted(dev) == [str(s) for s in fx["match/%s/keys" % name]]
    for key, v in got.items():
        assert isinstance(v, np.ndarray) and same_as_fixture(fx, "match/%s/%s" % (name, key), v)
        assert _same(_np(dev[key]), v)
    if name == "too_few":
        assert got == {} and dev == {}


def test_matching_first_index_wins_and_half_goes_to_even():
    uvs1 = np.array([[0.5, 0.5], [1.5, 2.5], [0.4, -0.4], [-1.5, -0.5], [2.0, 2.0]] * 3)
    uvs2 = np.array([[2.2, 1.8], [-2.0, 0.0], [0.0, 0.0]] * 4)
    got = eg.matching_uvs_in_one_img(uvs1, uvs2, MIN_MATCHED_PIXELS=1)
    # cells of set 1: (0,0) (2,2) (0,0) (-2,0) (2,2); shared with set 2, ascending (u, v): (-2,0), (0,0), (2,2)
    assert got["uv_match_idx1"].tolist() == [3, 0, 1] and got["uv_match_idx2"].tolist() == [1, 2, 0]
    assert got["uv_match_idx1"].dtype == np.int64


@pytest.mark.parametrize("name", ec.OVERLAP_CASES)
def test_overlap_filter_equals_the_reference(fx, name):
    uvs1, uvs2 = ec.overlap_case(name)
    a, b = eg.filter_overlap_uvs(uvs1, uvs2)
    assert isinstance(a, np.ndarray) and same_as_fixture(fx, "overlap/%s/uvs1" % name, a) and same_as_fixture(fx, "overlap/%s/uvs2" % name, b)
    ta, tb = eg.filter_overlap_uvs(_cuda(uvs1), _cuda(uvs2))
    assert _same(_np(ta), a) and _same(_np(tb), b)
    if name == "every_point_overlaps":
        assert a.shape == (0, 2) and a.dtype == np.float32


@pytest.mark.parametrize("name", list(ec.FLOW_CASES))
def test_flow_to_matched_uvs_equals_the_reference(fx, name):
    flow, mask = ec.flow_case(name)
    a, b = eg.flow_to_matched_uvs(flow, mask)
    ta, tb = eg.flow_to_matched_uvs(_cuda(flow), _cuda(mask))
    assert isinstance(a, np.ndarray) and _same(_np(ta), a) and _same(_np(tb), b)
    if not mask.any():
        assert a.shape == (0, 2) and a.dtype == np.float64
        assert eg.build_set2ds_by_flowds({0: {}, 1: {}}, {(0, 1): dict(flow_abs=flow, common_fov_mask=mask)}) == {}
        return
    assert same_as_fixture(fx, "flow/%s/from" % name, a) and same_as_fixture(fx, "flow/%s/to" % name, b)


def test_build_set2ds_equals_the_reference(fx):
    viewds, flowds = ec.flowds_case("two_way")
    got = eg.build_set2ds_by_flowds(viewds, flowds)
    assert all(isinstance(v, np.ndarray) for d in got.values() for v in d.values())
    check_set2ds(fx, "two_way", got)
    dev = eg.build_set2ds_by_flowds({k: {kk: _cuda(vv) for kk, vv in v.items()} for k, v in viewds.items()},
                                    {k: {kk: _cuda(vv) for kk, vv in v.items()} for k, v in flowds.items()})
    check_set2ds(fx, "two_way", dev, _np)
    # the one-direction flow_normal without a view mask, where the reference fails: scaled to its own (h, w)
    viewds, flowds = ec.flowds_case("normal_no_view_mask")
    got, want = eg.build_set2ds_by_flowds(viewds, flowds), er.set2ds(viewds, flowds)
    assert list(got) == list(want) and list(got[frozenset((0, 1))]) == ["uvs_ij_i", "uvs_ij_j", "uvs_i", "uvs_j"]
    assert all(_same(got[frozenset((0, 1))][k], v) for k, v in want[frozenset((0, 1))].items())


@pytest.mark.parametrize("name", list(ec.CONVERT_CASES))
def test_flow_conversions_equal_the_reference(fx, name):
    seed, hw, target = ec.CONVERT_CASES[name]
    flow = ec.flow_abs(seed, hw)
    normal = eg.flow_abs_to_normal(flow)
    assert same_as_fixture(fx, "convert/%s/normal" % name, normal) and _same(_np(eg.flow_abs_to_normal(_cuda(flow))), normal)
    back = eg.flow_normal_to_abs(normal, target)
    assert same_as_fixture(fx, "convert/%s/abs" % name, back) and _same(_np(eg.flow_normal_to_abs(_cuda(normal), target)), back)
    assert same_as_fixture(fx, "convert/%s/abs_of_f64" % name, eg.flow_normal_to_abs(normal.astype(np.float64), target))
    assert same_as_fixture(fx, "convert/%s/normal_of_f64" % name, eg.flow_abs_to_normal(flow.astype(np.float64)))
    assert _same(eg.flow_abs_to_normal(np.asfortranarray(flow)), normal)  # any strides


# ---- EssentialMatrixStereo -----------------------------------------------------------------------------------------------
def _construct(c, cuda=False):
    conv = _cuda if cuda else (lambda a: a)
    if "record" in c:
        return ca.EssentialMatrixStereo.from_stereo(conv(c["uvs1"]), conv(c["uvs2"]), ca.Stereo().load(c["record"]))
    return ca.EssentialMatrixStereo(conv(c["uvs1"]), conv(c["uvs2"]), c["K1"], c["K2"], baseline=c["baseline"], xy1=c["xy1"],
                                    xy2=c["xy2"])


def _mean_bound(z, got, what):
    """|got - exact mean| <= (m + d + 1) 2^-53 mean|z|: m serial additions and d tree levels per term (the header's
    reduction shape), one more rounding for the division by n."""
    n = len(z)
    m, d = er.reduction_shape(n)
    mean, mean_abs = er.exact_mean(z)
    err, bound = abs(float(got) - float(mean)), (m + d + 1) * U * float(mean_abs)
    print("%s: n=%d m=%d d=%d  |mean - exact| = %.3g, bound %.3g" % (what, n, m, d, err, bound))
    assert err <= bound, what


@pytest.mark.parametrize("name", ec.ALL_POSE_CASES)
def test_pose_equals_the_reference_within_its_sensitivity(fx, name):
    c = pose_case(fx, name)
    st = _construct(c)
    ep, f = st.epipolar, ec.SENS_FACTOR
    assert sorted(ep) == ["E", "uvs1", "uvs2", "z1", "z2", "zs1", "zs2"]
    assert isinstance(ep["zs1"], np.ndarray) and ep["zs1"].dtype == np.float64 and ep["zs1"].shape == (len(c["uvs1"]),)
    assert isinstance(ep["E"], np.ndarray) and ep["E"].shape == (3, 3) and type(ep["z1"]) is float and type(ep["z2"]) is float
    assert ep["uvs1"] is c["uvs1"] and ep["uvs2"] is c["uvs2"]
    assert st.candidate == int(fx[name + "/winner"]), "not the candidate the reference chose"
    got = dict(R=st.R, t=st.t.reshape(3), z1=ep["z1"], z2=ep["z2"])
    for k, v in got.items():
        dist = float(np.abs(np.asarray(v) - fx["%s/%s" % (name, k)]).max())
        allowed = f * float(fx["%s/sens_%s" % (name, k)])
        if k == "R":  # float32-rounded entries: sens_R is 0, one float32 ulp is allowed (epipolar_cases.R_ULP says why)
            allowed = max(allowed, ec.R_ULP)
        print("%s: |%s - reference| = %.3g (sens %.3g, allowed %.3g)" % (name, k, dist, fx["%s/sens_%s" % (name, k)], allowed))
        assert dist <= allowed, k
    assert er.E_distance(ep["E"], fx[name + "/E"]) <= f * fx[name + "/sens_E"]
    assert abs(st.baseline - float(fx[name + "/baseline"])) <= 1e-15 * st.baseline + f * fx[name + "/sens_t"] * 3
    for k in ("R1", "R2", "K"):  # the rig the pose leads to
        assert np.abs(getattr(st, k) - fx["%s/%s" % (name, k)]).max() <= 1e-9 * max(1.0, np.abs(fx["%s/%s" % (name, k)]).max()), k
    # depths: a seeded sample against the exact solve under the object's own pose
    K2 = c["K1"] if c["K2"] is None else c["K2"]
    rows = ec.zs_sample(len(c["uvs1"]))
    err = er.zs_relerr(ep["zs1"], ep["zs2"], c["uvs1"], c["uvs2"], c["K1"], K2, st.R, st.t, rows)
    print("%s: zs %.3g relative from exact (reference %.3g)" % (name, err, fx[name + "/ref_zs_relerr"]))
    assert err <= 2 * fx[name + "/ref_zs_relerr"]
    _mean_bound(ep["zs1"], ep["z1"], name + " z1")
    _mean_bound(ep["zs2"], ep["z2"], name + " z2")
    # tensors in -> tensors out, the same numbers
    dv = _construct(c, cuda=True)
    assert isinstance(dv.epipolar["zs1"], torch.Tensor) and dv.epipolar["zs1"].is_cuda and isinstance(dv.epipolar["uvs1"], torch.Tensor)
    assert _same(_np(dv.epipolar["zs1"]), ep["zs1"]) and _same(_np(dv.epipolar["zs2"]), ep["zs2"])
    assert _same(dv.R, st.R) and _same(dv.t, st.t) and dv.epipolar["z1"] == ep["z1"] and _same(dv.epipolar["E"], ep["E"])
    if "record" in c:  # from_stereo: everything of the source record except R, t survives
        import json
        mine, ref, src = st.dump(return_dict=True), json.loads(str(fx[name + "/dump_json"])), ca.Stereo().load(c["record"]).dump(return_dict=True)
        for cam in ("cam1", "cam2"):
            assert mine[cam] == src[cam] and mine[cam]["D"] == ref[cam]["D"] and mine[cam]["name"] == ref[cam]["name"]
        assert sorted(mine) == sorted(src) and np.any(st.cam1.D) and mine["R"] != src["R"]
        assert all(mine[k] == src[k] for k in src if k not in ("R", "t")), "every entry but R, t is kept, by value"
        rec = dict(c["record"], retval=0.4321)  # a record that carries more than the cameras
        kept = ca.EssentialMatrixStereo.from_stereo(c["uvs1"], c["uvs2"], ca.Stereo().load(rec)).dump(return_dict=True)
        assert kept["retval"] == 0.4321 and all(kept[k] == mine[k] for k in mine)
        assert abs(st.baseline - ca.Stereo().load(c["record"]).baseline) < 1e-12


def _row_alignment(fx, name):
    """(rig, largest |v1 - v2| px of the case's scene points projected through the rig's two rectified cameras, its bound,
    the same with camera 2 where it truly stood, the reference's own figure for that).
    Bound of the first.  With exact arithmetic the rectifying rotations put a point on one row in both cameras of the rig.
    The pose may differ from the reference's by SENS_FACTOR x sens; a change dR of the rotation / dt of the translation
    moves a rectified ray by at most |dR| + |dt| / |t| rad (first order), fy times that in pixels, in both cameras: factor
    2, and 3 entries per matrix row.  The rotation the reference returns is itself rounded through float32 (its
    R_t_to_T), so it is orthogonal to 2^-24 per entry only.  On top of that the case's pixel noise level (sigma of its
    Gaussian noise) is allowed, as the issue states."""
    c = pose_case(fx, name)
    st = _construct(c)
    fy = float(st.K[1, 1])
    sens = 2 * fy * (3 * float(fx[name + "/sens_R"]) + 3 * float(fx[name + "/sens_t"]) / st.baseline + 3 * 2.0 ** -24)
    v1, v2 = er.rectified_v(st, c["X1"])
    w1, w2 = er.rectified_v(st, c["X1"], c["R"], c["t"])
    return (st, float(np.abs(v1 - v2).max()), c["noise"] + ec.SENS_FACTOR * sens, float(np.abs(w1 - w2).max()),
            float(fx[name + "/ref_row_error"]))


@pytest.mark.parametrize("name", ["scene_720p_clean", "scene_720p_noise"])
def test_rectify_and_get_depth_run_and_epipolar_rows_align(fx, name):
    st, worst, bound, true_worst, ref_true_worst = _row_alignment(fx, name)
    print("%s: max |v1 - v2| = %.3g px through the rig's rectified cameras, bound %.3g" % (name, worst, bound))
    assert worst < bound
    # Beyond the issue: camera 2 where it truly stood.  Now the 8-point estimate's own error shows (at 0.3 px of noise it
    # comes from 178 of 17 873 matches): the reference's own rig is 1.7e-5 px (no noise) and 0.789 px (0.3 px) off, figures
    # the fixture holds.  The rule of the triangulation tests: at most twice the reference's own error.
    print("%s: ... with camera 2 where it truly stood %.3g px (the reference's rig: %.3g)" % (name, true_worst, ref_true_worst))
    assert true_worst <= 2 * ref_true_worst
    rng = np.random.default_rng(5)
    img1 = rng.integers(0, 256, (720, 1280, 3)).astype(np.uint8)
    r1, r2 = st.rectify(img1, img1)
    assert r1.shape == (720, 1280, 3) and r2.dtype == np.uint8
    st.set_stereo_matching(ca.SemiGlobalBlockMatching({}), max_depth=20.0)
    res = st.get_depth(img1, np.roll(img1, -8, 1))
    assert res["unrectify_depth"].shape == (720, 1280) and np.isfinite(res["rectify_depth"]).all()


def test_set_scale_and_align_scale_with(fx):
    tc = ec.trio_case()
    A, B = ca.EssentialMatrixStereo(**tc["A"]), ca.EssentialMatrixStereo(**tc["B"])
    B.set_stereo_matching(ca.SemiGlobalBlockMatching({}), max_depth=5.0)
    before = dict(t=B.t.copy(), z1=B.epipolar["z1"], zs2=B.epipolar["zs2"].copy(), R1=B.R1.copy())
    assert B.set_scale(2.0) is B
    assert _same(B.t, before["t"] * 2) and B.epipolar["z1"] == before["z1"] * 2 and _same(B.epipolar["zs2"], before["zs2"] * 2)
    assert abs(B.baseline - 2.0) < 1e-15 * 4 and _same(B.R1, before["R1"])
    assert B.min_disparity == int(B.cam1.K[0, 0] * B.baseline / B.max_depth)  # nothing derived from the baseline goes stale
    B.align_scale_with(A)
    ratio = B.baseline / A.baseline
    print("ratio %.15g reference %.15g true %.15g sens %.3g" % (ratio, fx["trio/ratio"], tc["true_ratio"], fx["trio/sens_ratio"]))
    assert abs(ratio - float(fx["trio/ratio"])) <= ec.SENS_FACTOR * float(fx["trio/sens_ratio"])
    # against the truth: the rotations come back rounded through float32 (<= 3 * 2^-24 rad per ray), which moves a depth
    # triangulated under a parallax angle >= theta_min by that over theta_min, relatively; two rigs take part
    assert abs(ratio / tc["true_ratio"] - 1) <= 2 * 3 * 2.0 ** -24 / tc["theta_min"]
    B.align_scale_with(A)
    assert abs(B.baseline / A.baseline / ratio - 1) <= 1e-12
    # the gathered mean obeys the bound of its reduction shape
    m = eg.matching_uvs_in_one_img(B.epipolar["uvs1"], A.epipolar["uvs1"])
    assert len(m["uv_match_idx1"]) > 1000
    _mean_bound(B.epipolar["zs1"][m["uv_match_idx1"]], eg._mean(B.epipolar["zs1"], m["uv_match_idx1"]), "gathered mean")
    _mean_bound(A.epipolar["zs1"], eg._mean(_cuda(A.epipolar["zs1"])), "plain mean")
    with pytest.raises(IndexError):
        eg._mean(A.epipolar["zs1"], np.array([0, len(A.epipolar["zs1"])]))
    with pytest.raises(AssertionError, match="share no camera"):
        B.align_scale_with(ca.EssentialMatrixStereo(**dict(tc["A"], name1="x", name2="y")))
    with pytest.raises(AssertionError, match="same pair"):
        A.align_scale_with(ca.EssentialMatrixStereo(**tc["A"]))


# ---- determinism, the C ABI, scale ---------------------------------------------------------------------------------------
def test_identical_calls_give_identical_bits(fx):
    uvs1, uvs2, d, k = ec.match_case("uniform_300k_d1")
    a, b = _cuda(uvs1), _cuda(uvs2)
    for call in (lambda: list(eg.matching_uvs_in_one_img(a, b).values()), lambda: list(eg.filter_overlap_uvs(a, a.flip(0))),
                 lambda: list(eg.flow_to_matched_uvs(*map(_cuda, ec.flow_case("vga_third")))),
                 lambda: [eg.flow_abs_to_normal(_cuda(ec.flow_abs(1, (64, 96))))], lambda: [eg.flow_normal_to_abs(_cuda(ec.flow_abs(1, (64, 96)).transpose(2, 0, 1)))]):
        first, second = call(), call()
        assert all(_same(_np(x), _np(y)) for x, y in zip(first, second))
    c = pose_case(fx, "scene_720p_noise")
    s1, s2 = _construct(c, cuda=True), _construct(c, cuda=True)
    assert s1.epipolar["z1"] == s2.epipolar["z1"] and s1.epipolar["z2"] == s2.epipolar["z2"] and _same(s1.t, s2.t)
    assert _same(_np(s1.epipolar["zs1"]), _np(s2.epipolar["zs1"]))
    z = _cuda(np.random.default_rng(3).normal(0, 1, 700001))
    assert eg._mean(z) == eg._mean(z)


def test_raw_c_abi_with_a_row_stride():
    """Every entry point of csrc/epipolar.hip at least once, straight through ctypes; those that take a row stride on rows
    of 3 elements (u, v, payload)."""
    lib, st = _native.lib(), _native.current_stream()
    rng = np.random.default_rng(11)
    n = 5000
    wide1 = np.concatenate([rng.uniform(-20, 40, (n, 2)), rng.normal(0, 1, (n, 1))], 1)
    wide2 = np.concatenate([rng.uniform(-20, 40, (n, 2)), rng.normal(0, 1, (n, 1))], 1)
    want = er.matching(wide1[:, :2], wide2[:, :2], 2)
    a, b = _cuda(wide1), _cuda(wide2)
    cu0, cv0, cw, ch = -11, -11, 33, 33  # rint(-20 / 2) - 1 .. rint(40 / 2) + 1
    first = torch.empty((2, cw * ch), dtype=torch.int32, device="cuda")
    counters = torch.zeros(3, dtype=torch.int64, device="cuda")
    for k, uv in enumerate((a, b)):
        assert lib.camd_cell_first_index(uv.data_ptr(), _native.VALUE_F64, n, 3, 2.0, cu0, cv0, cw, ch, first[k].data_ptr(),
                                         counters[1 + k:].data_ptr(), st) == 0
    col = torch.empty(cw, dtype=torch.int32, device="cuda")
    assert lib.camd_cell_intersect_count(first[0].data_ptr(), first[1].data_ptr(), cw, ch, col.data_ptr(), st) == 0
    start = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(col, 0, dtype=torch.int64)])
    idx = torch.empty((2, n), dtype=torch.int64, device="cuda")
    assert lib.camd_cell_intersect_emit(first[0].data_ptr(), first[1].data_ptr(), cw, ch, start.data_ptr(), idx[0].data_ptr(),
                                        idx[1].data_ptr(), n, counters.data_ptr(), st) == 0
    cnt, o1, o2 = counters.cpu().tolist()
    assert (o1, o2) == (0, 0) and cnt == len(want["uv_match_idx1"])
    assert np.array_equal(_np(idx[0, :cnt]), want["uv_match_idx1"]) and np.array_equal(_np(idx[1, :cnt]), want["uv_match_idx2"])
    # a window that is too small: the rows outside are counted, nothing is written outside the grid
    assert lib.camd_cell_first_index(a.data_ptr(), _native.VALUE_F64, n, 3, 2.0, 0, 0, 5, 5, first[0].data_ptr(),
                                     counters[1:].data_ptr(), st) == 0
    c5 = np.rint(wide1[:, :2] / 2.0)
    assert int(counters[1].item()) == int((~((c5 >= 0) & (c5 < 5)).all(1)).sum()) > 0
    # overlap filter
    w1, w2 = np.ascontiguousarray(wide1.astype(np.float32)), np.ascontiguousarray(wide2.astype(np.float32))
    wa, wb = er.overlap_filter(w1[:, :2], w2[:, :2])
    a32, b32 = _cuda(w1), _cuda(w2)
    pop = torch.empty((2, 63 * 63), dtype=torch.int32, device="cuda")
    for k, uv in enumerate((a32, b32)):
        assert lib.camd_cell_population(uv.data_ptr(), _native.VALUE_F32, n, 3, -21, -21, 63, 63, pop[k].data_ptr(),
                                        counters[1 + k:].data_ptr(), st) == 0
    blocks = lib.camd_overlap_blocks(n)
    keep, bc = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(blocks, dtype=torch.int32, device="cuda")
    assert lib.camd_overlap_keep(a32.data_ptr(), b32.data_ptr(), _native.VALUE_F32, n, 3, -21, -21, 63, 63, pop[0].data_ptr(),
                                 pop[1].data_ptr(), keep.data_ptr(), bc.data_ptr(), st) == 0
    start = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(bc, 0, dtype=torch.int64)])
    out = torch.empty((2, n, 2), dtype=torch.float32, device="cuda")
    assert lib.camd_overlap_emit(a32.data_ptr(), b32.data_ptr(), _native.VALUE_F32, n, 3, keep.data_ptr(), start.data_ptr(),
                                 out[0].data_ptr(), out[1].data_ptr(), n, counters.data_ptr(), st) == 0
    cnt = int(counters[0].item())
    assert cnt == len(wa) and _same(_np(out[0, :cnt]), wa) and _same(_np(out[1, :cnt]), wb)
    # sums (contiguous [n][2] by contract), vector sum, flow
    c = ec.pose_case("same_K")
    u1, u2 = _cuda(c["uvs1"]), _cuda(c["uvs2"])
    m = len(c["uvs1"])
    Kinv = np.ascontiguousarray(np.linalg.inv(c["K1"])).reshape(9)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = c["R"], c["t"]
    T4 = np.ascontiguousarray(np.stack([T, T, T, T])).reshape(64)
    partials = torch.empty(lib.camd_epipolar_sums_blocks(m) * 8, dtype=torch.float64, device="cuda")
    sums = torch.empty(8, dtype=torch.float64, device="cuda")
    assert lib.camd_epipolar_sums(u1.data_ptr(), u2.data_ptr(), m, Kinv.ctypes.data, Kinv.ctypes.data, T4.ctypes.data,
                                  partials.data_ptr(), sums.data_ptr(), st) == 0
    zs = eg.matched_uvs_to_zs(u1, u2, c["K1"], c["K1"], T)
    s = _np(sums).reshape(4, 2)
    assert (s == s[0]).all()  # the same pose four times: the same bits
    _mean_bound(_np(zs["zs1"]), s[0, 0] / m, "C ABI sums zs1")  # ... of the very zs camd_matched_uvs_to_zs returns
    _mean_bound(_np(zs["zs2"]), s[0, 1] / m, "C ABI sums zs2")
    assert lib.camd_epipolar_sums_blocks(1) == 1 and lib.camd_epipolar_sums_blocks(10 ** 7) == 1024
    # the plain and the gathered sum: idx == NULL against a gather, the out-of-range count, the refusals
    zv = rng.normal(3.0, 2.0, 70001)
    gi = rng.integers(0, len(zv), 30011)
    zd, gd = _cuda(zv), _cuda(gi)
    assert lib.camd_vector_sum_blocks(257) == 2 and lib.camd_vector_sum_blocks(len(zv)) == 274
    vp = torch.empty(lib.camd_vector_sum_blocks(len(zv)) * 2, dtype=torch.float64, device="cuda")
    vs = torch.empty(2, dtype=torch.float64, device="cuda")
    assert lib.camd_vector_sum(zd.data_ptr(), len(zv), None, len(zv), vp.data_ptr(), vs.data_ptr(), st) == 0
    plain = _np(vs).copy()
    assert plain[1] == 0
    _mean_bound(zv, plain[0] / len(zv), "C ABI plain sum")
    assert lib.camd_vector_sum(zd.data_ptr(), len(zv), gd.data_ptr(), len(gi), vp.data_ptr(), vs.data_ptr(), st) == 0
    assert _np(vs)[1] == 0
    _mean_bound(zv[gi], _np(vs)[0] / len(gi), "C ABI gathered sum")
    ident = _cuda(np.arange(len(zv), dtype=np.int64))  # the identity gather adds the same terms in the same order
    assert lib.camd_vector_sum(zd.data_ptr(), len(zv), ident.data_ptr(), len(zv), vp.data_ptr(), vs.data_ptr(), st) == 0
    assert _np(vs)[0] == plain[0]
    bad = gi.copy()
    bad[[5, 77, 3000]] = [-1, len(zv), 2 ** 40]
    keep = np.ones(len(gi), bool)
    keep[[5, 77, 3000]] = False
    assert lib.camd_vector_sum(zd.data_ptr(), len(zv), _cuda(bad).data_ptr(), len(bad), vp.data_ptr(), vs.data_ptr(), st) == 0
    assert _np(vs)[1] == 3  # counted, nothing read outside z, nothing added for them
    _mean_bound(zv[gi[keep]], _np(vs)[0] / keep.sum(), "C ABI gathered sum without the three bad rows")
    assert lib.camd_vector_sum(zd.data_ptr(), len(zv), None, len(zv) + 1, vp.data_ptr(), vs.data_ptr(), st) == _native.CAMD_ERR_BAD_ARG
    assert lib.camd_vector_sum(zd.data_ptr(), len(zv), None, 0, vp.data_ptr(), vs.data_ptr(), st) == _native.CAMD_ERR_BAD_ARG
    # the flow unit conversions
    small = ec.flow_abs(31, (37, 53))
    sd = _cuda(small)
    nrm = torch.empty((2, 37, 53), dtype=torch.float32, device="cuda")
    assert lib.camd_flow_abs_to_normal(sd.data_ptr(), _native.VALUE_F32, 53, 37, nrm.data_ptr(), st) == 0
    assert _same(_np(nrm), er.abs_to_normal(small))
    back = torch.empty((37, 53, 2), dtype=torch.float64, device="cuda")
    assert lib.camd_flow_normal_to_abs(nrm.data_ptr(), _native.VALUE_F32, 53, 37, 75.0, 111.0, back.data_ptr(), st) == 0
    assert _same(_np(back), er.normal_to_abs(_np(nrm), (111, 75)))
    n64 = _cuda(_np(nrm).astype(np.float64))
    assert lib.camd_flow_normal_to_abs(n64.data_ptr(), _native.VALUE_F64, 53, 37, 53.0, 37.0, back.data_ptr(), st) == 0
    assert _same(_np(back), er.normal_to_abs(_np(nrm).astype(np.float64)))
    assert lib.camd_flow_abs_to_normal(sd.data_ptr(), _native.VALUE_U8, 53, 37, nrm.data_ptr(), st) == _native.CAMD_ERR_BAD_ARG
    flow, mask = ec.flow_case("vga_third")
    f, mk = _cuda(flow.astype(np.float64)), _cuda(mask).view(torch.uint8)
    rows = torch.empty((2, 100, 2), dtype=torch.float64, device="cuda")  # capacity below the count: nothing beyond it is written
    rows[:] = -7.0
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.camd_arr2d_mask_workspace_bytes(480), dtype=torch.uint8, device="cuda")
    assert lib.camd_flow_to_matched_uvs(f.data_ptr(), _native.VALUE_F64, mk.data_ptr(), 640, 480, rows[0].data_ptr(),
                                        rows[1].data_ptr(), 99, count.data_ptr(), ws.data_ptr(), st) == 0
    wf, wt = er.flow_to_uvs(flow, mask)
    assert int(count.item()) == len(wf) and _same(_np(rows[0, :99]), wf[:99]) and _same(_np(rows[1, :99]), wt[:99])
    assert (_np(rows[:, 99]) == -7.0).all()
    assert lib.camd_cell_first_index(a.data_ptr(), _native.VALUE_F64, n, 1, 2.0, 0, 0, 5, 5, first[0].data_ptr(),
                                     counters.data_ptr(), st) == _native.CAMD_ERR_BAD_ARG
    assert lib.camd_cell_population(a.data_ptr(), _native.VALUE_F64, n, 3, 0, 0, 1 << 15, 1 << 14, first[0].data_ptr(),
                                    counters.data_ptr(), st) == _native.CAMD_ERR_BAD_ARG  # 2^29 cells


def test_matching_and_flow_at_scale():
    uvs1, uvs2 = ec.match_scale_case()
    want = er.matching(uvs1, uvs2)
    got = eg.matching_uvs_in_one_img(_cuda(uvs1), _cuda(uvs2))
    print("1080p, 2 000 000 points per set: %d shared cells" % len(want["uv_match_idx1"]))
    for k in want:
        assert rc.sha(_np(got[k])) == rc.sha(want[k]), k
    flow, mask = ec.flow_scale_case()
    wf, wt = er.flow_to_uvs(flow, mask)
    gf, gt = eg.flow_to_matched_uvs(_cuda(flow), _cuda(mask))
    assert rc.sha(_np(gf)) == rc.sha(wf) and rc.sha(_np(gt)) == rc.sha(wt)
    assert math.isclose(float(gf[0, 0]), 0.5 - 1e-8, rel_tol=0, abs_tol=1e-16)
