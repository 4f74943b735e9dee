"""The RANSAC 8-point estimator without a GPU: the NumPy restatement (tests/essential_ref.py) against independent
yardsticks, the fixtures (tests/essential_cases.py) against the conditions the GPU tests rely on, and the refusals of
``find_essential_matrix`` that must come before the device is touched."""
import inspect
import math

import numpy as np
import pytest

import epipolar_ref
import essential_cases as es
import essential_ref as er
from calibrating_amd import epipolar_geometry as eg

# the largest angle between the restatement's null vector (inverse iteration on the normal matrix, which squares the
# system's condition number) and np.linalg.svd's of the same 8 x 9 system, measured over every hypothesis of
# es.STAGE_CASES: 2.86e-9 rad (case 1000 x 1024).  The bound is 16 times that.
NULL_VECTOR_ANGLE = 2.86e-9


def _today(s, rows=None):
    """the existing 8-point fit on the scene's matches (``rows``: a mask), as EssentialMatrixStereo feeds it"""
    u1, u2 = (s["uvs1"], s["uvs2"]) if rows is None else (s["uvs1"][rows], s["uvs2"][rows])
    n = len(u1)
    return eg.compute_essential_matrix(eg.uvs_to_xyz_noramls(eg._host_subsample(u1, n), s["K1"]),
                                       eg.uvs_to_xyz_noramls(eg._host_subsample(u2, n), s["K2"]))


def test_samples_are_distinct_in_range_and_independent_of_the_count():
    for n in (8, 9, 63, 1000, 2 ** 31 - 1):
        few, many = er.samples(3, 5, n), er.samples(3, 130, n)
        assert np.array_equal(few, many[:5])
        assert many.min() >= 0 and many.max() < n
        assert all(len(set(row)) == 8 for row in many.tolist())
    assert all(sorted(row) == list(range(8)) for row in er.samples(0, 64, 8).tolist())  # n = 8: every sample is the whole set
    assert not np.array_equal(er.samples(0, 4, 1000), er.samples(1, 4, 1000))
    # the multiply-high map, written out once
    _, key = er._splitmix64(3)
    state, z = er._splitmix64(er._splitmix64(key ^ 2)[1])
    assert er.sample(3, 2, 1000)[0] == (z * 1000) >> 64


@pytest.mark.parametrize("n,hypotheses,dtype", es.STAGE_CASES)
def test_null_vector_against_svd(n, hypotheses, dtype):
    uvs1, uvs2, K1, K2 = es.stage_inputs(n, dtype)
    ref = es.stage_reference(n, hypotheses, dtype)
    a, b = er.rays(uvs1, K1), er.rays(uvs2, K2)
    assert ref["samples"].min() >= 0 and ref["samples"].max() < n
    for h in range(hypotheses):
        e = ref["Es"][h]
        assert e.any(), "a sample of the scene is marked"
        assert abs(np.linalg.norm(e) - 1) < 1e-14 and e[np.argmax(np.abs(e))] > 0
        want = np.linalg.svd(er.rows(a[ref["samples"][h]], b[ref["samples"][h]]))[2][-1]
        assert er.angle9(want, e) <= 16 * NULL_VECTOR_ANGLE
    assert ref["hypothesis"] == int(np.argmax(ref["counts"])) and ref["counts"].dtype == np.int32


def test_rays_and_rows_are_the_reference_layout():
    s = es.end_to_end("clean")
    a, b = er.rays(s["uvs1"], s["K1"]), er.rays(s["uvs2"], s["K2"])
    assert np.abs(a - eg.uvs_to_xyz_noramls(s["uvs1"], s["K1"])).max() < 1e-15
    (x1, y1, z1), (x2, y2, z2) = a.T, b.T
    layout = np.stack([x1 * x2, x2 * y1, z1 * x2, x1 * y2, y1 * y2, z1 * y2, x1 * z2, y1 * z2, z1 * z2], 1)
    assert np.array_equal(er.rows(a, b), layout)
    # row . e = b^T E a, and the true matrix has the clean matches as inliers
    E = er.true_E(s["R"], s["t"])
    assert np.allclose(er.rows(a, b) @ E.reshape(9), np.einsum("ni,ij,nj->n", b, E, a), atol=1e-15)
    assert es.true_mask(s).mean() > 0.99


@pytest.mark.parametrize("n", [8, 257, 1000])
def test_moments_hold_the_exact_sums(n):
    """the fixed-order reduction restated in essential_ref.moments against math.fsum of the same terms"""
    s = es.scene(n=n, wrong=0.2 if n > 8 else 0.0, seed=4300 + n)
    a, b = er.rays(s["uvs1"], s["K1"]), er.rays(s["uvs2"], s["K2"])
    E = er.true_E(s["R"], s["t"]).reshape(9)
    thr2 = er.ray_threshold2(s["K1"], s["K2"], es.THRESHOLD)
    mask, sums = er.moments(E, a, b, thr2)
    assert np.array_equal(mask, er.inliers(E, a, b, thr2)) and sums[45] == mask.sum()
    r = er.rows(a, b)[mask]
    exact = [math.fsum(r[:, p] * r[:, q]) for p in range(9) for q in range(p + 1)]
    assert np.allclose(sums[:45], exact, rtol=1e-13, atol=1e-13 * abs(np.array(exact)).max())


def test_eight_copies_of_one_match_are_marked():
    uvs1, uvs2, K1, K2 = es.degenerate_inputs()
    info = er.find(uvs1, uvs2, K1, K2, es.THRESHOLD, 5, 0)
    assert not info["Es"].any() and not info["counts"].any()
    assert info["status"] == "degenerate" and not info["E"].any() and info["n_inliers"] == 0 and not info["inliers"].any()


@pytest.mark.parametrize("name", list(es.END_TO_END))
def test_fixtures_hold_the_conditions_the_gpu_tests_rely_on(name):
    """The restatement on the end-to-end scenes: its pose error is within twice that of the existing fit on the true
    inliers, its mask within 2 % of the true matrix' mask.  Measured (rotation, translation direction, radians):
    wrong_30 (4.8e-4, 2.6e-3) against (1.2e-3, 2.7e-3), mask 0.2 %; clean (5.4e-4, 2.8e-3) against (2.9e-3, 3.6e-3), mask
    0 %; eight_exact 0 against 0 (both below arccos' resolution)."""
    s = es.end_to_end(name)
    info = er.find(s["uvs1"], s["uvs2"], s["K1"], s["K2"], es.THRESHOLD, 1024, 0)
    ours, base = er.pose_error(info["E"], s["R"], s["t"]), er.pose_error(_today(s, ~s["wrong"]), s["R"], s["t"])
    print(name, "restatement", ours, "existing fit on the true inliers", base)
    assert info["status"] == "ok" and ours[0] <= 2 * base[0] and ours[1] <= 2 * base[1]
    differ = (info["inliers"] != es.true_mask(s)).mean()
    print(name, "mask differs on", differ)
    assert differ <= es.MASK_LIMIT
    assert np.linalg.matrix_rank(info["E"], tol=1e-12) == 2


def test_todays_path_misses_the_bound_on_the_contaminated_scene():
    """The contrast that gives the fixture its meaning: the plain fit of every n // 100-th match of the scene with 30 %
    wrong pairs is (0.15, 1.33) rad off, against (1.2e-3, 2.7e-3) for the same fit on the true inliers."""
    s = es.end_to_end("wrong_30")
    assert abs(s["wrong"].mean() - 0.3) < 1e-9
    today, base = er.pose_error(_today(s), s["R"], s["t"]), er.pose_error(_today(s, ~s["wrong"]), s["R"], s["t"])
    print("today", today, "on the true inliers", base)
    assert today[0] > 2 * base[0] and today[1] > 2 * base[1]


def test_the_default_is_todays_path():
    for fn in (eg.EssentialMatrixStereo.__init__, eg.EssentialMatrixStereo.from_stereo):
        assert inspect.signature(fn).parameters["robust"].default is None
    sig = inspect.signature(eg.find_essential_matrix).parameters
    assert [(k, p.default) for k, p in sig.items()][3:] == [("K2", None), ("threshold", 1.0), ("hypotheses", 1024), ("seed", 0),
                                                            ("refine", True), ("return_info", False)]
    # the fit itself is what it was: the helper that now forces the rank is the three lines it replaced
    s = es.end_to_end("clean")
    a, b = eg.uvs_to_xyz_noramls(s["uvs1"][::10], s["K1"]), eg.uvs_to_xyz_noramls(s["uvs2"][::10], s["K2"])
    (x1, y1, z1), (x2, y2, z2) = a.T, b.T
    A = np.stack([x1 * x2, x2 * y1, z1 * x2, x1 * y2, y1 * y2, z1 * y2, x1 * z2, y1 * z2, z1 * z2], 1)
    U, S, Vt = np.linalg.svd(np.linalg.svd(A)[2][-1].reshape(3, 3))
    S[2] = 0
    assert np.array_equal(eg.compute_essential_matrix(a, b), np.dot(U, np.dot(np.diag(S), Vt)))
    assert epipolar_ref.E_distance(eg.compute_essential_matrix(a, b), er.force_rank2(np.linalg.svd(A)[2][-1].reshape(3, 3))) == 0


def test_entries_refuse_bad_arguments_and_fail_loudly_without_a_device():
    import torch
    from calibrating_amd import _native
    lib = _native.lib()
    assert lib.camd_essential_moments_blocks(1) == 1 and lib.camd_essential_moments_blocks(257) == 2
    assert lib.camd_essential_moments_blocks(10 ** 7) == 1024
    k = np.eye(3).ravel()
    A = 0x7000000000  # a made-up, aligned device address: never dereferenced
    rows = (A, A + (1 << 20), _native.VALUE_F64, 8, 2, 2, k.ctypes.data, k.ctypes.data)
    bad = [lib.camd_essential_hypotheses(*rows[:3], 7, *rows[4:], 0, 4, A, A, None),
           lib.camd_essential_hypotheses(*rows[:4], 1, 2, *rows[6:], 0, 4, A, A, None),
           lib.camd_essential_hypotheses(*rows, 0, 0, A, A, None),
           lib.camd_essential_hypotheses(*rows, 0, 4, None, A, None),
           lib.camd_essential_score(*rows, A, 4, 0.0, A, A, None),
           lib.camd_essential_score(*rows, A, (1 << 20) + 1, 1e-6, A, A, None),
           lib.camd_essential_moments(*rows, None, 1e-6, A, A, A, None),
           lib.camd_essential_moments(*rows, A, float("nan"), A, A, A, None)]
    assert bad == [_native.CAMD_ERR_BAD_ARG] * len(bad)
    if torch.cuda.is_available():
        return
    assert lib.camd_essential_hypotheses(*rows, 0, 4, A, A, None) == _native.CAMD_ERR_NO_DEVICE
    assert lib.camd_essential_score(*rows, A, 4, 1e-6, A, A, None) == _native.CAMD_ERR_NO_DEVICE
    assert lib.camd_essential_moments(*rows, A, 1e-6, A, A, A, None) == _native.CAMD_ERR_NO_DEVICE
    s = es.end_to_end("clean")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eg.find_essential_matrix(s["uvs1"], s["uvs2"], s["K1"], s["K2"])


REFUSALS = {
    "few": lambda s: dict(uvs1=s["uvs1"][:7], uvs2=s["uvs2"][:7]),
    "rows": lambda s: dict(uvs2=s["uvs2"][:-1]),
    "shape": lambda s: dict(uvs1=np.zeros((1000, 3))),
    "dtype": lambda s: dict(uvs2=s["uvs2"].astype(np.float32)),
    "integers": lambda s: dict(uvs1=s["uvs1"].astype(np.int64), uvs2=s["uvs2"].astype(np.int64)),
    "no_hypotheses": lambda s: dict(hypotheses=0),
    "too_many_hypotheses": lambda s: dict(hypotheses=(1 << 20) + 1),
    "zero_threshold": lambda s: dict(threshold=0.0),
    "negative_threshold": lambda s: dict(threshold=-1.0),
    "nan_threshold": lambda s: dict(threshold=float("nan")),
    "nan_K": lambda s: dict(K1=np.where(np.eye(3) > 0, np.nan, s["K1"])),
    "inf_K2": lambda s: dict(K2=np.where(s["K2"] != 0, np.inf, 0.0)),
    "singular_K": lambda s: dict(K1=np.zeros((3, 3))),
    "nan_coordinate": lambda s: dict(uvs1=np.where(np.arange(2000).reshape(1000, 2) == 777, np.nan, s["uvs1"])),
    "inf_coordinate": lambda s: dict(uvs2=np.where(np.arange(2000).reshape(1000, 2) == 1999, np.inf, s["uvs2"])),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refused_before_the_device_is_touched(name):
    """ValueError, not the RuntimeError of a missing device or library: nothing was uploaded or queued"""
    s = es.end_to_end("clean")
    kw = dict(uvs1=s["uvs1"], uvs2=s["uvs2"], K1=s["K1"], K2=s["K2"])
    kw.update(REFUSALS[name](s))
    with pytest.raises(ValueError):
        eg.find_essential_matrix(**kw)
    if name in ("few", "rows", "nan_coordinate"):
        with pytest.raises(ValueError):
            eg.EssentialMatrixStereo(kw["uvs1"], kw["uvs2"], K1=kw["K1"], K2=kw["K2"], xy1=s["xy1"], xy2=s["xy2"], robust=True)
