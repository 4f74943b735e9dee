"""``find_essential_matrices`` on the GPU (-m gpu): every field of every pair of a batch bit for bit against
``find_essential_matrix`` on that pair alone, and the batch's stage outputs against the NumPy restatement
(tests/essential_ref.py) called pair by pair.  Plain imports: a missing feature fails."""
import numpy as np
import pytest
import torch

import calibrating_amd as ca
from calibrating_amd import epipolar_geometry as eg

import essential_batch_cases as ebc
import essential_cases as es
import essential_ref as er

pytestmark = pytest.mark.gpu

STATUS = {"ok": 0, "degenerate": 1}
_SINGLE = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def batched(b, conv=lambda a: a, **kw):
    return ca.find_essential_matrices(b["K"], b["pairs"], conv(b["uvs_a"]), conv(b["uvs_b"]), b["counts"], **kw)


def single(b, p, **kw):
    """find_essential_matrix on pair p of the batch alone"""
    rows, (va, vb) = ebc.rows_of(b, p), b["pairs"][p]
    return eg.find_essential_matrix(b["uvs_a"][rows], b["uvs_b"][rows], b["K"][va], b["K"][vb], return_info=True, **kw)


def single_of_the_batch(dtype, hypotheses, refine, p):
    """the single call's answer for a pair of THE batch, computed once and shared"""
    key = (dtype, hypotheses, refine, p)
    if key not in _SINGLE:
        _SINGLE[key] = single(ebc.batch(dtype), p, hypotheses=hypotheses, seed=ebc.SEED, refine=refine)
    return _SINGLE[key]


def assert_pair_equals(res, b, p, want, inliers=None):
    rows = ebc.rows_of(b, p)
    inl = res["inliers"] if inliers is None else inliers
    assert res["status"][p] == STATUS[want["status"]], p
    assert res["E"][p].tobytes() == np.asarray(want["E"], np.float64).tobytes(), p
    assert np.array_equal(inl[rows], want["inliers"]), p
    for key in ("n_inliers", "hypothesis", "hypothesis_inliers", "refined"):
        assert res[key][p] == want[key], (p, key)


@pytest.mark.parametrize("dtype", ("float64", "float32"))
@pytest.mark.parametrize("refine", (True, False))
@pytest.mark.parametrize("hypotheses", ebc.HYPOTHESES)
def test_every_field_of_every_pair_equals_the_single_call_bit_for_bit(hypotheses, refine, dtype):
    b = ebc.batch(dtype)
    res = batched(b, hypotheses=hypotheses, seed=ebc.SEED, refine=refine)
    P, M = len(b["counts"]), len(b["uvs_a"])
    assert res["E"].shape == (P, 3, 3) and res["E"].dtype == np.float64
    assert isinstance(res["inliers"], np.ndarray) and res["inliers"].dtype == np.bool_ and res["inliers"].shape == (M,)
    for key in ("n_inliers", "hypothesis", "hypothesis_inliers", "status"):
        assert res[key].shape == (P,) and res[key].dtype.kind == "i", key
    assert res["refined"].shape == (P,) and res["refined"].dtype == np.bool_
    for p, n in enumerate(ebc.SIZES):
        if n < 8:
            assert res["status"][p] == 2 and not res["E"][p].any() and not res["inliers"][ebc.rows_of(b, p)].any()
            assert res["n_inliers"][p] == 0 and not res["refined"][p]
        else:
            assert_pair_equals(res, b, p, single_of_the_batch(dtype, hypotheses, refine, p))
    print("H=%d refine=%s %s: status %s, inliers %s" % (hypotheses, refine, dtype, res["status"].tolist(), res["n_inliers"].tolist()))
    assert (res["status"][[p for p, n in enumerate(ebc.SIZES) if n >= 63]] == 0).all() or hypotheses == 1


def test_the_seven_row_and_the_empty_pair():
    b = ebc.batch("float64")
    res = batched(b, hypotheses=64, seed=ebc.SEED)
    for p in (ebc.SIZES.index(0), ebc.SIZES.index(7)):
        assert res["status"][p] == 2 and not res["E"][p].any()
    rows = ebc.rows_of(b, ebc.SIZES.index(7))
    assert rows.stop - rows.start == 7 and not res["inliers"][rows].any()
    assert 0 < ebc.SIZES.index(0) < len(ebc.SIZES) - 1 and 0 < ebc.SIZES.index(7) < len(ebc.SIZES) - 1


def test_a_pair_alone_permuted_pairs_and_two_runs():
    b = ebc.batch("float64")
    kw = dict(hypotheses=65, seed=ebc.SEED)
    res = batched(b, **kw)
    again = batched(b, **kw)
    for key in res:
        assert res[key].tobytes() == again[key].tobytes(), key
    for p in (2, 5, 8):  # alone in a batch of one
        one = batched(ebc.reordered(b, [p]), **kw)
        assert one["E"][0].tobytes() == res["E"][p].tobytes() and np.array_equal(one["inliers"], res["inliers"][ebc.rows_of(b, p)])
        for key in ("n_inliers", "hypothesis", "hypothesis_inliers", "refined", "status"):
            assert one[key][0] == res[key][p], (p, key)
    order = np.random.default_rng(3).permutation(len(ebc.SIZES)).tolist()
    c = ebc.reordered(b, order)
    perm = batched(c, **kw)
    for k, p in enumerate(order):
        assert perm["E"][k].tobytes() == res["E"][p].tobytes()
        assert np.array_equal(perm["inliers"][ebc.rows_of(c, k)], res["inliers"][ebc.rows_of(b, p)])
        for key in ("n_inliers", "hypothesis", "hypothesis_inliers", "refined", "status"):
            assert perm[key][k] == res[key][p], (p, key)


@pytest.mark.parametrize("dtype", ("float64", "float32"))
def test_stage_outputs_equal_the_restatement_pair_by_pair(dtype):
    b = ebc.batch(dtype, ebc.STAGE_SIZES, ebc.STAGE_VIEW_PAIRS)
    H, threshold = ebc.STAGE_HYPOTHESES, es.THRESHOLD
    pairs, counts, table = eg._essential_batch_checks(b["K"], b["pairs"], b["uvs_a"], b["uvs_b"], b["counts"], threshold, H)
    for lds_sum in (1, 0):
        samples, Es, hcounts, winner, batch, keep = eg._essential_batch_stages(b["uvs_a"], b["uvs_b"], counts, table.copy(), H, ebc.SEED,
                                                                               lds_sum=lds_sum)
        take = counts >= 8
        mask, sums = eg._essential_batch_moments(batch, counts, take, winner, 11)
        samples, Es, hcounts, winner, mask, sums = (t.cpu().numpy() for t in (samples, Es, hcounts, winner, mask, sums))
        assert samples.dtype == np.int32 and hcounts.dtype == np.int32 and hcounts.shape == (len(counts), H)
        for p, n in enumerate(ebc.STAGE_SIZES):
            rows, (va, vb) = ebc.rows_of(b, p), b["pairs"][p]
            if n < 8:  # marked, and nothing is drawn or counted
                assert (samples[p] == -1).all() and not Es[p].any() and not hcounts[p].any() and not sums[p].any()
                continue
            ua, ub, Ka, Kb = b["uvs_a"][rows], b["uvs_b"][rows], b["K"][va], b["K"][vb]
            want_samples, want_Es = er.hypotheses(ua, ub, Ka, Kb, H, ebc.SEED)
            assert np.array_equal(samples[p], want_samples) and Es[p].tobytes() == want_Es.tobytes(), p
            same = er.find(ua, ub, Ka, Kb, threshold, H, ebc.SEED, Es=Es[p])
            assert np.array_equal(hcounts[p], same["counts"]), (p, lds_sum)
            assert int(winner[p, 9]) == same["hypothesis"] and int(winner[p, 10]) == same["hypothesis_inliers"]
            assert np.array_equal(winner[p, :9], Es[p, same["hypothesis"]])
            assert np.array_equal(mask[rows] != 0, same["hypothesis_mask"]) and sums[p].tobytes() == same["hypothesis_sums"].tobytes(), p
        del keep


def test_tensors_in_tensors_out_and_a_strided_view_is_read_in_place():
    b = ebc.batch("float64")
    kw = dict(hypotheses=65, seed=ebc.SEED)
    want = batched(b, **kw)
    got = batched(b, _cuda, **kw)
    assert isinstance(got["inliers"], torch.Tensor) and got["inliers"].dtype == torch.bool and got["inliers"].is_cuda
    assert isinstance(got["E"], np.ndarray) and isinstance(got["status"], np.ndarray)
    assert np.array_equal(got["inliers"].cpu().numpy(), want["inliers"])
    for key in ("E", "n_inliers", "hypothesis", "hypothesis_inliers", "refined", "status"):
        assert got[key].tobytes() == want[key].tobytes(), key
    rng = np.random.default_rng(9)
    M = len(b["uvs_a"])
    wide_a, wide_b = _cuda(rng.uniform(-1e6, 1e6, (M, 5))), _cuda(rng.uniform(-1e6, 1e6, (M, 3)))
    wide_a[:, 1:3], wide_b[:, 1:3] = _cuda(b["uvs_a"]), _cuda(b["uvs_b"])
    va, vb = wide_a[:, 1:3], wide_b[:, 1:3]
    assert eg._EssentialRows._in_place(va) == (va, 5) and eg._EssentialRows._in_place(vb)[1] == 3
    view = ca.find_essential_matrices(b["K"], b["pairs"], va, vb, b["counts"], **kw)
    assert isinstance(view["inliers"], torch.Tensor) and np.array_equal(view["inliers"].cpu().numpy(), want["inliers"])
    for key in ("E", "n_inliers", "hypothesis", "hypothesis_inliers", "refined", "status"):
        assert view[key].tobytes() == want[key].tobytes(), key
    bad = _cuda(b["uvs_a"])
    bad[5000, 0] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        ca.find_essential_matrices(b["K"], b["pairs"], bad, _cuda(b["uvs_b"]), b["counts"], **kw)


def test_a_degenerate_pair_among_good_ones():
    b = ebc.with_degenerate()
    res = batched(b, hypotheses=5, seed=ebc.SEED)
    assert res["status"].tolist() == [0, 1, 0] and not res["E"][1].any() and res["n_inliers"][1] == 0
    assert not res["inliers"][ebc.rows_of(b, 1)].any() and not res["refined"][1]
    for p in range(3):  # the degenerate pair as the single call reports it, the others as without it
        assert_pair_equals(res, b, p, single(b, p, hypotheses=5, seed=ebc.SEED))
    without = batched(ebc.reordered(b, [0, 2]), hypotheses=5, seed=ebc.SEED)
    assert without["E"][0].tobytes() == res["E"][0].tobytes() and without["E"][1].tobytes() == res["E"][2].tobytes()
    assert np.array_equal(without["inliers"], np.concatenate([res["inliers"][ebc.rows_of(b, 0)], res["inliers"][ebc.rows_of(b, 2)]]))


def test_the_estimate_keyword_builds_the_robust_rig_without_estimating():
    s = es.end_to_end("wrong_30")
    info = eg.find_essential_matrix(s["uvs1"], s["uvs2"], s["K1"], s["K2"], return_info=True)
    a = ca.EssentialMatrixStereo(s["uvs1"], s["uvs2"], s["K1"], s["K2"], xy1=s["xy1"], xy2=s["xy2"], robust=True)
    b = ca.EssentialMatrixStereo(s["uvs1"], s["uvs2"], s["K1"], s["K2"], xy1=s["xy1"], xy2=s["xy2"], estimate=info)
    assert np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t) and a.candidate == b.candidate
    assert np.array_equal(a.epipolar["E"], b.epipolar["E"]) and np.array_equal(a.epipolar["zs1"], b.epipolar["zs1"])
    assert np.array_equal(b.epipolar["inliers"], info["inliers"]) and b.epipolar["n_inliers"] == info["n_inliers"]
    with pytest.raises(ValueError, match="determine"):
        ca.EssentialMatrixStereo(s["uvs1"], s["uvs2"], s["K1"], s["K2"], xy1=s["xy1"], xy2=s["xy2"], estimate=dict(info, status="degenerate"))
