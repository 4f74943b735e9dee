"""ReconstructionExtrinsics on the GPU (-m gpu): the batched triple matching against the single call bit for bit, the
depth-row kernels against NumPy (pack and scale bit for bit, the sum within the bound of its documented reduction
shape), and the whole class against the reference's own output (tests/golden/reference_reconstruction.npz): every decision
and every integer equal, T_re and depths within SENS_FACTOR x the reference's recorded one-ulp sensitivity.  Plain
imports: a missing feature fails."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import calibrating_amd as ca
from calibrating_amd import _native, epipolar_geometry as eg, reconstruction_epipolar_geometry as reg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import reference_cases as rc  # noqa: E402
import epipolar_cases as ec  # noqa: E402
import epipolar_ref as er  # noqa: E402
import reconstruction_cases as rcc  # noqa: E402
from test_epipolar_cpu import same_as_fixture  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
Z_STEP = 8  # make_reconstruction_golden.Z_STEP


@pytest.fixture(scope="module")
def fx():
    f = rcc.load_fixture()
    assert f is not None, "tests/golden/reference_reconstruction.npz is missing"
    return f


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    assert isinstance(t, torch.Tensor) and t.is_cuda, type(t)
    return t.cpu().numpy()


_runs = {}


def reconstruct(fx, name):
    """(object, viewds, true poses) of a case, computed once and left unchanged."""
    if name not in _runs:
        viewds, flowds, Ts = rcc.case(name, int(fx[name + "/seed"]))
        _runs[name] = (ca.ReconstructionExtrinsics(viewds, flowds=flowds), viewds, Ts)
    return _runs[name]


_pairs = {}


def ten_triples_pairs(fx):
    """The (uvs_main of jj, uvs_main of kk) of every triple of ``ten_triples``: shared objects, as the class passes them."""
    if not _pairs:
        viewds, flowds, _ = rcc.case("ten_triples", int(fx["ten_triples/seed"]))
        set2ds = eg.build_set2ds_by_flowds(viewds, flowds)
        sizes = {k: len(v["uvs_i"]) for k, v in set2ds.items()}
        out = []
        for set3, (ii, jj, kk), _ in reg.plan_triples(list(viewds), sizes):
            out.append(tuple(set2ds[frozenset((o, ii))]["uvs_" + "ij"[tuple(sorted((o, ii))).index(ii)]] for o in (jj, kk)))
        _pairs["p"] = out
    return _pairs["p"]


def _equal_matches(got, want, host=lambda a: a):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for k in w:
            assert _same(host(g[k]), host(w[k])), k


# ---- the batch alone ---------------------------------------------------------------------------------------------------
def test_batch_equals_the_single_call_bit_for_bit(fx):
    pairs = list(ten_triples_pairs(fx))
    assert len(pairs) == 10 and len({id(s) for p in pairs for s in p}) < 20, "sets are shared between triples"
    f32 = ec.match_case("float32_100k")[:2]
    neg = ec.match_case("half_and_negative")[:2]
    few = ec.match_case("too_few")[:2]
    pairs += [f32, neg, few, (f32[1], f32[0])]
    want = [eg.matching_uvs_in_one_img(a, b) for a, b in pairs]
    got = eg.matching_uvs_in_one_img_batch(pairs)
    _equal_matches(got, want)
    assert all(isinstance(v, np.ndarray) and v.dtype == np.int64 for g in got for v in g.values())
    assert got[12] == {} and want[12] == {} and all(len(g["uv_match_idx1"]) > 20 for k, g in enumerate(got) if k != 12)
    assert er.matching(*neg)["uv_match_idx1"].tolist() == got[11]["uv_match_idx1"].tolist()  # ... and the restatement's
    # tensors in -> tensors out, the same bits; identical calls give identical bits
    cache = {}
    dev = [tuple(cache.setdefault(id(s), _cuda(s)) for s in p) for p in pairs]
    got_dev = eg.matching_uvs_in_one_img_batch(dev)
    _equal_matches([{k: _np(v) for k, v in g.items()} for g in got_dev], want)
    _equal_matches([{k: _np(v) for k, v in g.items()} for g in eg.matching_uvs_in_one_img_batch(dev)], want)
    # other cell sizes and thresholds
    for d, k in ((0.5, 10), (3, 2000)):
        _equal_matches(eg.matching_uvs_in_one_img_batch(pairs[:10] + [neg], d, k), [eg.matching_uvs_in_one_img(a, b, d, k) for a, b in pairs[:10] + [neg]])
    assert eg.matching_uvs_in_one_img_batch([]) == []


def test_batch_below_the_threshold_gives_an_empty_dict(fx):
    pairs = ten_triples_pairs(fx)
    counts = [len(m["uv_match_idx1"]) for m in eg.matching_uvs_in_one_img_batch(pairs)]
    assert counts == [len(er.matching(a, b)["uv_match_idx1"]) for a, b in pairs]
    k = sorted(counts)[5]
    got = eg.matching_uvs_in_one_img_batch(pairs, MIN_MATCHED_PIXELS=k)
    assert [bool(g) for g in got] == [c >= k for c in counts] and not all(got) and any(got)


def test_batch_in_several_passes_gives_the_same_bits(fx):
    pairs = ten_triples_pairs(fx)
    want = eg.matching_uvs_in_one_img_batch(pairs)
    window = 66 * 50  # cells of one 64 x 48 view's window at most: rint(-0.5 .. 64.5) x rint(-0.5 .. 48.5)
    for cap in (2 * window, 3 * window, 7 * window):  # one pair per pass ... a few main views per pass
        _equal_matches(eg.matching_uvs_in_one_img_batch(pairs, max_cells=cap), want)
    with pytest.raises(ValueError, match="max_cells"):
        eg.matching_uvs_in_one_img_batch(pairs, max_cells=window)
    with pytest.raises(ValueError, match="at least one point"):
        eg.matching_uvs_in_one_img_batch([(pairs[0][0], np.zeros((0, 2)))])


# ---- pack, column sum, column scale ------------------------------------------------------------------------------------
def test_pack_sum_scale_kernels():
    lib, st = _native.lib(), _native.current_stream()
    rng = np.random.default_rng(21)
    n1, n2, total = 70001, 513, 70001 + 513 + 7
    uv64, uv32 = rng.uniform(-5, 700, (n1, 2)), rng.uniform(-5, 700, (n2, 2)).astype(np.float32)
    z1, z2 = rng.normal(3.0, 2.0, n1), rng.normal(3.0, 2.0, n2)
    buf = torch.full((total, 4), -7.0, dtype=torch.float64, device="cuda")
    # prepending is a choice of offsets: the second block goes in front of the first
    assert lib.camd_uvzi_pack(_cuda(uv64).data_ptr(), _native.VALUE_F64, _cuda(z1).data_ptr(), n1, 5.0, buf.data_ptr(), total, n2, st) == 0
    assert lib.camd_uvzi_pack(_cuda(uv32).data_ptr(), _native.VALUE_F32, _cuda(z2).data_ptr(), n2, 11.0, buf.data_ptr(), total, 0, st) == 0
    want = np.concatenate([np.concatenate((uv32, z2[:, None], [[11]] * n2), -1), np.concatenate((uv64, z1[:, None], [[5]] * n1), -1),
                           np.full((7, 4), -7.0)])
    assert want.dtype == np.float64 and _same(_np(buf), want)
    bad = _native.CAMD_ERR_BAD_ARG
    assert lib.camd_uvzi_pack(_cuda(uv32).data_ptr(), _native.VALUE_F32, _cuda(z2).data_ptr(), n2, 1.0, buf.data_ptr(), total, total - n2 + 1, st) == bad
    assert lib.camd_uvzi_pack(_cuda(uv32).data_ptr(), _native.VALUE_U8, _cuda(z2).data_ptr(), n2, 1.0, buf.data_ptr(), total, 0, st) == bad
    # the sum of a strided column of a row range: within the bound of the header's reduction shape, the same bits twice
    for row0, n in ((0, n1 + n2), (n2, n1), (3, 1), (0, 257)):
        m, d = er.reduction_shape(n)
        assert lib.camd_column_sum_blocks(n) == min(max(-(-n // 256), 1), 1024)
        z = want[row0:row0 + n, 2]
        got = reg._column_sum(buf, row0, n)
        exact, exact_abs = er.exact_mean(z)
        err, bound = abs(got - float(exact * n)), (m + d) * U * float(exact_abs * n)
        print("column sum n=%d m=%d d=%d: |sum - exact| = %.3g, bound %.3g" % (n, m, d, err, bound))
        assert err <= bound and reg._column_sum(buf, row0, n) == got
    assert reg._column_sum(buf, n2, n1, 3) == 5.0 * n1 and reg._column_sum(buf, 0, n2, 3) == 11.0 * n2
    part, out = torch.empty(1024, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda")
    for args in ((total, 4, 2, 1, total), (total, 4, 4, 0, 5), (total, 4, 2, 0, 0), (total, 4, -1, 0, 5)):
        assert lib.camd_column_sum(buf.data_ptr(), *args, part.data_ptr(), out.data_ptr(), st) == bad
    # the scale: one multiply per element, NumPy's *=, on a row range; nothing else moves
    rate = 1 / np.float64(3.0000001)
    reg._column_scale(buf, n2, n1, rate)
    want[n2:n2 + n1, 2] *= rate
    assert _same(_np(buf), want)
    view = buf[5:300]  # a view's slice, as change_scale passes it
    reg._column_scale(view, 0, 295, 2.0)
    want[5:300, 2] *= 2.0
    assert _same(_np(buf), want)
    assert lib.camd_column_scale(buf.data_ptr(), total, 4, 2, total - 3, 4, 2.0, st) == bad


# ---- the whole class against the reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", rcc.REFERENCE_SUCCEEDS)
def test_class_equals_the_reference(fx, name):
    re, viewds, Ts = reconstruct(fx, name)
    p, f = name + "/", ec.SENS_FACTOR
    assert re.viewds is viewds and re.cfg == {} and re.flowds is not None and sorted(map(sorted, re.set2ds)) == sorted(map(sorted, {frozenset(k) for k in re.flowds}))
    assert sorted(re.seed) == fx[p + "seed3"].tolist()
    assert [[i] + sorted(s) for i, s in re.propagate_path] == fx[p + "propagate_path"].tolist()
    assert [rcc.triple_name(s) for s in re.set3ds] == [str(s) for s in fx[p + "triples"]]
    assert [d["idx_sorted"] for d in re.set3ds.values()] == fx[p + "idx_sorted"].tolist()
    assert [list(k) for k in re.stereods] == fx[p + "stereos"].tolist()
    assert all(isinstance(s, ca.EssentialMatrixStereo) for s in re.stereods.values())
    for s, d in re.set3ds.items():
        assert sorted(d) == ["idx_sorted", "not_include_uvsn", "uv_match_idx1", "uv_match_idx2", "uvsd"]
        assert sorted(d["uvsd"]) == sorted(d["idx_sorted"][1:]) and sorted(d["not_include_uvsn"]) == sorted(s)
        for key in ("uv_match_idx1", "uv_match_idx2"):
            assert isinstance(d[key], np.ndarray) and same_as_fixture(fx, "%s%s/%s" % (p, rcc.triple_name(s), key), d[key])
    if name == "rerooted":
        assert len(fx[p + "rerooted"]) >= 1
    for k, d in viewds.items():
        uvzis, T = d["uvzis"], d["T_re"]
        assert isinstance(uvzis, np.ndarray) and uvzis.dtype == np.float64 and uvzis.shape == (int(fx["%sview%d/rows" % (p, k)]), 4)
        assert isinstance(T, np.ndarray) and T.dtype == np.float64 and T.shape == (4, 4)
        assert rc.sha(np.ascontiguousarray(uvzis[:, [0, 1, 3]])) == str(fx["%sview%d/uvi_sha" % (p, k)]), "u, v, view columns / row order"
        dz = float(np.abs(uvzis[::Z_STEP, 2] - fx["%sview%d/z" % (p, k)]).max())
        want = fx["%sview%d/T_re" % (p, k)]
        dT, dR = float(np.abs(T - want).max()), float(np.abs(T[:3, :3] - want[:3, :3]).max())
        print("%s view %d: |T_re - reference| = %.3g (rotation %.3g; sens %.3g), |z - reference| = %.3g (sens %.3g)" % (
            name, k, dT, dR, fx[p + "sens_T_re"], dz, fx[p + "sens_z"]))
        assert dz <= f * float(fx[p + "sens_z"])
        assert float(np.abs(T[:3, 3] - want[:3, 3]).max()) <= f * float(fx[p + "sens_T_re"])
        assert dR <= max(f * float(fx[p + "sens_T_re"]), ec.R_ULP)
    err = rcc.rotation_error({k: d["T_re"] for k, d in viewds.items()}, Ts)
    print("%s: rotation error against the truth %.3g (reference %.3g)" % (name, err, fx[p + "ref_rot_error"]))
    assert err <= f * float(fx[p + "ref_rot_error"])


def _mean_one_bound(viewds):
    """Bound of |mean of all depths - 1| after the constructor.  The sum S^ the kernel returns has relative error <= (m + d) u
    (all depths are positive, so sum |z| = S); the mean S^ / n, the rate 1 / mean and each product z * rate round once more
    (3 u), and math.fsum / the division by n that measure it here add 2 u."""
    n = sum(len(d["uvzis"]) for d in viewds.values())
    m, d = er.reduction_shape(n)
    return n, (m + d + 5) * U


def test_deferred_seed_completes(fx):
    assert str(fx["deferred_seed/raises"]) == "KeyError: 'T_re'"
    re, viewds, Ts = reconstruct(fx, "deferred_seed")
    reached = [k for k, d in viewds.items() if "T_re" in d and "uvzis" in d]
    assert len(reached) >= 6
    allowed = ec.SENS_FACTOR * max(float(fx[n + "/ref_rot_error"]) for n in rcc.REFERENCE_SUCCEEDS)
    err = rcc.rotation_error({k: d["T_re"] for k, d in viewds.items()}, Ts)
    print("deferred_seed: rotation error against the truth %.3g, allowed %.3g" % (err, allowed))
    assert err <= allowed
    zs = np.concatenate([d["uvzis"][:, 2] for d in viewds.values()])
    assert (zs > 0).all()
    n, bound = _mean_one_bound(viewds)
    mean = math.fsum(zs) / n
    print("deferred_seed: |mean depth - 1| = %.3g over %d rows, bound %.3g" % (abs(mean - 1), n, bound))
    assert abs(mean - 1) <= bound
    # view 0 at z = -(its mean depth): the mean through the same reduction (m + d + 1 roundings on mean |z|), then
    # T0_target @ inv(T_re[0]) @ T_re[0] on the host: 4 x 4 products and an inverse of a rigid motion with entries below 2,
    # 64 u on entries of that size
    z0 = viewds[0]["uvzis"][:, 2]
    m, d = er.reduction_shape(len(z0))
    mean0 = math.fsum(z0) / len(z0)
    T0 = viewds[0]["T_re"]
    bound0 = (m + d + 3) * U * mean0 + 64 * U * 2
    print("deferred_seed: |T_re[0][2, 3] + mean depth of view 0| = %.3g, bound %.3g" % (abs(T0[2, 3] + mean0), bound0))
    assert abs(T0[2, 3] + mean0) <= bound0
    want = np.eye(4)
    want[2, 3] = -mean0
    assert np.abs(T0 - want).max() <= bound0


def test_two_groups_raises_naming_the_unreached_views(fx):
    viewds, flowds, _ = rcc.case("two_groups", int(fx["two_groups/seed"]))
    with pytest.raises(ValueError, match=r"3 views are not reached.*\[(0, 1, 2|3, 4, 5)\]$"):
        ca.ReconstructionExtrinsics(viewds, flowds=flowds)


def test_tensor_sets_in_tensors_out_and_the_loop_gives_the_same(fx):
    viewds, flowds, _ = rcc.case("ten_triples", int(fx["ten_triples/seed"]))
    host = {k: {kk: vv.astype(np.float32) for kk, vv in v.items() if kk in ("uvs_i", "uvs_j")}
            for k, v in eg.build_set2ds_by_flowds(viewds, flowds).items()}
    a = ca.ReconstructionExtrinsics(rcc.fresh(viewds), set2ds=host)
    dev = {k: {kk: _cuda(vv) for kk, vv in v.items()} for k, v in host.items()}
    b = ca.ReconstructionExtrinsics(rcc.fresh(viewds), set2ds=dev)
    c = ca.ReconstructionExtrinsics(rcc.fresh(viewds), set2ds=dev, cfg=dict(triple_stage="loop"))
    assert a.flowds is None and b.set2ds is dev and c.cfg == dict(triple_stage="loop")
    for other in (b, c):
        assert other.seed == a.seed and other.propagate_path == a.propagate_path and list(other.stereods) == list(a.stereods)
        for s, d in a.set3ds.items():
            assert other.set3ds[s]["idx_sorted"] == d["idx_sorted"]
            for key in ("uv_match_idx1", "uv_match_idx2"):
                assert _same(_np(other.set3ds[s][key]), d[key])
        for k, d in a.viewds.items():
            assert isinstance(d["uvzis"], np.ndarray) and _same(_np(other.viewds[k]["uvzis"]), d["uvzis"])
            assert isinstance(other.viewds[k]["T_re"], np.ndarray) and _same(other.viewds[k]["T_re"], d["T_re"])


def test_change_scale_and_apply_T_and_back(fx):
    viewds, flowds, _ = rcc.case("one_triple", int(fx["one_triple/seed"]))
    host = ca.ReconstructionExtrinsics(viewds, flowds=flowds)
    dev = ca.ReconstructionExtrinsics(rcc.fresh(viewds), set2ds={k: {kk: _cuda(vv) for kk, vv in v.items()} for k, v in host.set2ds.items()})
    T = np.eye(4)
    T[:3, :3] = rcc._rodrigues([0.3, -0.2, 0.5])
    T[:3, 3] = [0.7, -1.3, 0.4]
    for re, get in ((host, lambda a: a), (dev, _np)):
        before = {k: (d["T_re"].copy(), get(d["uvzis"]).copy()) for k, d in re.viewds.items()}
        assert re.change_scale(2) is re.viewds
        for k, d in re.viewds.items():
            assert _same(get(d["uvzis"])[:, 2], before[k][1][:, 2] * 2) and _same(d["T_re"][:3, 3], before[k][0][:3, 3] * 2)
            assert _same(d["T_re"][:3, :3], before[k][0][:3, :3])
        scaled = {k: d["T_re"].copy() for k, d in re.viewds.items()}
        assert re.apply_T(T) is re.viewds
        assert all(_same(d["T_re"], T @ scaled[k]) for k, d in re.viewds.items())
        with pytest.raises(AssertionError):
            re.change_scale(2, T)
        re.apply_T(np.linalg.inv(T))
        re.change_scale(0.5)
        for k, d in re.viewds.items():
            assert _same(get(d["uvzis"]), before[k][1]), "x2 and x0.5 are exact"
            tol = 4 * np.spacing(np.abs(before[k][0]).max())
            print("view %s: |T_re - before| = %.3g, 4 ulp = %.3g" % (k, np.abs(d["T_re"] - before[k][0]).max(), tol))
            assert np.abs(d["T_re"] - before[k][0]).max() <= tol
