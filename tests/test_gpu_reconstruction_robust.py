"""``ReconstructionExtrinsics(viewds, set2ds, cfg=dict(robust=...))`` on the GPU (-m gpu): matches of the reconstruction cases
in which a seeded 30 % of every pair's rows are wrong pairs (tests/essential_batch_cases.py).  The filtered pairs and every
rig's E are bit-equal to ``find_essential_matrix`` on the pair alone; the poses stay within 4 x what the CPU composition
leaves (measured by tests/golden/make_essential_batch_bound.py); without ``robust`` the same matches miss that bound."""
import numpy as np
import pytest
import torch

import calibrating_amd as ca
from calibrating_amd import epipolar_geometry as eg

import bundle_ref as ref
import epipolar_cases as ec
import essential_batch_cases as ebc
import reconstruction_cases as rc

pytestmark = pytest.mark.gpu

NAMES = ("one_triple", "ten_triples")
_CASE = {}


def case(name):
    """(viewds, Ts, the clean set2ds, the contaminated set2ds) -- computed once, shared, never written to"""
    if name not in _CASE:
        fx = rc.load_fixture()
        assert fx is not None
        viewds, flowds, Ts = rc.case(name, int(fx[name + "/seed"]))
        clean = ca.build_set2ds_by_flowds(viewds, flowds)
        _CASE[name] = (viewds, Ts, clean, ebc.contaminated(clean))
    return _CASE[name]


def errors(viewds, Ts):
    keys = sorted(viewds)
    return ref.pose_errors(np.array([viewds[k]["T_re"] for k in keys]), np.array([Ts[k] for k in keys]))


def bound(name):
    return tuple(ebc.BOUND_FACTOR * v for v in ebc.CPU_ERRORS[name])


@pytest.mark.parametrize("name", NAMES)
def test_robust_filters_every_pair_as_the_single_call_and_holds_the_poses(name):
    viewds, Ts, _, bad = case(name)
    before = {k: {kk: vv.copy() for kk, vv in d.items()} for k, d in bad.items()}
    re_ = ca.ReconstructionExtrinsics(rc.fresh(viewds), set2ds=bad, cfg=dict(robust=dict(ebc.ROBUST)))
    assert re_.set2ds_all is bad and re_.set2ds is not bad and list(re_.set2ds) == list(bad)
    assert all(set(d) == {"uvs_i", "uvs_j"} and np.array_equal(d["uvs_i"], before[k]["uvs_i"]) and np.array_equal(d["uvs_j"], before[k]["uvs_j"])
               for k, d in bad.items())  # the caller's dicts are as they were
    singles = {}
    for p, (set2, d) in enumerate(bad.items()):
        i, j = sorted(set2)
        info = eg.find_essential_matrix(d["uvs_i"], d["uvs_j"], viewds[i]["K"], viewds[j]["K"], return_info=True, **ebc.ROBUST)
        singles[(i, j)] = info
        assert info["status"] == "ok" and re_.robust["status"][p] == 0 and re_.robust["keys"][p] == (i, j)
        assert re_.robust["E"][p].tobytes() == info["E"].tobytes()
        for key, mine in (("uvs_i", d["uvs_i"]), ("uvs_j", d["uvs_j"])):
            got = re_.set2ds[set2][key]
            assert isinstance(got, np.ndarray) and got.tobytes() == mine[info["inliers"]].tobytes(), (set2, key)
    assert re_.stereods
    for (ii, jj), stereo in re_.stereods.items():
        want = singles[(ii, jj)]["E"] if ii < jj else singles[(jj, ii)]["E"].T
        assert np.asarray(stereo.epipolar["E"]).tobytes() == np.ascontiguousarray(want).tobytes(), (ii, jj)
        assert stereo.epipolar["inliers"].all() and stereo.epipolar["n_inliers"] == len(stereo.epipolar["uvs1"])
    got, most = errors(re_.viewds, Ts), bound(name)
    print("%s robust: rotation %.3g rad (bound %.3g), centre %.3g (bound %.3g)" % (name, got[0], most[0], got[1], most[1]))
    assert got[0] <= most[0] and got[1] <= most[1]
    re_.refine()
    used = int((re_.refinement["status"] == 0).sum())
    assert re_.refinement["status"].shape == (sum(len(d["uvs_i"]) for d in re_.set2ds.values()),) and used > 0  # inliers only
    after = errors(re_.viewds, Ts)
    print("%s refined: rotation %.3g rad, centre %.3g" % (name, after[0], after[1]))
    assert np.isfinite(after).all()


@pytest.mark.parametrize("name", NAMES)
def test_without_robust_the_same_matches_raise_or_miss_the_bound(name):
    viewds, Ts, _, bad = case(name)
    try:
        re_ = ca.ReconstructionExtrinsics(rc.fresh(viewds), set2ds={k: dict(d) for k, d in bad.items()})
    except (ValueError, AssertionError, KeyError, IndexError) as e:
        print("%s without robust raises %s: %s" % (name, type(e).__name__, e))
        return
    got, most = errors(re_.viewds, Ts), bound(name)
    print("%s without robust: rotation %.3g rad (bound %.3g), centre %.3g (bound %.3g)" % (name, got[0], most[0], got[1], most[1]))
    assert re_.robust is None and (got[0] > most[0] or got[1] > most[1])


@pytest.mark.parametrize("name", NAMES)
def test_without_robust_the_clean_case_is_what_it_was(name):
    """the constructor without cfg["robust"] against the existing fixture, as test_gpu_bundle.py does; cfg["robust"] = None is
    the same constructor bit for bit"""
    fx = rc.load_fixture()
    viewds, Ts, clean, _ = case(name)
    plain = ca.ReconstructionExtrinsics(rc.fresh(viewds), set2ds={k: dict(d) for k, d in clean.items()})
    none = ca.ReconstructionExtrinsics(rc.fresh(viewds), set2ds={k: dict(d) for k, d in clean.items()}, cfg=dict(robust=None))
    assert plain.robust is None and none.robust is None and plain.set2ds is plain.set2ds_all
    for k, d in plain.viewds.items():
        want, sens = fx["%s/view%d/T_re" % (name, k)], ec.SENS_FACTOR * float(fx[name + "/sens_T_re"])
        assert d["uvzis"].shape == (int(fx["%s/view%d/rows" % (name, k)]), 4)
        assert np.abs(d["T_re"][:3, 3] - want[:3, 3]).max() <= sens and np.abs(d["T_re"][:3, :3] - want[:3, :3]).max() <= max(sens, ec.R_ULP)
        assert np.array_equal(none.viewds[k]["T_re"], d["T_re"]) and np.array_equal(none.viewds[k]["uvzis"], d["uvzis"])
    assert all(np.array_equal(plain.stereods[k].epipolar["E"], none.stereods[k].epipolar["E"]) for k in plain.stereods)
    assert all("inliers" not in s.epipolar for s in plain.stereods.values())


def test_tensor_matches_are_filtered_on_the_device_and_give_the_same():
    viewds, Ts, _, bad = case("one_triple")
    dev = torch.device("cuda", torch.cuda.current_device())
    on_device = {k: {kk: torch.from_numpy(vv).to(dev) for kk, vv in d.items()} for k, d in bad.items()}
    a = ca.ReconstructionExtrinsics(rc.fresh(viewds), set2ds=bad, cfg=dict(robust=dict(ebc.ROBUST)))
    b = ca.ReconstructionExtrinsics(rc.fresh(viewds), set2ds=on_device, cfg=dict(robust=dict(ebc.ROBUST)))
    for set2 in bad:
        for key in ("uvs_i", "uvs_j"):
            got = b.set2ds[set2][key]
            assert isinstance(got, torch.Tensor) and got.device == dev and np.array_equal(got.cpu().numpy(), a.set2ds[set2][key])
    for k in a.viewds:
        assert np.array_equal(a.viewds[k]["T_re"], b.viewds[k]["T_re"])
        assert isinstance(b.viewds[k]["uvzis"], torch.Tensor) and np.array_equal(b.viewds[k]["uvzis"].cpu().numpy(), a.viewds[k]["uvzis"])
