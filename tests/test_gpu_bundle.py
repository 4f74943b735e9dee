"""``bundle_adjust_pairs`` and ``ReconstructionExtrinsics.refine`` on the GPU (csrc/bundle.hip) against the NumPy restatement
tests/bundle_ref.py: the start points and the status bit for bit, the solution within the bounds of
tests/golden/bundle_tolerance.json (8 times the restatement's own disagreement under a change of summation order)."""
import numpy as np
import pytest

import calibrating_amd as ca

import bundle_cases as bc
import bundle_ref as ref
import bundle_tolerance as tolerance
import epipolar_cases as ec
import reconstruction_cases as rc

pytestmark = pytest.mark.gpu

_GOT = {}


def call(c, **kw):
    return ca.bundle_adjust_pairs(c["K"], c["T0"], c["pairs"], c["uvs_a"], c["uvs_b"], c["counts"], **kw)


def got(name, noisy=True):
    """the GPU's result of a case, computed once"""
    if (name, noisy) not in _GOT:
        _GOT[name, noisy] = call(tolerance.solved(name, noisy)[0], return_start=True)
    return _GOT[name, noisy]


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in ("T", "points", "status", "pair_error")) and \
        all(a[k] == b[k] for k in ("retval", "cost0", "cost", "iterations", "evaluations", "anchor"))


@pytest.mark.parametrize("noisy", (False, True))
@pytest.mark.parametrize("name", bc.NAMES)
def test_start_and_status_equal_the_restatement_bit_for_bit(name, noisy):
    _, want = tolerance.solved(name, noisy)
    g = got(name, noisy)
    assert g["status"].dtype == np.int32 and np.array_equal(g["status"], want["status"])
    assert np.array_equal(g["start"], want["start"], equal_nan=True)


@pytest.mark.parametrize("name", bc.NAMES)
def test_solution_within_the_measured_bounds(name):
    rec = tolerance.load()
    _, want = tolerance.solved(name, True)
    g = got(name, True)
    d = tolerance.difference(g, want)
    print("%s: |gpu - restatement| %s, bounds %s; evaluations %d / %d" % (name, d, rec["bound"], g["evaluations"], want["evaluations"]))
    assert np.array_equal(g["status"], want["status"]) and g["anchor"] == want["anchor"]
    assert np.array_equal(np.isnan(g["points"]), np.isnan(want["points"])) and np.array_equal(np.isnan(g["pair_error"]), np.isnan(want["pair_error"]))
    assert all(d[k] <= rec["bound"][k] for k in tolerance.KEYS), d
    assert g["evaluations"] < ref.MAX_EVALUATIONS / 2 and g["cost"] <= g["cost0"]


def test_two_runs_give_identical_bits():
    c, _ = tolerance.solved("borders", True)
    assert same_bits(call(c), got("borders"))


def test_bad_rows_and_threshold_equal_the_call_without_them():
    c, _ = tolerance.solved("five", True)
    p, rows = bc.planted(c)
    a = call(p, threshold=bc.THRESHOLD)
    clean, keep = bc.without(p, rows)
    b = call(clean, threshold=bc.THRESHOLD)
    assert (a["status"][rows] != 0).all() and np.isnan(a["points"][rows]).all() and (b["status"] == 0).sum() > 1900
    assert same_bits(dict(a, points=a["points"][keep], status=a["status"][keep]), b)
    assert a["retval"] < 2 * bc.NOISE_SIGMA


def test_a_pair_alone_gets_the_start_and_status_it_gets_among_the_others():
    c, _ = tolerance.solved("five", True)
    g = got("five")
    for p in (0, 4, 9):
        rows = bc.single_pair(c, p)
        a, b = (int(v) for v in c["pairs"][p])
        # a problem of its own around the pair: three views, the pair and two small pairs that keep the third view in
        third = next(v for v in range(5) if v not in (a, b))
        views = sorted((a, b, third))
        at = {v: i for i, v in enumerate(views)}
        others = [q for q, (x, y) in enumerate(c["pairs"]) if x in views and y in views and q != p]
        order = sorted([p] + others, key=lambda q: (at[int(c["pairs"][q][0])], at[int(c["pairs"][q][1])]))
        sl = {q: bc.single_pair(c, q) for q in order}
        sub = dict(K=c["K"][views], T0=c["T0"][views], pairs=np.array([(at[int(c["pairs"][q][0])], at[int(c["pairs"][q][1])]) for q in order], np.int32),
                   uvs_a=np.concatenate([c["uvs_a"][sl[q]] for q in order]), uvs_b=np.concatenate([c["uvs_b"][sl[q]] for q in order]),
                   counts=np.array([c["counts"][q] for q in order]))
        r = call(sub, return_start=True)
        first = int(sum(c["counts"][q] for q in order[:order.index(p)]))
        mine = slice(first, first + int(c["counts"][p]))
        assert np.array_equal(r["status"][mine], g["status"][rows])
        assert np.array_equal(r["start"][mine], g["start"][rows], equal_nan=True)


def test_float32_matches():
    rec = tolerance.load()
    c = bc.case("three", bc.NOISE_SIGMA, bc.NOISY_SEED, dtype=np.float32)
    want = tolerance.solve(c)  # (the restatement on the same float32 pixels)
    g = call(c, return_start=True)
    assert np.array_equal(g["status"], want["status"]) and np.array_equal(g["start"], want["start"], equal_nan=True)
    d = tolerance.difference(g, want)
    assert all(d[k] <= rec["bound"][k] for k in tolerance.KEYS), d
    assert g["points"].dtype == np.float64 and g["pair_error"].dtype == np.float64


def test_tensors_in_tensors_out():
    import torch
    c, _ = tolerance.solved("three", True)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = ca.bundle_adjust_pairs(c["K"], c["T0"], c["pairs"], torch.from_numpy(c["uvs_a"]).to(dev), torch.from_numpy(c["uvs_b"]).to(dev), c["counts"])
    g = got("three")
    for k in ("points", "status", "pair_error"):
        assert isinstance(t[k], torch.Tensor) and t[k].device == dev
    assert isinstance(t["T"], np.ndarray) and isinstance(t["retval"], float)
    assert same_bits(dict(t, points=t["points"].cpu().numpy(), status=t["status"].cpu().numpy(), pair_error=t["pair_error"].cpu().numpy()), g)
    with pytest.raises(ValueError):
        ca.bundle_adjust_pairs(c["K"], c["T0"], c["pairs"], torch.from_numpy(c["uvs_a"]).to(dev), c["uvs_b"], c["counts"])


def test_sixteen_views_solve_and_seventeen_are_refused():
    c, want = tolerance.solved("sixteen", True)
    g = got("sixteen")
    assert g["T"].shape == (16, 4, 4) and len(g["pair_error"]) == 120
    start, result = ref.pose_errors(c["T0"], c["T_true"]), ref.pose_errors(g["T"], c["T_true"])
    assert result[0] < start[0] and result[1] < start[1]
    with pytest.raises(ValueError, match="3 .. 16 views, got 17"):
        ca.bundle_adjust_pairs(np.concatenate([c["K"], c["K"][:1]]), np.concatenate([c["T0"], c["T0"][:1]]), c["pairs"], c["uvs_a"], c["uvs_b"],
                               c["counts"])


def test_singular_problems_raise():
    c, _ = tolerance.solved("three", True)
    # every view at one centre: no match has a start point, and the views are left without observations
    T = c["T0"].copy()
    T[:, :3, 3] = T[0, :3, 3]
    with pytest.raises(ValueError, match="used observations"):
        ca.bundle_adjust_pairs(c["K"], T, c["pairs"], c["uvs_a"], c["uvs_b"], c["counts"])
    # view 2 is seen only through eight copies of one match: two equations for its six unknowns
    rows01, rows12 = bc.single_pair(c, 0), bc.single_pair(c, 2)
    ua = np.concatenate([c["uvs_a"][rows01], np.repeat(c["uvs_a"][rows12][:1], 8, 0)])
    ub = np.concatenate([c["uvs_b"][rows01], np.repeat(c["uvs_b"][rows12][:1], 8, 0)])
    with pytest.raises(ValueError, match=r"status 3 .* after \d+ evaluations, smallest pivot") as e:
        ca.bundle_adjust_pairs(c["K"], c["T0"], np.array([[0, 1], [1, 2]], np.int32), ua, ub, np.array([300, 8]))
    print(e.value)


def test_a_view_with_too_few_observations_is_named():
    c, _ = tolerance.solved("three", True)
    rows01, rows12 = bc.single_pair(c, 0), bc.single_pair(c, 2)
    ua = np.concatenate([c["uvs_a"][rows01], c["uvs_a"][rows12][:5]])
    ub = np.concatenate([c["uvs_b"][rows01], c["uvs_b"][rows12][:5]])
    with pytest.raises(ValueError, match="view 2 is left with 5 used observations"):
        ca.bundle_adjust_pairs(c["K"], c["T0"], np.array([[0, 1], [1, 2]], np.int32), ua, ub, np.array([300, 5]))


def aligned_errors(viewds, Ts):
    """pose errors against the scene's truth after the class's own alignment: view 0 on view 0, one scale"""
    keys = sorted(viewds)
    return ref.pose_errors(np.array([viewds[k]["T_re"] for k in keys]), np.array([Ts[k] for k in keys]))


@pytest.mark.parametrize("name", ("one_triple", "ten_triples"))
def test_refine_moves_the_propagated_poses_towards_the_truth(name):
    fx = rc.load_fixture()
    assert fx is not None
    viewds, flowds, Ts = rc.case(name, int(fx[name + "/seed"]))
    re_ = ca.ReconstructionExtrinsics(rc.fresh(viewds), flowds=flowds)
    for k, d in re_.viewds.items():  # the constructor's own outputs are what the reference gave, as the existing test asks
        want, sens = fx["%s/view%d/T_re" % (name, k)], ec.SENS_FACTOR * float(fx[name + "/sens_T_re"])
        assert d["uvzis"].shape == (int(fx["%s/view%d/rows" % (name, k)]), 4)
        assert np.abs(d["T_re"][:3, 3] - want[:3, 3]).max() <= sens and np.abs(d["T_re"][:3, :3] - want[:3, :3]).max() <= max(sens, ec.R_ULP)
    before_T = {k: v["T_re"].copy() for k, v in re_.viewds.items()}
    before_rows = {k: np.array(v["uvzis"]) for k, v in re_.viewds.items()}
    before = aligned_errors(re_.viewds, Ts)
    before_distance = ref.pose_distance(np.array([re_.viewds[k]["T_re"] for k in sorted(re_.viewds)]), np.array([Ts[k] for k in sorted(re_.viewds)]))
    again = ca.ReconstructionExtrinsics(rc.fresh(viewds), flowds=flowds)  # no refine: nothing differs from the first
    assert all(np.array_equal(again.viewds[k]["T_re"], before_T[k]) and np.array_equal(again.viewds[k]["uvzis"], before_rows[k]) for k in before_T)
    out = re_.refine()
    after = aligned_errors(re_.viewds, Ts)
    print("%s: rotation %.3g -> %.3g rad, centre %.3g -> %.3g; retval %.3g px after %d evaluations"
          % (name, before[0], after[0], before[1], after[1], re_.refinement["retval"], re_.refinement["evaluations"]))
    # "closer" is the distance of the whole pose, |T - T_true|_F.  The rotations alone cannot come closer on these noise-free
    # scenes: view 0 is the frame of reference and keeps the constructor's rotation, whose entries are float32-rounded, so
    # both sides of the comparison sit at that floor (4e-8 .. 6e-8 rad); the centres are what the propagation leaves off.
    keys = sorted(re_.viewds)
    closer = ref.pose_distance(np.array([re_.viewds[k]["T_re"] for k in keys]), np.array([Ts[k] for k in keys]))
    assert out is re_.viewds and closer < before_distance and after[1] < before[1] and after[0] < max(before[0], 4 * ec.R_ULP)
    rows = np.concatenate([v["uvzis"] for v in re_.viewds.values()])
    assert rows.dtype == np.float64 and rows.shape[1] == 4 and abs(rows[:, 2].mean() - 1) < 1e-12
    T0 = re_.viewds[0]["T_re"]
    assert np.abs(T0[:3, :3] - np.eye(3)).max() < 1e-12 and np.abs(T0[:2, 3]).max() < 1e-12
    assert abs(T0[2, 3] + re_.viewds[0]["uvzis"][:, 2].mean()) < 1e-12
    used = int((re_.refinement["status"] == 0).sum())
    assert len(rows) == 2 * used and set(np.unique(rows[:, 3])) == set(float(k) for k in re_.viewds)
