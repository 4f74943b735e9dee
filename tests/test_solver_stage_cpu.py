"""The stage fixture of the two joint solvers without a GPU: tests/golden/solver_stage_tolerance.json is the restatements'
measured error against tests/golden/solver_stage_exact.npz, times 8 and below the cap; the fixture's small cases come out
of tests/solver_stage_exact.py again bit for bit (where mpmath is installed); every case meets the conditions the
comparison relies on; and the comparison the GPU test uses rejects nine structural mistakes, planted in the restatement's
output, by at least 1000 times its bound."""
import numpy as np
import pytest

import calibrate_ref
import solver_stage_cases as cases
import solver_stage_tolerance as tolerance
import stereo_calibrate_ref

SENSITIVITY = 1000


def test_tolerance_file_is_the_measurement():
    """the bounds are 8 x the restatement's own error against the exact fixture (8 roundings where that is less than one),
    every one below the cap; a fresh measurement lies within them"""
    rec, now = tolerance.load(), tolerance.measure()
    expect = sorted(tolerance.kinds("calib") + tolerance.kinds("stereo"))
    assert sorted(rec["bound"]) == sorted(rec["measured"]) == sorted(now["measured"]) == expect
    assert rec["factor"] == tolerance.FACTOR == 8 and rec["cap"] == tolerance.CAP == 1e-10 and rec["ulp"] == 2.0 ** -52
    for k in expect:
        assert rec["bound"][k] == 8 * max(rec["measured"][k], rec["ulp"]) and rec["bound"][k] < rec["cap"], k
        assert now["measured"][k] <= rec["bound"][k], (k, now["measured"][k], rec["bound"][k])
    assert sorted(rec["cases"]) == sorted(cases.NAMES)
    for name, (c, want) in tolerance.fixture().items():
        assert rec["cases"][name] == tolerance.conditions(want), name


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_meets_its_conditions(name):
    """from the exact numbers alone: the candidate's cost at least 0.1 % below the current one (above it, for the rejected
    case), so that no decision hinges on the 64-ulp rule; every frame's damped block and the reduced matrix positive
    definite; the smallest unit-diagonal pivot four orders above SINGULAR_PIVOT"""
    c, want = tolerance.fixture()[name]
    got = tolerance.conditions(want)
    assert got["definite"] and got["pivot"] >= 1e-6 >= 1e4 * calibrate_ref.SINGULAR_PIVOT
    if name == cases.REJECTED:
        assert got["cost_change"] >= 1e-3 and not bool(want["accept"]) and float(c["lam"]) == 1e-9
    else:
        assert got["cost_change"] <= -1e-3 and bool(want["accept"]) and float(c["lam"]) == 1e-3
    has_rows = "ws" in want
    assert has_rows == (name != cases.MANY)
    if has_rows:
        frames = len(c["counts"])
        width = 136 if c["kind"] == "calib" else 91
        assert want["ws"].shape == want["scale"].shape == (frames, width) and want["cand"].shape == (frames, 16)
        assert (np.abs(want["ws"]) <= want["scale"].astype(np.float64) * (1 + 2.0 ** -23)).all()
    if c["kind"] == "calib":
        fixed = c["mask"] == 0
        assert (want["step"][fixed] == 0).all() and np.array_equal(want["shared"][fixed], c["k"][fixed])


def test_the_cases_cover_the_edges():
    f = tolerance.fixture()
    for kind in ("calib", "stereo"):
        mine = [c for c, _ in f.values() if c["kind"] == kind]
        assert {int(n) for c in mine for n in c["counts"]} >= {4, 63, 64, 65, 130}
        assert {len(c["counts"]) for c in mine} >= {1, 3, 4, 5, 65}
        assert any(c["obj"].dtype == np.float32 and c[("uv" if kind == "calib" else "uv1")].dtype == np.float32 for c in mine)
        assert any(bool(c["shared"]) for c in mine) and any(sorted(set(c["counts"].tolist())) == [4, 130] for c in mine)
    assert {(len(c["D1"]), len(c["D2"])) for c, _ in f.values() if c["kind"] == "stereo"} >= {(5, 5), (0, 12), (4, 8)}
    masks = {tuple(c["mask"]) for c, _ in f.values() if c["kind"] == "calib"}
    assert masks == {tuple(cases.FREE), tuple(cases.FIX_K3), tuple(cases.FIX_PRINCIPAL_POINT)}
    assert len(f[cases.MANY][0]["counts"]) == 4097


@pytest.mark.parametrize("name", cases.SMALL)
def test_the_fixture_regenerates_bit_for_bit(name):
    pytest.importorskip("mpmath")
    import solver_stage_exact
    c, want = tolerance.fixture()[name]
    again = solver_stage_exact.evaluate(c)
    assert sorted(again) == sorted(want)
    for k in want:
        assert again[k].dtype == want[k].dtype and np.array_equal(again[k], want[k]), k


# ---- sensitivity: the comparison against nine planted mistakes ------------------------------------------------------
def rejection(name, lin=None, step=None, after=None):
    """how many times its bound the worst error of a mutated restatement is: ``lin`` replaces the sums, ``step`` the
    shared step and the frames' factors, ``after`` changes the finished output"""
    c, want = tolerance.fixture()[name]
    good, rest = tolerance.linearised(c)
    lin = good if lin is None else lin(c, good, rest)
    bound = tolerance.load()["bound"]
    solve = (lambda: calibrate_ref.shared_step(lin, float(c["lam"]), c["mask"] != 0)) if c["kind"] == "calib" else \
        (lambda: stereo_calibrate_ref.shared_step(lin, float(c["lam"])))
    if step is None and solve() is None:  # mutated sums without a definite system: the sums alone are compared
        e = tolerance.block_errors(c["kind"], tolerance.pack(lin), want["ws"], want["scale"])
    else:
        got = tolerance.stages(c, lin, rest, step=None if step is None else step(c, lin))
        if after is not None:
            after(got)
        e = tolerance.errors(c["kind"], got, want)
    assert all(v <= bound[k] for k, v in tolerance.errors(c["kind"], tolerance.stages(c, good, rest), want).items())
    return max(v / bound[k] for k, v in e.items())


def stereo_terms(c, rest, change):
    poses, R, t, objs, uv1s, uv2s, cams = rest
    out = []
    for (Ri, ti), obj, u1, u2 in zip(poses, objs, uv1s, uv2s):
        r1, J1, r2, Jf, Jr = stereo_calibrate_ref.frame_terms(Ri, ti, R, t, obj, u1, u2, cams)
        out.append(stereo_calibrate_ref.blocks(*change(r1, J1, r2, Jf.copy(), Jr.copy(), R, R @ ti)))
    return out


def without_cross_term(c, good, rest):
    def change(r1, J1, r2, Jf, Jr, R, rt):
        Jr[:, :3] -= np.cross(rt, Jr[:, 3:])
        return r1, J1, r2, Jf, Jr
    return stereo_terms(c, rest, change)


def frame_jacobian_not_turned(c, good, rest):
    def change(r1, J1, r2, Jf, Jr, R, rt):
        return r1, J1, r2, np.concatenate([Jf[:, :3] @ R.T, Jf[:, 3:] @ R.T], 1), Jr
    return stereo_terms(c, rest, change)


def b_transposed(c, good, rest):
    return [(A, B.T.copy(), C, gp, gs, cost) for A, B, C, gp, gs, cost in good]


def k3_column_with_r4(c, good, rest):
    poses, objs, uvs = rest
    out = []
    for (R, t), obj, uv in zip(poses, objs, uvs):
        r, Jp, Jk = calibrate_ref.frame_terms(R, t, obj, uv, c["k"])
        Jk[:, 8] = Jk[:, 5]
        out.append(calibrate_ref.blocks(r, Jp, Jk))
    return out


def last_point(of, how):
    """frame 0 of a 65-point case summed without its last point (how = 0) or with it twice (how = 2)"""
    def lin(c, good, rest):
        assert c["counts"][0] == 65
        rows = slice(0, 64) if how == 0 else list(range(65)) + [64]
        if c["kind"] == "calib":
            poses, objs, uvs = rest
            first = calibrate_ref.linearise(poses[:1], [objs[0][rows]], [uvs[0][rows]], c["k"])
        else:
            poses, R, t, objs, uv1s, uv2s, cams = rest
            first = stereo_calibrate_ref.linearise(poses[:1], R, t, [objs[0][rows]], [uv1s[0][rows]], [uv2s[0][rows]], cams)
        return first + good[1:]
    return lin


def shared_system(c, lin, frames, damping):
    """(shared step, all frames' factors) from the reduced system over ``frames`` with lambda x ``damping(S, dC)`` added"""
    lam = float(c["lam"])
    if c["kind"] == "calib":
        free = c["mask"] != 0
        S, g, dC, _ = calibrate_ref.reduced(lin[frames], lam, free)
        S, g = calibrate_ref.mask_system(S + lam * np.diag(damping(S, dC)), g, free)
        return np.linalg.solve(S, -g), calibrate_ref.reduced(lin, lam, free)[3]
    S, g, dC, _ = stereo_calibrate_ref.reduced(lin[frames], lam)
    return np.linalg.solve(S + lam * np.diag(damping(S, dC)), -g), stereo_calibrate_ref.reduced(lin, lam)[3]


def without_frame_64(c, lin):
    assert len(lin) == 65
    return shared_system(c, lin, slice(0, 64), lambda S, dC: dC)


def damping_on_s(c, lin):
    return shared_system(c, lin, slice(None), lambda S, dC: np.diag(S))


def norm_of_the_candidate(got):
    got["cand"] = got["cand"].copy()
    got["cand"][:, 14] = 3.0 + (got["cand"][:, 9:12] ** 2).sum(1)


MUTATIONS = {
    "Jr without the (R t_i) x Jd term": ("stereo-f5-n65", dict(lin=without_cross_term)),
    "Jf not turned by R": ("stereo-f5-n65", dict(lin=frame_jacobian_not_turned)),
    "B transposed (stereo)": ("stereo-f5-n65", dict(lin=b_transposed)),
    "the k3 column built with r^4": ("calib-f3-n63", dict(lin=k3_column_with_r4)),
    "the 65th point left out (calibrate)": ("calib-f5-n65-fix-pp", dict(lin=last_point("calib", 0))),
    "the 65th point left out (stereo)": ("stereo-f5-n65", dict(lin=last_point("stereo", 0))),
    "the 65th point counted twice (calibrate)": ("calib-f5-n65-fix-pp", dict(lin=last_point("calib", 2))),
    "the 65th point counted twice (stereo)": ("stereo-f5-n65", dict(lin=last_point("stereo", 2))),
    "frame 64 of 65 left out of the reduced system (calibrate)": ("calib-f65-n4", dict(step=without_frame_64)),
    "frame 64 of 65 left out of the reduced system (stereo)": ("stereo-f65-n4", dict(step=without_frame_64)),
    "damping on S, not on diag sum C (calibrate)": ("calib-f3-n63", dict(step=damping_on_s)),
    "damping on S, not on diag sum C (stereo)": ("stereo-f5-n65", dict(step=damping_on_s)),
    "|pose|^2 of the candidate (calibrate)": ("calib-f3-n63", dict(after=norm_of_the_candidate)),
    "|pose|^2 of the candidate (stereo)": ("stereo-f5-n65", dict(after=norm_of_the_candidate)),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_the_comparison_rejects_a_planted_mistake(what):
    name, how = MUTATIONS[what]
    times = rejection(name, **how)
    print("%s: %.3g times the bound" % (what, times))
    assert times >= SENSITIVITY
