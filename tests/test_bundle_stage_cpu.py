"""The stage fixture of the bundle adjustment without a GPU: tests/golden/bundle_stage_tolerance.json is the restatement's
measured error against tests/golden/bundle_stage_exact.npz, times 8 and below the cap; the fixture's inputs are
tests/bundle_stage_cases.py regenerated, and its smallest cases come out of tests/bundle_stage_exact.py again bit for bit
(where mpmath is installed); every case meets the conditions the comparison relies on; and the comparison the GPU test
uses rejects nine structural mistakes, planted in the restatement, by at least 1000 times a bound.  (The restatement's
Jacobians against differences: tests/test_bundle_cpu.py.)"""
import numpy as np
import pytest

from calibrating_amd import _native

import bundle_ref as ref
import bundle_stage_cases as cases
import bundle_stage_tolerance as tolerance

SENSITIVITY = 1000


def test_tolerance_file_is_the_measurement():
    """the bounds are 8 x the restatement's own error against the exact fixture (8 roundings where that is less than one),
    every one below the cap; a fresh measurement lies within them"""
    rec, now = tolerance.load(), tolerance.measure()
    assert sorted(rec["bound"]) == sorted(rec["measured"]) == sorted(now["measured"]) == sorted(tolerance.KINDS)
    assert rec["factor"] == tolerance.FACTOR == 8 and rec["cap"] == tolerance.CAP == 1e-10 and rec["ulp"] == 2.0 ** -52
    for k in tolerance.KINDS:
        assert rec["bound"][k] == 8 * max(rec["measured"][k], rec["ulp"]) and rec["bound"][k] < rec["cap"], k
        assert now["measured"][k] <= rec["bound"][k], (k, now["measured"][k], rec["bound"][k])
    assert sorted(rec["cases"]) == sorted(cases.NAMES)
    for name, (c, want) in tolerance.fixture().items():
        assert rec["cases"][name] == tolerance.conditions(c, want), name


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_meets_its_conditions(name):
    """from the exact numbers alone: every point's block and the reduced matrix positive definite, six observations and
    more per view, no candidate behind a view, the candidate's cost at least 0.1 % off the current one (far above the 64 ulp
    of lm_better and above every bound), so that no rounding flips the decision; and every used match has a triangulation
    sine of MIN_SINE and more by the restatement's start()"""
    c, want = tolerance.fixture()[name]
    got = tolerance.conditions(c, want)
    assert got["definite"] and got["observations"] >= ref.MIN_OBSERVATIONS and got["behind"] == 0
    assert got["pivot"] >= 1e-6 >= 1e4 * ref.SINGULAR_PIVOT
    assert abs(got["cost_change"]) >= 1e-3 > 1e6 * ref.COST_RESOLUTION
    assert got["accept"] == (got["cost_change"] < 0) == (name != cases.REJECTED)
    assert float(c["lam"]) == (1e-9 if name == cases.REJECTED else 1e-3)
    R, t = ref.poses_from_T(c["T0"])
    _, status = ref.start(c["K"], R, t, [tuple(p) for p in c["pairs"]], c["uvs_a"], c["uvs_b"], [int(n) for n in c["counts"]])
    assert np.array_equal(status, c["status"]) and np.array_equal(np.flatnonzero(status == 0), c["src"])
    assert c["X"].shape == (len(c["src"]), 3) and not np.array_equal(c["src"], np.arange(len(c["src"])))
    P, N = len(c["pairs"]), len(c["K"])
    assert want["pair_blocks"].shape == want["pair_scale"].shape == (P, 103) and want["eval_blocks"].shape == (P, 3)
    assert want["step"].shape == (N, 6) and want["cand"].shape == (N, 12)
    assert (np.abs(want["pair_blocks"]) <= want["pair_scale"].astype(np.float64) * (1 + 2.0 ** -22)).all()
    fixed = int(c["fixed_view"])
    anchor, axis = ref.gauge(c["T0"], fixed)
    assert (want["step"][fixed] == 0).all() and np.array_equal(want["cand"][fixed], np.concatenate([R[fixed].reshape(9), t[fixed]]))
    Ra, ta = want["cand"][anchor, :9].reshape(3, 3), want["cand"][anchor, 9:]
    assert abs((Ra.T @ ta)[axis] - (R[anchor].T @ t[anchor])[axis]) < 1e-14  # (the exact candidate keeps the held coordinate)
    if name == cases.MANY:
        assert "partials" not in want and "depth_a" not in want and want["dX"].shape == (32, 3)
        assert c["uvs_a"].dtype == np.float32 and np.array_equal(c["X"], c["X"].astype(np.float32))
        assert {0, 255, 256, 16383, 16384} <= set(want["dX_rows"].tolist())
    else:
        chunks = len(tolerance.chunk_rows(c)[0])
        assert want["partials"].shape == want["partials_scale"].shape == (chunks, 103) and want["eval_partials"].shape == (chunks, 3)
        assert want["dX"].shape == c["X"].shape and want["depth_a"].shape == want["depth_b"].shape == (len(c["X"]),)
        assert (want["depth_a"] > 0).all() and (want["depth_b"] > 0).all()


def test_the_cases_cover_the_edges():
    f = tolerance.fixture()
    used = {name: cases.used_counts(c) for name, (c, _) in f.items()}
    assert used["v3-n7-64-65"] == [7, 64, 65] and used["v5-borders"] == used["v5-borders-f32-fixed3"] == [6, 63, 255, 256, 257] + [20] * 5
    assert used["v12-p66"] == [6] * 66 and used["v16-p120"] == [6] * 120 and used[cases.MANY] == [64 * 256 + 1, 8, 8]
    assert 66 > 64 and 6 * 16 == 96 and len(tolerance.chunk_rows(f[cases.MANY][0])[0]) == 65 + 2
    c = f["v5-borders-f32-fixed3"][0]
    assert c["uvs_a"].dtype == c["uvs_b"].dtype == np.float32 and int(c["fixed_view"]) == 3 and ref.gauge(c["T0"], 3)[0] == 0
    assert [ref.gauge(f[n][0]["T0"], int(f[n][0]["fixed_view"]))[1] for n in cases.AXES] == [0, 1, 2]
    for name, (c, _) in f.items():  # rows that are not used at the start, in the middle and at the end of a pair
        bounds = np.concatenate([[0], np.cumsum(c["counts"])])
        st = c["status"]
        assert set(st.tolist()) == {0, 1, 2}, name
        assert any(st[bounds[p]] != 0 and st[bounds[p + 1] - 1] != 0 and (st[bounds[p] + 1:bounds[p + 1] - 1] != 0).any()
                   for p in range(len(c["counts"]))), name
    assert _native.BUNDLE_CHUNK == 256 and _native.BUNDLE_PARTIAL_DOUBLES == 104 and tolerance.BLOCKS["cost"].stop == 103


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_fixture_holds_the_cases_regenerated(name):
    c, _ = tolerance.fixture()[name]
    again = cases.case(name)
    for k in cases.INPUT_KEYS:
        a = again[k].astype(np.float32).astype(np.float64) if name == cases.MANY and k == "X" else again[k]
        assert a.dtype == c[k].dtype and np.array_equal(a, c[k], equal_nan=True), k


@pytest.mark.parametrize("name", cases.AXES)
def test_the_fixture_regenerates_bit_for_bit(name):
    pytest.importorskip("mpmath")
    import bundle_stage_exact
    assert bundle_stage_exact.CHUNK == _native.BUNDLE_CHUNK and bundle_stage_exact.BLOCKS == tolerance.BLOCKS
    c, want = tolerance.fixture()[name]
    again = bundle_stage_exact.evaluate(c)
    assert sorted(again) == sorted(want)
    for k in want:
        assert again[k].dtype == want[k].dtype and np.array_equal(again[k], want[k]), k


# ---- sensitivity: the comparison against nine planted mistakes ------------------------------------------------------
def s_ba_transposed(terms, blocks, chunk_blocks):
    return [dict(b, ba=b["ba"].T.copy()) for b in blocks]


def zty_dropped(terms, blocks, chunk_blocks):
    out = []
    for o, b in zip(terms, blocks):
        ga = (o["Ja"][:, 0] * o["ra"][:, :1] + o["Ja"][:, 1] * o["ra"][:, 1:]).sum(0)
        gb = (o["Jb"][:, 0] * o["rb"][:, :1] + o["Jb"][:, 1] * o["rb"][:, 1:]).sum(0)
        out.append(dict(b, ga=ga, gb=gb))
    return out


def last_chunk_left_out(terms, blocks, chunk_blocks):
    assert max(len(ch) for ch in chunk_blocks) == 2
    return [b if len(ch) == 1 else ch[0] for b, ch in zip(blocks, chunk_blocks)]


def held_row_one_further(prob):
    prob.keep = [e for e in range(6 * prob.N) if e // 6 != prob.fixed and e != 6 * prob.anchor + 3 + (prob.axis + 1) % 3]


def undamped_factor(terms, undamped):
    return [dict(o, L=o0["L"], il=o0["il"]) for o, o0 in zip(terms, undamped)]


def anchor_moved_like_any_view(out, prob, R, t, x):
    a = prob.anchor
    out["cand"] = out["cand"].copy()
    out["cand"][a, 9:] = t[a] + x[6 * a + 3:6 * a + 6]


def anchor_matrix_without_the_cross_block(R, t):
    M = np.zeros((6, 6))
    M[:3, :3] = np.eye(3)
    M[3:, 3:] = -R
    return M


MUTATIONS = {
    "S_ba transposed": dict(blocks=s_ba_transposed),
    "lambda diag U left off the views": dict(view_lam=0.0),
    "lambda left off the points' V": dict(point_lam=0.0),
    "the -[t]x block of the anchor's M zeroed": dict(anchor_matrix=anchor_matrix_without_the_cross_block),
    "the anchor's held row taken at 3 + (axis + 1) % 3": dict(problem=held_row_one_further),
    "Z^T y dropped from g": dict(blocks=zty_dropped),
    "the point step solved with the undamped L": dict(candidate_terms=undamped_factor),
    "the last chunk of a pair left out": dict(blocks=last_chunk_left_out),
    "the anchor's candidate t' = t + d": dict(after=anchor_moved_like_any_view),
}
MUTATED_CASE = "v5-borders"


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_the_comparison_rejects_a_planted_mistake(what, monkeypatch):
    c, want = tolerance.fixture()[MUTATED_CASE]
    bound = tolerance.load()["bound"]
    assert all(v <= bound[k] for k, v in tolerance.errors(tolerance.stages(c), want).items())
    how = dict(MUTATIONS[what])
    if "anchor_matrix" in how:
        monkeypatch.setattr(ref, "anchor_matrix", how.pop("anchor_matrix"))
    got = tolerance.stages(c, mutate=how)
    e = tolerance.errors(got, want, tolerance.EVALUATION + tolerance.FINAL if "step" in got else ())
    times = {k: v / bound[k] for k, v in e.items()}
    worst = max(times, key=times.get)
    print("%s: %s is %.3g times its bound of %.3g" % (what, worst, times[worst], bound[worst]))
    assert times[worst] >= SENSITIVITY
