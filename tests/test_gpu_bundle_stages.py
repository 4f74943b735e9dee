"""The stages of the bundle adjustment on the MI355X (-m gpu), each driven alone through ``_native.call`` as ``bundle.py``
drives them, against the exact fixture tests/golden/bundle_stage_exact.npz within the bounds of
tests/golden/bundle_stage_tolerance.json (measured on the NumPy restatement, never on a kernel): ``camd_bundle_start / emit /
step / finish`` at one evaluation point off the minimum per case.  Every buffer has the size ``bundle.py`` gives it and
starts as zeros; the stages are called in the package's order only.  Nothing here needs mpmath."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from calibrating_amd import _native, bundle  # noqa: E402
from calibrating_amd._arrays import FLOAT_TYPES, dtype_name, to_device  # noqa: E402

import bundle_stage_cases as cases  # noqa: E402
import bundle_stage_tolerance as tolerance  # noqa: E402

N = _native
WHAT = "bundle stage test"
LABEL0 = 40.0  # the views' labels are 40, 41, ...: no index, no status, no count


class Solver:
    """One case on the device, built as ``bundle_adjust_pairs`` builds it: the same sizes, segments, chunks, gauge and
    poses, zero-filled buffers.  After ``camd_bundle_start`` and ``camd_bundle_emit`` the status and the source rows are
    the fixture's, and the case's evaluation point is written over the start points."""

    def __init__(self, c, converged=0.0, rows=False, lam=None):
        self.c = c
        K, T = np.asarray(c["K"], np.float64), np.asarray(c["T0"], np.float64)
        pairs, counts = np.ascontiguousarray(c["pairs"], np.int32), np.asarray(c["counts"], np.int64)
        self.views, self.pairs, M = len(K), len(pairs), len(c["uvs_a"])
        self.fixed = int(c["fixed_view"])
        self.anchor, self.axis = bundle.gauge(T, self.fixed)
        R0, t0 = bundle.poses_from_T(T)
        self.start_poses = np.concatenate([R0.reshape(self.views, 9), t0], 1)
        name = dtype_name(c["uvs_a"])
        self.ua = to_device(np.array(c["uvs_a"]), dtype=name)  # (copies: the fixture is read-only)
        self.dev = dev = self.ua.device
        self.ub = to_device(np.array(c["uvs_b"]), dtype=name, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        host = np.zeros(N.BUNDLE_STATE_DOUBLES)
        host[N.BUNDLE_LAMBDA] = float(c["lam"]) if lam is None else lam
        host[N.BUNDLE_CONVERGED] = converged
        host[N.BUNDLE_FIXED], host[N.BUNDLE_ANCHOR], host[N.BUNDLE_AXIS] = self.fixed, self.anchor, self.axis
        host[N.BUNDLE_LABEL:N.BUNDLE_LABEL + self.views] = LABEL0 + np.arange(self.views)
        host[N.BUNDLE_POSES:N.BUNDLE_POSES + 12 * self.views] = self.start_poses.reshape(-1)
        host[N.BUNDLE_K:N.BUNDLE_K + 4 * self.views] = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1).reshape(-1)
        self.state = torch.from_numpy(host).to(dev)
        seg_first, seg_n = bundle._segments(counts)
        pair_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        put = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
        self.d_pairs, self.d_start, self.d_seg_first, self.d_seg_n = put(pairs.reshape(-1)), put(pair_start), put(seg_first), put(seg_n)
        self.status = torch.zeros(M, dtype=torch.int32, device=dev)
        self.points = torch.zeros((M, 3), **f64)
        self.rowoff = torch.zeros(len(seg_n) + 1, dtype=torch.int64, device=dev)
        self.rowcount = torch.zeros(len(seg_n), dtype=torch.int32, device=dev)
        self.b = b = N.Bundle()
        b.uv_a, b.uv_b, b.pair_views, b.pair_start = self.ua.data_ptr(), self.ub.data_ptr(), self.d_pairs.data_ptr(), self.d_start.data_ptr()
        b.seg_first, b.seg_n, b.status, b.points = self.d_seg_first.data_ptr(), self.d_seg_n.data_ptr(), self.status.data_ptr(), self.points.data_ptr()
        b.rowoff, b.rowcount, b.state = self.rowoff.data_ptr(), self.rowcount.data_ptr(), self.state.data_ptr()
        b.threshold = -1.0
        b.matches, b.uv_type, b.views, b.pairs, b.segments = M, FLOAT_TYPES[name], self.views, self.pairs, len(seg_n)
        N.call("camd_bundle_start", dev, ctypes.byref(b), int(counts.max()), what=WHAT)
        off = self.rowoff.cpu().numpy()
        seg_of_pair = np.concatenate([[0], np.cumsum((counts + N.BUNDLE_SEGMENT - 1) // N.BUNDLE_SEGMENT)])
        self.used_counts = np.diff(off[seg_of_pair]).astype(np.int64)
        assert self.used_counts.tolist() == cases.used_counts(c)
        self.U = U = int(off[-1])
        self.table, self.ranges = bundle._chunks(self.used_counts)
        self.d_table, self.d_ranges = put(self.table.reshape(-1)), put(self.ranges)
        chunks = len(self.table)
        self.cua, self.cub = torch.zeros((U, 2), dtype=self.ua.dtype, device=dev), torch.zeros((U, 2), dtype=self.ua.dtype, device=dev)
        self.X, self.Xc = torch.zeros((U, 3), **f64), torch.zeros((U, 3), **f64)
        self.src = torch.zeros(U, dtype=torch.int64, device=dev)
        self.partials, self.pair_blocks = torch.zeros((chunks, N.BUNDLE_PARTIAL_DOUBLES), **f64), torch.zeros((self.pairs, N.BUNDLE_PARTIAL_DOUBLES), **f64)
        self.eval_partials, self.eval_blocks = torch.zeros((chunks, N.BUNDLE_EVAL_DOUBLES), **f64), torch.zeros((self.pairs, N.BUNDLE_EVAL_DOUBLES), **f64)
        self.pair_error = torch.zeros(self.pairs, **f64)
        if rows:
            self.rows_a, self.rows_b = torch.zeros((U, 4), **f64), torch.zeros((U, 4), **f64)
            b.rows_a, b.rows_b = self.rows_a.data_ptr(), self.rows_b.data_ptr()
        b.chunk_table, b.pair_chunk, b.uv_used_a, b.uv_used_b = self.d_table.data_ptr(), self.d_ranges.data_ptr(), self.cua.data_ptr(), self.cub.data_ptr()
        b.X, b.candidate, b.src, b.partials, b.pair_blocks = (self.X.data_ptr(), self.Xc.data_ptr(), self.src.data_ptr(), self.partials.data_ptr(),
                                                              self.pair_blocks.data_ptr())
        b.eval_partials, b.eval_blocks, b.pair_error = self.eval_partials.data_ptr(), self.eval_blocks.data_ptr(), self.pair_error.data_ptr()
        b.used, b.chunks = U, chunks
        N.call("camd_bundle_emit", dev, ctypes.byref(b), what=WHAT)
        assert np.array_equal(self.host("status"), c["status"]) and np.array_equal(self.host("src"), c["src"])
        used = c["status"] == 0
        assert np.array_equal(self.host("cua"), c["uvs_a"][used]) and np.array_equal(self.host("cub"), c["uvs_b"][used])
        self.X.copy_(torch.from_numpy(np.array(c["X"], np.float64)).to(dev))  # the evaluation point, to the bit

    def step(self):
        N.call("camd_bundle_step", self.dev, ctypes.byref(self.b), what=WHAT)
        return self

    def finish(self):
        N.call("camd_bundle_finish", self.dev, ctypes.byref(self.b), what=WHAT)
        return self

    def host(self, what):
        return getattr(self, what).cpu().numpy()

    def read(self):
        """(solved, accept, evaluations, iterations, done), lambda, and the state"""
        s = self.host("state")
        flags = tuple(int(s[k]) for k in (N.BUNDLE_SOLVED, N.BUNDLE_ACCEPT, N.BUNDLE_EVALUATIONS, N.BUNDLE_ITERATIONS, N.BUNDLE_DONE))
        return flags, s[N.BUNDLE_LAMBDA], s

    def poses(self, s, where):
        return s[where:where + 12 * self.views].reshape(self.views, 12)

    def evaluation(self):
        """what one step left behind, in the layout of the exact fixture"""
        s = self.host("state")
        return dict(partials=self.host("partials"), pair_blocks=self.host("pair_blocks"),
                    step=s[N.BUNDLE_STEP:N.BUNDLE_STEP + 6 * self.views].reshape(self.views, 6), cand=self.poses(s, N.BUNDLE_CANDIDATE),
                    dX=self.host("Xc") - self.host("X"), eval_partials=self.host("eval_partials"), eval_blocks=self.host("eval_blocks"),
                    cand_cost=self.host("eval_blocks")[:, 0].sum(), cost=s[N.BUNDLE_COST])


def want_of(name):
    return tolerance.fixture()[name]


@pytest.fixture(scope="module")
def bound():
    return tolerance.load()["bound"]


def check(name, e, bound, keys=None):
    keys = sorted(e) if keys is None else keys
    print("%s: %s" % (name, ", ".join("%s %.3g (bound %.3g)" % (k, e[k], bound[k]) for k in keys)))
    assert all(e[k] <= bound[k] for k in keys), {k: (e[k], bound[k]) for k in keys if not e[k] <= bound[k]}


def relative(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b) / np.abs(b)))


@pytest.mark.parametrize("name", cases.SMALL)
def test_step_gives_the_exact_sums(name, bound):
    """every entry of every chunk's partial and of every pair's block within its bound of the exact sum, on the scale of its
    absolute products; no point's block failed to factor; a second fresh run gives the same bits"""
    c, want = want_of(name)
    a, b = Solver(c).step(), Solver(c).step()
    partials, blocks = a.host("partials"), a.host("pair_blocks")
    check(name + " chunks", tolerance.block_errors(partials, want["partials"], want["partials_scale"]), bound)
    check(name + " pairs", tolerance.block_errors(blocks, want["pair_blocks"], want["pair_scale"]), bound)
    assert (partials[:, 103] == 0).all() and (blocks[:, 103] == 0).all()
    assert np.array_equal(partials, b.host("partials")) and np.array_equal(blocks, b.host("pair_blocks"))
    assert np.array_equal(a.host("eval_blocks"), b.host("eval_blocks")) and np.array_equal(a.host("state"), b.host("state"))


@pytest.mark.parametrize("name", [n for n in cases.SMALL if n != cases.REJECTED])
def test_step_takes_the_exact_candidate(name, bound):
    """after one step: the flags and counts, lambda's bits, the cost, every view's step and candidate, every point's step,
    the candidates' sums; then the hand-over into the next evaluation"""
    c, want = want_of(name)
    s = Solver(c).step()
    flags, lam, state = s.read()
    assert bool(want["accept"]) and flags == (1, 1, 1, 1, 0)
    assert lam == float(c["lam"]) * 0.1
    got = s.evaluation()
    e = tolerance.errors(got, want, tolerance.EVALUATION, sums=False)
    e["cost"] = max(relative(state[N.BUNDLE_COST], want["cost"]), relative(state[N.BUNDLE_COST0], want["cost"]))
    check(name, e, bound)
    assert (got["step"][s.fixed] == 0).all() and np.array_equal(got["cand"][s.fixed], s.start_poses[s.fixed])
    Ra, ta = got["cand"][s.anchor, :9].reshape(3, 3), got["cand"][s.anchor, 9:]
    R0, t0 = s.start_poses[s.anchor, :9].reshape(3, 3), s.start_poses[s.anchor, 9:]
    held = abs(float((Ra.T @ ta)[s.axis] - (R0.T @ t0)[s.axis]))
    print("%s: the anchor's centre moves by %.3g along its held axis %d (bound %.3g)" % (name, held, s.axis, bound["pose"]))
    assert held <= bound["pose"]
    assert (got["eval_partials"][:, 3] == 0).all() and (got["eval_blocks"][:, 3] == 0).all()
    assert np.array_equal(s.poses(state, N.BUNDLE_POSES), got["cand"])  # an accepted step: the views have moved
    assert np.array_equal(s.host("X"), c["X"])  # (the points follow in the next linearisation)
    Xc = s.host("Xc")
    flags2, _, state2 = s.step().read()
    assert np.array_equal(s.host("X"), Xc) and flags2[2] == 2
    again = relative(state2[N.BUNDLE_COST], got["cand_cost"])
    print("%s: the candidate's cost in the next evaluation differs by %.3g (bound %.3g)" % (name, again, bound["cost"]))
    assert again <= bound["cost"]


def test_a_rejected_step_moves_nothing():
    c, want = want_of(cases.REJECTED)
    assert not bool(want["accept"])
    s = Solver(c).step()
    flags, lam, state = s.read()
    assert flags == (1, 0, 1, 0, 0) and lam == float(c["lam"]) * 10.0
    assert np.array_equal(s.poses(state, N.BUNDLE_POSES), s.start_poses) and np.array_equal(s.host("X"), c["X"])
    # the next linearisation is the one of a fresh state at ten times lambda: neither the views nor the points have moved
    fresh = Solver(c, lam=lam).step()
    s.step()
    assert np.array_equal(s.host("X"), c["X"]) and np.array_equal(s.host("partials"), fresh.host("partials"))
    assert np.array_equal(s.host("pair_blocks"), fresh.host("pair_blocks"))


def test_the_rejected_candidate_is_the_exact_one(bound):
    """the step that is not taken is still the exact one: the same comparison as for an accepted step"""
    c, want = want_of(cases.REJECTED)
    check(cases.REJECTED, tolerance.errors(Solver(c).step().evaluation(), want, tolerance.EVALUATION), bound)


@pytest.mark.parametrize("name", cases.SMALL)
def test_finish_gives_the_exact_cost_pivot_errors_and_rows(name, bound):
    """on a fresh state, straight after the evaluation point is written: not converged is status 3, converged is status 0"""
    c, want = want_of(name)
    used = c["status"] == 0
    for converged, status in ((0.0, 3), (1.0, 0)):
        s = Solver(c, converged=converged, rows=True).finish()
        flags, lam, state = s.read()
        rows_a, rows_b = s.host("rows_a"), s.host("rows_b")
        got = dict(cost=state[N.BUNDLE_COST], pivot=state[N.BUNDLE_PIVOT], pair_error=s.host("pair_error"), depth_a=rows_a[:, 2], depth_b=rows_b[:, 2])
        check(name, tolerance.errors(got, want, tolerance.FINAL, sums=False), bound)
        assert state[N.BUNDLE_STATUS] == status and flags[2] == 0 and lam == float(c["lam"]) and state[N.BUNDLE_ACCEPT] == 0
        points = s.host("points")
        assert np.array_equal(points[c["src"]], c["X"]) and np.isnan(points[~used]).all()
        assert np.array_equal(rows_a[:, :2], c["uvs_a"][used].astype(np.float64)) and np.array_equal(rows_b[:, :2], c["uvs_b"][used].astype(np.float64))
        pair_of = np.repeat(np.arange(s.pairs), s.used_counts)
        assert np.array_equal(rows_a[:, 3], LABEL0 + c["pairs"][pair_of, 1]) and np.array_equal(rows_b[:, 3], LABEL0 + c["pairs"][pair_of, 0])


@pytest.mark.parametrize("pair", cases.SUBSET[1])
def test_a_pairs_sums_depend_on_nothing_else(pair):
    """a pair's block among the ten pairs of five views equals, bit for bit, its block in a problem of three views"""
    c, _ = want_of(cases.SUBSET[0])
    whole = Solver(c).step().host("pair_blocks")
    sub, at = cases.subproblem(c, pair)
    alone = Solver(sub).step().host("pair_blocks")
    assert np.array_equal(whole[pair], alone[at])


def test_16385_matches_of_one_pair_sum_their_partials_in_strides(bound):
    """65 chunks: lane 0 of k_bundle_pair_sum takes two.  The pairs' blocks and the state's numbers against the exact
    fixture; every pair's block against the exactly rounded sum of the GPU's own partials"""
    c, want = want_of(cases.MANY)
    assert cases.used_counts(c)[0] == 64 * 256 + 1 and "partials" not in want
    s = Solver(c).step()
    flags, lam, state = s.read()
    assert flags == (1, 1, 1, 1, 0) and lam == float(c["lam"]) * 0.1 and len(s.table) == 65 + 2
    got = tolerance.named(s.evaluation(), want)
    partials, blocks = got.pop("partials"), got["pair_blocks"]
    assert (partials[:, 103] == 0).all() and (blocks[:, 103] == 0).all()
    e = tolerance.errors(got, want, tolerance.EVALUATION)
    e["cost"] = relative(state[N.BUNDLE_COST], want["cost"])
    check(cases.MANY, e, bound)
    summed = np.array([[math.fsum(partials[int(s.ranges[p]):int(s.ranges[p + 1]), q]) for q in range(103)] for p in range(s.pairs)])
    check(cases.MANY + " (the blocks against the sum of the GPU's partials)", tolerance.block_errors(blocks, summed, want["pair_scale"]), bound)
    f = Solver(c, converged=1.0).finish()
    _, _, state = f.read()
    final = dict(cost=state[N.BUNDLE_COST], pivot=state[N.BUNDLE_PIVOT], pair_error=f.host("pair_error"))
    check(cases.MANY + " (finish)", tolerance.errors(final, want, ("cost", "pivot", "pair_error"), sums=False), bound)
    assert state[N.BUNDLE_STATUS] == 0
