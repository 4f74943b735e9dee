"""The stages of the two joint solvers on the MI355X (-m gpu), each driven alone through ``_native.call`` as
``calibrate.py`` and ``stereo_calibrate.py`` drive them, against the exact fixture tests/golden/solver_stage_exact.npz
within the bounds of tests/golden/solver_stage_tolerance.json (measured on the NumPy restatements, never on a kernel):
``camd_calib_linearise / step / finish`` and ``camd_stereo_linearise / step / finish`` at one evaluation point off the
minimum per case.  Every buffer has its documented size and starts as zeros; the stages are called in the package's
order only.  Nothing here needs mpmath."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from calibrating_amd import _native, pnp  # noqa: E402
from calibrating_amd._arrays import dist, to_device  # noqa: E402

import solver_stage_cases as cases  # noqa: E402
import solver_stage_tolerance as tolerance  # noqa: E402

N = _native
PLACES = {"calib": dict(done=N.CALIB_DONE, accept=N.CALIB_ACCEPT, lam=N.CALIB_LAMBDA, cost=N.CALIB_COST, evaluations=N.CALIB_EVALUATIONS,
                        iterations=N.CALIB_ITERATIONS, status=N.CALIB_STATUS, converged=N.CALIB_CONVERGED, solved=N.CALIB_SOLVED,
                        pivot=N.CALIB_PIVOT, start=slice(N.CALIB_K, N.CALIB_K + 9), step=slice(N.CALIB_DK, N.CALIB_DK + 9)),
          "stereo": dict(done=N.STEREO_DONE, accept=N.STEREO_ACCEPT, lam=N.STEREO_LAMBDA, cost=N.STEREO_COST,
                         evaluations=N.STEREO_EVALUATIONS, iterations=N.STEREO_ITERATIONS, status=N.STEREO_STATUS,
                         converged=N.STEREO_CONVERGED, solved=N.STEREO_SOLVED, pivot=N.STEREO_PIVOT,
                         start=slice(N.STEREO_RIG, N.STEREO_RIG + 12), step=slice(N.STEREO_STEP, N.STEREO_STEP + 6),
                         candidate=slice(N.STEREO_CANDIDATE, N.STEREO_CANDIDATE + 12))}
SIZES = {"calib": (N.CALIB_STATE_DOUBLES, N.CALIB_WORKSPACE_DOUBLES, N.CALIB_CANDIDATE_DOUBLES),
         "stereo": (N.STEREO_STATE_DOUBLES, N.STEREO_WORKSPACE_DOUBLES, N.STEREO_CANDIDATE_DOUBLES)}


class Solver:
    """One case on the device: the points as the package packs them, the frames ``used`` of them (all by default), and
    zero-filled buffers of the sizes include/calibrating_amd.h documents."""

    def __init__(self, c, used=None, converged=0.0):
        self.c, self.kind, self.at = c, c["kind"], PLACES[c["kind"]]
        counts = np.asarray(c["counts"], np.int64)
        used = np.arange(len(counts)) if used is None else np.asarray(used)
        self.n = n = len(used)
        first = c["uv"] if self.kind == "calib" else c["uv1"]
        self.pts, self.dev, self.alive = pnp.pack_points(np.array(c["obj"]), np.array(first), counts, bool(c["shared"]))  # (copies: the fixture is read-only)
        f64 = dict(dtype=torch.float64, device=self.dev)
        states, ws, cand = SIZES[self.kind]
        host = np.zeros(states)
        host[self.at["lam"]] = float(c["lam"])
        host[self.at["converged"]] = converged
        host[self.at["start"]] = c["k"] if self.kind == "calib" else c["rig"]
        if self.kind == "calib":
            host[N.CALIB_MASK:N.CALIB_MASK + 9] = c["mask"]
        self.state = torch.from_numpy(host).to(self.dev)
        self.used = torch.from_numpy(used.astype(np.int32)).to(self.dev)
        self.poses = torch.from_numpy(np.array(c["poses"][used], np.float64)).to(self.dev)
        self.ws, self.cand, self.err = torch.zeros((n, ws), **f64), torch.zeros((n, cand), **f64), torch.zeros(n, **f64)
        if self.kind == "stereo":
            img2 = to_device(np.array(c["uv2"]), device=self.dev).reshape(-1, 2)
            p = self.pts
            self.pts2 = N.PnpPoints(p.object, img2.data_ptr(), p.start, p.object_rows, img2.shape[0], p.object_type, p.image_type, 3, 2,
                                    p.object_shared, p.frames)
            self.partials = torch.zeros(((n + 63) // 64, N.STEREO_PARTIAL_DOUBLES), **f64)
            self.K = [np.ascontiguousarray(c[k], np.float64) for k in ("K1", "K2")]
            self.D = [dist(np.asarray(c[k], np.float64) if len(c[k]) else None) for k in ("D1", "D2")]
            self.alive += (img2,)
            self.rig = N.StereoRig(p, self.pts2, self.K[0].ctypes.data, self.D[0][1], self.K[1].ctypes.data, self.D[1][1],
                                   self.used.data_ptr(), self.state.data_ptr(), self.poses.data_ptr(), self.cand.data_ptr(),
                                   self.ws.data_ptr(), self.partials.data_ptr(), self.err.data_ptr(), self.D[0][2], self.D[1][2], n, 0)

    def _calib(self, name, *buffers):
        N.call(name, self.dev, ctypes.byref(self.pts), self.used.data_ptr(), self.n, self.state.data_ptr(),
               *(b.data_ptr() for b in buffers), what="stage test")

    def linearise(self):
        if self.kind == "calib":
            self._calib("camd_calib_linearise", self.poses, self.ws)
        else:
            N.call("camd_stereo_linearise", self.dev, ctypes.byref(self.rig), what="stage test")
        return self

    def step(self):
        if self.kind == "calib":
            self._calib("camd_calib_step", self.poses, self.cand, self.ws)
        else:
            N.call("camd_stereo_step", self.dev, ctypes.byref(self.rig), what="stage test")
        return self

    def finish(self):
        if self.kind == "calib":
            self._calib("camd_calib_finish", self.ws, self.err)
        else:
            N.call("camd_stereo_finish", self.dev, ctypes.byref(self.rig), what="stage test")
        return self

    def read(self):
        """(state, name -> its places' values) through camd_calib_read, as the package reads it"""
        out = np.empty(len(self.state))
        N.call("camd_calib_read", self.dev, self.state.data_ptr(), len(out), out.ctypes.data, what="stage test")
        return out, {k: out[v] for k, v in self.at.items()}

    def host(self, what):
        return getattr(self, what).cpu().numpy()

    def evaluation(self):
        """what one linearise + step left behind, in the layout of the exact fixture"""
        _, s = self.read()
        shared = s["start"] if self.kind == "calib" else s["candidate"]  # (calibrate: K has taken K + DK)
        return dict(ws=self.host("ws"), step=s["step"], shared=shared, cand=self.host("cand"))


def want_of(name):
    return tolerance.fixture()[name]


@pytest.fixture(scope="module")
def bound():
    return tolerance.load()["bound"]


def check(name, e, bound, keys=None):
    keys = sorted(e) if keys is None else keys
    print("%s: %s" % (name, ", ".join("%s %.3g (bound %.3g)" % (k, e[k], bound[k]) for k in keys)))
    assert all(e[k] <= bound[k] for k in keys), {k: (e[k], bound[k]) for k in keys if not e[k] <= bound[k]}


@pytest.mark.parametrize("name", cases.SMALL)
def test_linearise_gives_the_exact_sums(name, bound):
    """every entry of every frame's workspace within its block's bound of the exact sum, on the scale of its absolute
    products; a second call gives the same bits"""
    c, want = want_of(name)
    a, b = Solver(c).linearise(), Solver(c).linearise()
    ws = a.host("ws")
    check(name, tolerance.block_errors(c["kind"], ws, want["ws"], want["scale"]), bound)
    assert np.array_equal(ws, b.host("ws")) and np.array_equal(ws, a.linearise().host("ws"))
    assert np.array_equal(a.host("poses"), c["poses"])


@pytest.mark.parametrize("name", [n for n in cases.SMALL if n != cases.REJECTED])
def test_step_takes_the_exact_candidate(name, bound):
    """after linearise + step: the flags and counts, lambda's bits, the shared step, the candidate K or rig, every
    frame's candidate pose, cost, |step|^2 and |pose|^2 against the exact evaluation; then the hand-over into the next
    linearisation"""
    c, want = want_of(name)
    kind = c["kind"]
    s = Solver(c).linearise().step()
    state, at = s.read()
    assert bool(want["accept"])
    assert (at["solved"], at["accept"], at["evaluations"], at["iterations"], at["done"]) == (1, 1, 1, 1, 0)
    assert at["lam"] == float(c["lam"]) * 0.1
    got = s.evaluation()
    cand = got["cand"]
    e = tolerance.errors(kind, got, want, tolerance.EVALUATION)
    check(name, e, bound, ["%s/%s" % (kind, k) for k in tolerance.EVALUATION])
    if kind == "calib":
        fixed = c["mask"] == 0
        assert (at["step"][fixed] == 0).all() and np.array_equal(at["start"][fixed], c["k"][fixed])
        # what camd_calib_step's comment promises of an accepted step: poses and K took the candidate
        assert np.array_equal(at["start"], c["k"] + at["step"]) and np.array_equal(s.host("poses"), cand[:, :12])
    else:
        assert np.array_equal(at["start"], at["candidate"])
        assert np.array_equal(s.host("poses"), c["poses"])  # (the frames follow in the next linearisation)
    s.linearise()
    assert np.array_equal(s.host("poses"), cand[:, :12])
    cost2 = s.host("ws")[:, -1]
    again = float(np.abs(cost2 - cand[:, 12]).max() / np.abs(cand[:, 12]).min())
    print("%s: the candidates' costs in the next workspace differ by %.3g of the cost (bound %.3g)" % (name, again, bound[kind + "/c"]))
    assert again <= bound[kind + "/c"]


def test_a_rejected_step_moves_nothing():
    c, want = want_of(cases.REJECTED)
    assert not bool(want["accept"])
    s = Solver(c).linearise().step()
    state, at = s.read()
    assert (at["solved"], at["accept"], at["evaluations"], at["iterations"], at["done"]) == (1, 0, 1, 0, 0)
    assert at["lam"] == float(c["lam"]) * 10.0
    assert np.array_equal(at["start"], c["rig"]) and np.array_equal(s.host("poses"), c["poses"])
    ws = s.host("ws")
    assert np.array_equal(s.linearise().host("poses"), c["poses"]) and np.array_equal(s.host("ws"), ws)


def test_the_rejected_candidate_is_the_exact_one(bound):
    """the step that is not taken is still the exact one: the same comparison as for an accepted step"""
    c, want = want_of(cases.REJECTED)
    e = tolerance.errors("stereo", Solver(c).linearise().step().evaluation(), want, tolerance.EVALUATION)
    check(cases.REJECTED, e, bound, ["stereo/%s" % k for k in tolerance.EVALUATION])


@pytest.mark.parametrize("name", cases.SMALL)
def test_finish_gives_the_exact_cost_pivot_and_errors(name, bound):
    """straight after the first linearisation, on a fresh state: not converged is status 3, converged is status 0"""
    c, want = want_of(name)
    kind = c["kind"]
    for converged, status in ((0.0, 3), (1.0, 0)):
        s = Solver(c, converged=converged).linearise().finish()
        _, at = s.read()
        got = dict(cost=at["cost"], pivot=at["pivot"], frame_error=s.host("err"))
        e = {k: v for k, v in tolerance.errors(kind, dict(got, ws=s.host("ws")), want, tolerance.FINAL).items()}
        check(name, e, bound, ["%s/%s" % (kind, k) for k in tolerance.FINAL])
        assert at["status"] == status and at["evaluations"] == 0 and at["lam"] == float(c["lam"])


@pytest.mark.parametrize("name", cases.SUBSET[:2])
def test_a_used_list_that_skips_frames_is_the_call_on_those_frames(name):
    c, _ = want_of(name)
    frames = cases.SUBSET[2]
    a = Solver(c, used=frames).linearise().step().finish()
    alone = cases.subset(c, frames)
    b = Solver(alone).linearise().step().finish()
    assert np.array_equal(a.read()[0], b.read()[0])
    for what in ("ws", "cand", "poses", "err"):
        assert np.array_equal(a.host(what), b.host(what)), what


def test_4097_frames_sum_their_partials_in_strides(bound):
    """65 partials: k_stereo_solve's lane 0 takes two.  The state's numbers against the exact fixture; the workspace of
    16 frames against the float64 restatement on the restatement's own scale of absolute products"""
    c, want = want_of(cases.MANY)
    assert len(c["counts"]) == 4097 and "ws" not in want
    s = Solver(c).linearise().step()
    got = s.evaluation()
    _, at = s.read()
    assert (at["solved"], at["accept"], at["evaluations"], at["iterations"], at["done"]) == (1, 1, 1, 1, 0)
    _, at = s.finish().read()
    got.update(cost=at["cost"], pivot=at["pivot"])
    which = tolerance.STATE
    e = tolerance.errors("stereo", got, want, which)
    check(cases.MANY, e, bound, ["stereo/%s" % k for k in which])
    assert at["status"] == 3
    frames = [0, 1, 63, 64, 65, 127, 128, 1000, 2047, 2048, 4031, 4032, 4095, 4096, 3000, 4000]
    values, scale = tolerance.restated_sums(cases.subset(c, frames))
    check(cases.MANY + " (16 frames against the restatement)", tolerance.block_errors("stereo", got["ws"][frames], values, scale), bound)
