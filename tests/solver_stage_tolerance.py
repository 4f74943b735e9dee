"""How one evaluation of the two joint solvers is compared with the exact fixture, and how far the float64 NumPy
restatements (tests/calibrate_ref.py, tests/stereo_calibrate_ref.py) lie from it.  No mpmath here: the exact numbers are
read from tests/golden/solver_stage_exact.npz (tests/golden/make_solver_stage_golden.py writes it).

``errors(got, want)`` is the one comparison -- of the restatement for the measurement, of its mutations for the
sensitivity test, of the GPU's stages in tests/test_gpu_solver_stages.py.  Its yardsticks:
    A B C gp gk/gr c   |value - exact| / s per entry, s = sum_i |a_i| |b_i| (the fixture's ``scale``); an entry whose s is
                       0 is a sum of zeros and has to be 0
    step, shared       the shared step, and the candidate K = K + step: relative to |step|; the candidate rig, a pose: to 1
    pose               every frame's candidate R, t: to 1
    cand_cost, cost    relative to the cost;  step2, norm2, frame_error: relative to themselves
    pivot              absolute: it is a pivot of a matrix with a unit diagonal
``measure()`` takes the restatement's errors over every case with the points and frames in forward and in reversed order.
A GPU stage differs from the restatement in the order of the same float64 arithmetic (lane strides, butterflies,
contraction, its own Cholesky), so it is allowed ``FACTOR`` = 8 times the largest error found, as in
tests/calibrate_tolerance.py; a quantity the restatement happens to get exactly is allowed 8 roundings of 2^-52, the
precision of the format.  Every bound has to stay below ``CAP`` = 1e-10: a structural error is of order 1 on these scales.
Nothing here comes from the kernels."""
import json
import os

import numpy as np

import calibrate_ref
import solver_stage_cases as cases
import stereo_calibrate_ref

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "solver_stage_exact.npz")
PATH = os.path.join(HERE, "golden", "solver_stage_tolerance.json")
FACTOR, CAP, ULP = 8, 1e-10, 2.0 ** -52
# the workspace of one frame: kind -> slice
BLOCKS = {"calib": dict(A=slice(0, 21), B=slice(21, 75), C=slice(75, 120), gp=slice(120, 126), gk=slice(126, 135), c=slice(135, 136)),
          "stereo": dict(A=slice(0, 21), B=slice(21, 57), C=slice(57, 78), gp=slice(78, 84), gr=slice(84, 90), c=slice(90, 91))}
EVALUATION = ("step", "shared", "pose", "cand_cost", "step2", "norm2")
FINAL = ("cost", "pivot", "frame_error")
STATE = ("step", "shared", "cost", "pivot")  # all the fixture holds of the 4097-frame case
EXACT_KEYS = ("ws", "scale", "step", "shared", "cand", "cost", "cand_cost", "accept", "frames_definite", "reduced_definite", "pivot",
              "pivot_definite", "frame_error")


def kinds(solver, blocks=True):
    return ["%s/%s" % (solver, k) for k in (list(BLOCKS[solver]) if blocks else []) + list(EVALUATION + FINAL)]


def block_errors(solver, ws, exact, scale):
    """per block kind the largest |ws - exact| / scale; infinite where a sum of zeros is not 0"""
    ws, exact, scale = (np.asarray(a, np.float64) for a in (ws, exact, scale))
    with np.errstate(all="ignore"):
        e = np.where(scale > 0, np.abs(ws - exact) / scale, np.where(ws == exact, 0.0, np.inf))
    e = np.where(np.isfinite(ws), e, np.inf)
    return {"%s/%s" % (solver, k): float(e[:, s].max()) for k, s in BLOCKS[solver].items()}


def errors(solver, got, want, which=EVALUATION + FINAL):
    """name -> error of ``got`` against the exact ``want`` (the docstring's yardsticks): the blocks where ``want`` holds a
    workspace, then the quantities ``which`` names.  got, want: dict(ws, step, shared, cand, cost, pivot, frame_error)."""
    out = {}
    if "ws" in want:
        out.update(block_errors(solver, got["ws"], want["ws"], want["scale"]))
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, np.float64) - b) / np.abs(b)))  # noqa: E731
    size = float(np.sqrt((want["step"] ** 2).sum()))
    for k in which:
        if k == "step":
            e = float(np.abs(got["step"] - want["step"]).max()) / size
        elif k == "shared":
            e = float(np.abs(got["shared"] - want["shared"]).max()) / (size if solver == "calib" else 1.0)
        elif k == "pose":
            e = float(np.abs(got["cand"][:, :12] - want["cand"][:, :12]).max())
        elif k in ("cand_cost", "step2", "norm2"):
            at = 12 + ("cand_cost", "step2", "norm2").index(k)
            e = rel(got["cand"][:, at], want["cand"][:, at])
        elif k == "pivot":
            e = abs(float(got["pivot"]) - float(want["pivot"]))
        else:
            e = rel(got[k], want[k])
        out["%s/%s" % (solver, k)] = e if np.isfinite(e) else np.inf
    return out


# ---- the restatement, stage by stage ------------------------------------------------------------------------------
def _tri(M):
    return M[np.tril_indices(len(M))]


def pack(lin):
    """the restatement's per-frame sums in the kernels' packing: A | B row-major | C | gp | gk or gr | c"""
    return np.stack([np.concatenate([_tri(A), B.reshape(-1), _tri(C), gp, gs, [c]]) for A, B, C, gp, gs, c in lin])


def camera(K9, D):
    return np.asarray(K9, np.float64).reshape(3, 3), (None if len(D) == 0 else np.asarray(D, np.float64))


def linearised(c, reverse=False):
    """(per-frame sums of the restatement, what its other stages need) with the points in forward or in reversed order;
    the frames stay in their order"""
    frames = cases.frames_of(c)
    order = slice(None, None, -1) if reverse else slice(None)
    objs, poses = [f[0][order] for f in frames], [f[2] for f in frames]
    if c["kind"] == "calib":
        uvs = [f[1][0][order] for f in frames]
        return calibrate_ref.linearise(poses, objs, uvs, c["k"]), (poses, objs, uvs)
    uv1s, uv2s = [f[1][0][order] for f in frames], [f[1][1][order] for f in frames]
    cams = camera(c["K1"], c["D1"]) + camera(c["K2"], c["D2"])
    R, t = c["rig"][:9].reshape(3, 3), c["rig"][9:]
    return stereo_calibrate_ref.linearise(poses, R, t, objs, uv1s, uv2s, cams), (poses, R, t, objs, uv1s, uv2s, cams)


def stages(c, lin, rest, reverse=False, step=None):
    """The restatement's float64 evaluation from its own sums, in the layout of the exact fixture.  ``reverse`` sums the
    frames in reversed order.  ``step``: (shared step, factors) computed elsewhere (the sensitivity test's mutations)."""
    order = slice(None, None, -1) if reverse else slice(None)
    turned = lambda rows: list(rows)[order]  # noqa: E731
    lam = float(c["lam"])
    lin_o = turned(lin)
    if c["kind"] == "calib":
        poses, objs, uvs = rest
        free = c["mask"] != 0
        ds, Ls = calibrate_ref.shared_step(lin_o, lam, free) if step is None else step
        r = calibrate_ref.candidates(lin_o, Ls, turned(poses), turned(objs), turned(uvs), c["k"], ds)
        shared = r["k2"]
        pivot, cost = calibrate_ref.final_stage(lin_o, free)
        per_point = 1.0
    else:
        poses, R, t, objs, uv1s, uv2s, cams = rest
        ds, Ls = stereo_calibrate_ref.shared_step(lin_o, lam) if step is None else step
        r = stereo_calibrate_ref.candidates(lin_o, Ls, turned(poses), R, t, turned(objs), turned(uv1s), turned(uv2s), cams, ds)
        shared = np.concatenate([r["R2"].reshape(9), r["t2"]])
        pivot, cost = stereo_calibrate_ref.final_stage(lin_o)
        per_point = 2.0
    cand = np.stack([np.concatenate([Rf.reshape(9), tf, [c2, s2, n2, 0.0]])
                     for (Rf, tf), c2, s2, n2 in zip(r["poses2"], r["cost2"], r["step2"], r["norm2"])])[order]
    return dict(ws=pack(lin), step=ds, shared=shared, cand=cand, cost=np.float64(cost), pivot=np.float64(pivot), accept=r["accept"],
                frame_error=np.sqrt(np.array([l[5] for l in lin]) / (per_point * c["counts"])))


def restated(c, reverse=False):
    lin, rest = linearised(c, reverse)
    return stages(c, lin, rest, reverse)


def restated_sums(c):
    """(the restatement's workspace, its own scale: the same sums over the absolute values of every factor) in float64"""
    frames = cases.frames_of(c)
    if c["kind"] == "calib":
        terms = [calibrate_ref.frame_terms(R, t, obj, uv, c["k"]) for obj, (uv,), (R, t) in frames]
        sums = calibrate_ref.blocks
    else:
        cams = camera(c["K1"], c["D1"]) + camera(c["K2"], c["D2"])
        terms = [stereo_calibrate_ref.frame_terms(Ri, ti, c["rig"][:9].reshape(3, 3), c["rig"][9:], obj, u1, u2, cams)
                 for obj, (u1, u2), (Ri, ti) in frames]
        sums = stereo_calibrate_ref.blocks
    return pack([sums(*t) for t in terms]), pack([sums(*(np.abs(a) for a in t)) for t in terms])


# ---- the fixture and the measurement --------------------------------------------------------------------------------
_LOADED = {}


def fixture():
    """name -> (case, exact): read once, shared by every test, never changed"""
    if not _LOADED:
        with np.load(FIXTURE) as z:
            for name in cases.NAMES:
                kind = cases.kind_of(name)
                c = {k: z["%s/in/%s" % (name, k)] for k in cases.INPUT_KEYS[kind]}
                c.update(kind=kind, name=name, poses=c["poses"].astype(np.float64))
                want = {k: z["%s/exact/%s" % (name, k)] for k in EXACT_KEYS if "%s/exact/%s" % (name, k) in z.files}
                for v in list(c.values()) + list(want.values()):
                    if isinstance(v, np.ndarray):
                        v.setflags(write=False)
                _LOADED[name] = (c, want)
    return _LOADED


def conditions(want):
    """what the issue asks of a case, from the exact numbers alone: the relative change of the cost, the definiteness
    flags and the smallest unit-diagonal pivot"""
    return dict(cost_change=float((want["cand_cost"] - want["cost"]) / want["cost"]), pivot=float(want["pivot"]),
                definite=bool(want["frames_definite"] and want["reduced_definite"] and want["pivot_definite"]))


def measure(names=None):
    """the restatement against the exact fixture over every case, forward and reversed -> the tolerance record"""
    worst = {}
    for name, (c, want) in fixture().items():
        if names is not None and name not in names:
            continue
        for reverse in (False, True):
            e = errors(c["kind"], restated(c, reverse), want, EVALUATION + FINAL if "cand" in want else STATE)
            worst.update({k: max(worst.get(k, 0.0), v) for k, v in e.items()})
    return dict(measured=worst, factor=FACTOR, cap=CAP, ulp=ULP, bound={k: FACTOR * max(v, ULP) for k, v in worst.items()})


def load():
    with open(PATH) as f:
        return json.load(f)
