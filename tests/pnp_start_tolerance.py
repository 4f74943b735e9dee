"""How the start stage (``camd_pnp_init``, ``camd_calib_homography``) is compared with the exact fixture
tests/golden/pnp_start_exact.npz, and how far the float64 NumPy restatement (``pnp_ref.init_pose(..., null="kernel")``,
``calibrate_ref.homography``) lies from it.  No mpmath here: tests/golden/make_pnp_start_golden.py writes the fixture.

The yardstick.  The stage's answer is the eigenvector of M's smallest eigenvalue; a perturbation dM of M turns it by
|dM| / (lambda2 - lambda1), and the rounding of M's sums is 2^-52 of its entries, whose size is trace M.  So every
error is expressed in units of ``2^-52 kappa`` with ``kappa = trace M / (lambda2 - lambda1)`` of the frame, from the exact
fixture, and cases of different conditioning share one number:
    G        max |G - exact| over the entries, both of unit Frobenius norm, with the sign of the exact one
    pose     max over R's entries and over t's, the latter relative to max(1, |t|_inf): t carries the object's offset
    K0       ``initial_camera_matrix`` of a case's homographies: fx, fy relative, in units of the case's largest kappa
``measure()`` takes the restatement's errors over every case with the point rows in forward and in reversed order.  A
kernel differs from the restatement in the order of the same float64 arithmetic (lane-strided partial sums, then an xor
butterfly; contraction; its own Cholesky), so it is allowed ``FACTOR`` = 8 times the largest ratio found, the rule of
tests/pnp_tolerance.py.  ``KAPPA_CAP`` bounds the conditioning of a case: a case the restatement cannot do to 1e-9 is no
test of the kernel.  Nothing here comes from a kernel."""
import json
import os

import numpy as np

import calibrate_ref
import pnp_ref as ref
import pnp_start_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "pnp_start_exact.npz")
PATH = os.path.join(HERE, "golden", "pnp_start_tolerance.json")
FACTOR, ULP = 8, 2.0 ** -52
KAPPA_CAP = 2e4  # with the bounds below, 2^-52 kappa bound stays under POSE_ACCURACY for every quantity
POSE_ACCURACY = 1e-9
ARRAYS = ("obj", "uv_noisy", "uv_exact", "camera", "exact")  # of the fixture: tests/golden/make_pnp_start_golden.py
QUANTITIES = ("G/planar", "G/cloud", "G/homography", "pose", "K0")
XY = (6200, 4100)  # the image size of the homography cases' camera: its centre is (almost) HOMOGRAPHY_K's principal point

_LOADED = {}


def fixture():
    """name -> case: dict(name, kind, obj, uv, K, D, plane; G, pose, eigen, kappa: a row per frame), read once, shared by
    every test, never changed"""
    if not _LOADED:
        with np.load(FIXTURE) as z:
            z = {k: z[k] for k in ARRAYS}
        at = dict.fromkeys(ARRAYS, 0)

        def take(k, rows):
            at[k] += rows
            return z[k][at[k] - rows:at[k]].astype(np.float64)
        for name in cases.NAMES:
            _, n, frames, ndist, sigma = cases.SPEC[name]
            kind = cases.kind_of(name)
            cam, want = take("camera", 1)[0], take("exact", frames)
            c = dict(obj=take("obj", n), uv=take("uv_noisy" if sigma else "uv_exact", frames * n).reshape(frames, n, 2),
                     K=cam[:9].reshape(3, 3), plane=cam[9:18].reshape(3, 3), D=cam[18:18 + ndist],
                     G=want[:, :12 if kind == "cloud" else 9], pose=want[:, 12:24], eigen=want[:, 24:])
            c = {k: np.ascontiguousarray(v) for k, v in c.items()}
            c["kappa"] = c["eigen"][:, 2] / (c["eigen"][:, 1] - c["eigen"][:, 0])
            for v in c.values():
                v.setflags(write=False)
            c.update(name=name, kind=kind)
            _LOADED[name] = c
        assert all(at[k] == len(z[k]) for k in ARRAYS), "the fixture is not of this SPEC"
    return _LOADED


def normalised(G, like):
    """G (..., 9 or 12) at unit Frobenius norm, with the sign of ``like`` at ``like``'s entry of largest magnitude"""
    G, like = np.asarray(G, np.float64), np.asarray(like, np.float64)
    at = np.abs(like).argmax(-1)[..., None]
    with np.errstate(all="ignore"):
        s = np.sqrt((G * G).sum(-1, keepdims=True)) * np.sign(np.take_along_axis(G, at, -1)) * np.sign(np.take_along_axis(like, at, -1))
        return G / s


def g_error(G, c):
    """per frame: max |normalised G - exact| in units of 2^-52 kappa; infinite where G is not finite"""
    e = np.abs(normalised(G, c["G"]) - c["G"]).max(-1) / (ULP * c["kappa"])
    return np.where(np.isfinite(e), e, np.inf)


def pose_error(pose, c):
    """per frame: the error of R, t (frames, 12) in units of 2^-52 kappa; infinite where the pose is not finite"""
    d = np.abs(np.asarray(pose, np.float64) - c["pose"])
    e = np.maximum(d[:, :9].max(1), d[:, 9:].max(1) / np.maximum(1.0, np.abs(c["pose"][:, 9:]).max(1))) / (ULP * c["kappa"])
    return np.where(np.isfinite(e), e, np.inf)


def k0_error(K0, c):
    """the error of a homography case's start intrinsics against ``exact_k0(c)``, in units of 2^-52 of the largest kappa"""
    want = exact_k0(c)
    e = max(abs(K0[0, 0] - want[0, 0]) / want[0, 0], abs(K0[1, 1] - want[1, 1]) / want[1, 1]) / (ULP * c["kappa"].max())
    return float(e) if np.isfinite(e) else np.inf


def exact_k0(c):
    return calibrate_ref.initial_camera_matrix(c["G"].reshape(-1, 3, 3), XY)


def restated(c, reverse=False):
    """(G (frames, 9 or 12), pose (frames, 12) or None) of the restatement, the kernel's null vector, the point rows in
    forward or in reversed order"""
    o = slice(None, None, -1) if reverse else slice(None)
    obj, D = c["obj"][o], (c["D"] if len(c["D"]) else None)
    if c["kind"] == "homography":
        return np.stack([calibrate_ref.homography(obj, uv[o], c["plane"], null="kernel").reshape(-1) for uv in c["uv"]]), None
    planar = c["kind"] == "planar"
    X = (obj @ c["plane"].T)[:, :2] if planar else obj
    G = [ref.normalised_dlt(X, ref.points_ref.undistort_trace(uv[o], c["K"], D, iters=10)[0], "kernel").reshape(-1) for uv in c["uv"]]
    T = [ref.init_pose(obj, uv[o], c["K"], D, planar, c["plane"], null="kernel") for uv in c["uv"]]
    return np.stack(G), np.stack([np.concatenate([t[:3, :3].reshape(-1), t[:3, 3]]) for t in T])


def case_errors(c, G, pose=None, K0=None):
    """quantity -> the largest error over the case's frames"""
    out = {"G/" + c["kind"]: float(g_error(G, c).max())}
    if pose is not None:
        out["pose"] = float(pose_error(pose, c).max())
    if K0 is not None:
        out["K0"] = k0_error(K0, c)
    return out


def measure():
    """the restatement against the exact fixture over every case, forward and reversed -> the tolerance record"""
    worst, per_case = {}, {}
    for name, c in fixture().items():
        for reverse in (False, True):
            G, pose = restated(c, reverse)
            K0 = calibrate_ref.initial_camera_matrix(G.reshape(-1, 3, 3), XY) if c["kind"] == "homography" else None
            e = case_errors(c, G, pose, K0)
            worst.update({k: max(worst.get(k, 0.0), v) for k, v in e.items()})
            per_case[name] = {k: max(per_case.get(name, {}).get(k, 0.0), v) for k, v in e.items()}
        per_case[name]["kappa"] = float(c["kappa"].max())
    return dict(measured=worst, factor=FACTOR, ulp=ULP, kappa_cap=KAPPA_CAP, unit="2^-52 kappa",
                bound={k: FACTOR * v for k, v in worst.items()}, cases=per_case)


def load():
    with open(PATH) as f:
        return json.load(f)
