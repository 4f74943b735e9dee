"""Seeded cases of the stage tests of the two joint solvers (tests/test_solver_stage_cpu.py,
tests/test_gpu_solver_stages.py): one evaluation point per case, OFF the minimum, at which ``camd_calib_*`` and
``camd_stereo_*`` are driven stage by stage.  Only DATA lives here.

The boards, cameras, rigs, poses and the noise are pnp_cases', calibrate_cases' and stereo_calibrate_cases'.  Every case
has noisy detections (``NOISE_SIGMA``) and a perturbed start -- ``pnp_cases.perturbed`` on every frame's pose,
``perturbed_rig`` on the rig, the free intrinsics off by up to a percent --, so that residuals are pixels, not rounding
noise, and nothing cancels in the gradients.  Point counts lie on the edges of the 64-lane stride over a frame's points
(4, 63, 64, 65, 130, and a ragged mix of 4 and 130), frame counts on the edges of the four-frame workgroup (1, 3, 4, 5) and
of the 64-frame strides (65); 4097 frames of four points put a 65th partial before ``k_stereo_solve``.

A case is a dict of arrays, the same for both solvers: kind ("calib" / "stereo"), obj (rows, 3), uv or uv1 and uv2
(rows, 2), counts, shared (the object rows are one block every frame reads from its start), poses (frames, 12: R
row-major, t), lam; calib: k (9: fx fy cx cy k1 k2 p1 p2 k3) and mask (9); stereo: rig (12), K1, K2 (9), D1, D2."""
import numpy as np

import calibrate_cases as cc
import pnp_cases as pc
import stereo_calibrate_cases as sc

NOISE_SIGMA = pc.NOISE_SIGMA
SEED = 4
LAMBDA = 1e-3
RAGGED = [4, 130, 4, 130, 4]
FIX_K3 = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0.0])
FIX_PRINCIPAL_POINT = np.array([1, 1, 0, 0, 1, 1, 1, 1, 1.0])
FREE = np.ones(9)


def _spec(counts, mask=FREE, truth="lens", target="board", rows="f64", lenses=(5, 5), lam=LAMBDA, far=0.0):
    return dict(counts=list(counts), mask=mask, truth=truth, target=target, rows=rows, lenses=lenses, lam=lam, far=far)


# one frame cannot fix nine intrinsics from a plane: that case looks at a cloud
CALIB = {
    "calib-f1-n130-cloud": _spec([130], target="cloud"),
    "calib-f3-n63": _spec([63] * 3),
    "calib-f4-n64-fix-k3": _spec([64] * 4, mask=FIX_K3, truth="k3=0"),
    "calib-f5-n65-fix-pp": _spec([65] * 5, mask=FIX_PRINCIPAL_POINT, truth="centred"),
    "calib-f65-n4": _spec([4] * 65),
    "calib-ragged": _spec(RAGGED),
    "calib-f3-n65-f32": _spec([65] * 3, rows="f32"),
    "calib-f4-n63-shared": _spec([63] * 4, rows="shared"),
}
STEREO = {
    "stereo-f1-n130": _spec([130]),
    "stereo-f3-n63-lens-0-12": _spec([63] * 3, lenses=(0, 12)),
    "stereo-f4-n64-lens-4-8": _spec([64] * 4, lenses=(4, 8)),
    "stereo-f5-n65": _spec([65] * 5),
    "stereo-f65-n4": _spec([4] * 65),
    "stereo-ragged-lens-4-8": _spec(RAGGED, lenses=(4, 8)),
    "stereo-f3-n65-f32-lens-0-12": _spec([65] * 3, rows="f32", lenses=(0, 12)),
    "stereo-f4-n63-shared": _spec([63] * 4, rows="shared"),
    # a rig turned ``far`` = 0.6 rad about every axis and next to no damping: the near-Gauss-Newton step overshoots (the
    # candidate's cost is 3.6 times the current one) and is rejected
    "stereo-f5-n12-rejected": _spec([12] * 5, lam=1e-9, far=0.6),
}
# float32 rows of one shared four-point board: what the fixture stores of it are float32 values, exact in both types
MANY = "stereo-f4097-n4-f32-shared"
STEREO_MANY = {MANY: _spec([4] * 4097, rows="f32-shared")}
SMALL = list(CALIB) + list(STEREO)
NAMES = SMALL + [MANY]
REJECTED = "stereo-f5-n12-rejected"
SUBSET = ("calib-f5-n65-fix-pp", "stereo-f5-n65", (0, 2, 3))  # the cases of the `used` test and the frames it keeps
F65 = ("calib-f65-n4", "stereo-f65-n4")
INPUT_KEYS = {"calib": ("obj", "uv", "counts", "shared", "poses", "lam", "k", "mask"),
              "stereo": ("obj", "uv1", "uv2", "counts", "shared", "poses", "lam", "rig", "K1", "K2", "D1", "D2")}


def kind_of(name):
    return name.split("-")[0]


def pose12(T):
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])


def _rows(objs, uvs, rows):
    """the object and image rows as the case hands them over"""
    shared = rows in ("shared", "f32-shared")
    obj = objs[0] if shared else np.concatenate(objs)
    uvs = [np.concatenate(u) for u in uvs]
    if rows in ("f32", "f32-shared"):
        obj, uvs = obj.astype(np.float32), [u.astype(np.float32) for u in uvs]
    return obj, uvs, shared


def calib_case(name):
    s = CALIB[name]
    K, D = cc.true_camera(s["truth"], SEED)
    counts = s["counts"]
    Ts = cc.poses(len(counts), SEED + sum(counts))
    objs, uvs = [], []
    for i, (n, T) in enumerate(zip(counts, Ts)):
        obj = pc.centred(pc.board_points(n)) if s["target"] == "board" else pc.cloud_points(n, SEED)
        objs.append(obj)
        uvs.append(pc.observe(obj, T, K, D, NOISE_SIGMA, SEED + 31 * i))
    obj, (uv,), shared = _rows(objs, [uvs], s["rows"])
    k = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], *D[:5]])
    off = 1 + 0.01 * np.random.default_rng([47, SEED, len(counts)]).uniform(-1, 1, 9)
    k = np.where(s["mask"] != 0, k * off, k)
    poses = np.stack([pose12(pc.perturbed(T, SEED + i)) for i, T in enumerate(Ts)])
    return dict(kind="calib", name=name, obj=obj, uv=uv, counts=np.array(counts, np.int64), shared=np.array(shared), poses=poses,
                lam=np.array(s["lam"]), k=k, mask=np.array(s["mask"], np.float64))


def cameras(lenses, seed):
    """stereo_calibrate_cases.cameras, with the four-coefficient lens as the five-coefficient one without k3"""
    out = []
    for at, nd in enumerate(lenses):
        K, D = pc.camera(5 if nd == 4 else nd, seed + at)
        out += [K, np.zeros(0) if D is None else np.array(D, np.float64).reshape(-1)[:nd]]
    return tuple(out)


def stereo_case(name):
    s = (STEREO_MANY if name == MANY else STEREO)[name]
    K1, D1, K2, D2 = cams = cameras(s["lenses"], SEED)
    R, t = sc.true_rig(SEED)
    counts = s["counts"]
    T12 = np.eye(4)
    T12[:3, :3], T12[:3, 3] = R, t
    Ts = sc.poses(len(counts), pc.centred(pc.board_points(max(counts))), cams, (R, t), SEED + sum(counts))
    objs, uv1s, uv2s = [], [], []
    for i, (n, T) in enumerate(zip(counts, Ts)):
        obj = pc.centred(pc.board_points(n))
        objs.append(obj)
        uv1s.append(pc.observe(obj, T, K1, D1, NOISE_SIGMA, SEED + 31 * i))
        uv2s.append(pc.observe(obj, T12 @ T, K2, D2, NOISE_SIGMA, SEED + 31 * i + 17))
    obj, (uv1, uv2), shared = _rows(objs, [uv1s, uv2s], s["rows"])
    R0, t0 = sc.perturbed_rig(R, t, SEED)
    if s["far"]:
        from calibrating_amd import geometry
        R0 = geometry.rodrigues(np.array([1.0, -1.0, 1.0]) * s["far"]) @ R0
    poses = np.stack([pose12(pc.perturbed(T, SEED + i)) for i, T in enumerate(Ts)])
    if name == MANY:
        poses = poses.astype(np.float32).astype(np.float64)  # (stored as float32: R is then a matrix near a rotation)
    return dict(kind="stereo", name=name, obj=obj, uv1=uv1, uv2=uv2, counts=np.array(counts, np.int64), shared=np.array(shared),
                poses=poses, lam=np.array(s["lam"]), rig=np.concatenate([R0.reshape(9), t0]), K1=K1.reshape(9), K2=K2.reshape(9),
                D1=D1, D2=D2)


def case(name):
    return calib_case(name) if kind_of(name) == "calib" else stereo_case(name)


def frames_of(c):
    """per frame (obj (n, 3), [uv (n, 2) per camera], (R (3, 3), t (3,))) in float64: what one frame's sums read"""
    start = np.concatenate([[0], np.cumsum(c["counts"])])
    uvs = [c["uv"]] if c["kind"] == "calib" else [c["uv1"], c["uv2"]]
    out = []
    for f, n in enumerate(c["counts"]):
        s = int(start[f])
        obj = c["obj"][:n] if c["shared"] else c["obj"][s:s + n]
        out.append((obj.astype(np.float64), [u[s:s + n].astype(np.float64) for u in uvs],
                    (c["poses"][f, :9].reshape(3, 3).copy(), c["poses"][f, 9:].copy())))
    return out


def subset(c, frames):
    """the case of these frames alone (rows, counts and poses)"""
    start = np.concatenate([[0], np.cumsum(c["counts"])])
    take = np.concatenate([np.arange(start[f], start[f + 1]) for f in frames])
    out = dict(c, counts=c["counts"][list(frames)], poses=c["poses"][list(frames)])
    for k in ("uv", "uv1", "uv2"):
        if k in c:
            out[k] = c[k][take]
    if not c["shared"]:
        out["obj"] = c["obj"][take]
    return out
