"""Seeded synthetic rigs of the stereo calibration tests (tests/test_stereo_calibrate_cpu.py,
tests/test_gpu_stereo_calibrate.py).  Only DATA lives here.

Two cameras of ``pnp_cases.camera`` (five lens coefficients on both; one case without a lens on camera 1 and twelve
coefficients on camera 2), a true rig ``x2 = R x1 + t`` with a baseline of about 0.1 m and a few degrees of rotation, and
board poses (the board in camera 1) drawn from ``pnp_cases.poses`` and kept only where every corner lies inside both
images.  Frame counts on the edges of the four-frame workgroup and of the 64-frame partial sums of the frame reduction,
point counts on the edges of the 64-lane stride over points."""
import numpy as np

import pnp_cases as pc

W, H = pc.W, pc.H
NOISE_SIGMA = pc.NOISE_SIGMA
SEED, NOISY_SEED = 0, 4


def true_rig(seed=0):
    """(R, t): camera 1 -> camera 2, ~0.1 m to the side, a few degrees about every axis"""
    from calibrating_amd import geometry
    rng = np.random.default_rng([41, seed])
    R = geometry.rodrigues(np.array([0.02, -0.05, 0.01]) + rng.uniform(-0.01, 0.01, 3))
    t = np.array([-0.1, 0.004, 0.006]) + rng.uniform(-0.003, 0.003, 3)
    return R, t


def cameras(lenses=(5, 5), seed=0):
    (K1, D1), (K2, D2) = pc.camera(lenses[0], seed), pc.camera(lenses[1], seed + 1)
    flat = lambda D: None if D is None else np.array(D, np.float64).reshape(-1)  # noqa: E731
    return K1, flat(D1), K2, flat(D2)


def in_view(uv):
    return bool((uv[:, 0] > 0).all() and (uv[:, 0] < W - 1).all() and (uv[:, 1] > 0).all() and (uv[:, 1] < H - 1).all())


def poses(frames, board, cams, rig, seed=0):
    """the first ``frames`` poses of pnp_cases.poses under which both cameras see the whole board"""
    K1, D1, K2, D2 = cams
    T12 = np.eye(4)
    T12[:3, :3], T12[:3, 3] = rig
    out = []
    for T in pc.poses(6 * frames + 24, seed):
        if in_view(pc.observe(board, T, K1, D1)) and in_view(pc.observe(board, T12 @ T, K2, D2)):
            out.append(T)
        if len(out) == frames:
            return np.stack(out)
    raise AssertionError("pnp_cases.poses(%d, %d) holds fewer than %d poses in view of both cameras" % (6 * frames + 24, seed, frames))


def _spec(counts, lenses=(5, 5), bad=False, markers=False):
    return dict(counts=list(counts), lenses=lenses, bad=bad, markers=markers)


SPECS = {
    "f1-n70": _spec([70]),
    "f3-n70": _spec([70] * 3),
    "f4-n70": _spec([70] * 4),
    "f5-n70": _spec([70] * 5),
    "f63-n12": _spec([12] * 63),
    "f64-n12": _spec([12] * 64),
    "f65-n12": _spec([12] * 65),
    "f130-n12": _spec([12] * 130),
    "f5-n4": _spec([4] * 5),
    "f5-n63": _spec([63] * 5),
    "f5-n64": _spec([64] * 5),
    "f5-n65": _spec([65] * 5),
    "f5-n130": _spec([130] * 5),
    "ragged": _spec([12, 63, 64, 65, 130, 70]),
    "lens-0-12": _spec([70] * 5, lenses=(0, 12)),
    "markers": _spec([70] * 5, markers=True),
    # frame 1 keeps 3 points, frame 3 holds a NaN in camera 2 only, frame 4 is seen head-on by camera 1 (and, but for the
    # rig's few degrees, by camera 2): the first two are left out, the third is a frame like any other
    "bad-frames": _spec([70] * 6, bad=True),
}
NAMES = list(SPECS)
BAD_STATUS = {1: 1, 3: 2, 4: 0}
MARKER_IDS = (5, 9, 2)  # camera 1 sees every id; 35 + 20 + 15 corners
MARKER_SPLIT = (35, 55)
MARKERS_MISSED = {1: (9,), 3: (5, 2)}  # frame -> the ids camera 2 did not see there


def case(name, sigma=0.0, seed=0):
    """dict(obj: [(n, 3)], uv1, uv2: [(n, 2)], counts, T (f, 4, 4): the board in camera 1, K1, D1, K2, D2, R, t, bad: the
    planted frames -> their status word).  The ``markers`` case holds the conjoint points of ``marker_frames``."""
    s = SPECS[name]
    cams = cameras(s["lenses"], seed)
    K1, D1, K2, D2 = cams
    R, t = true_rig(seed)
    counts = s["counts"]
    T12 = np.eye(4)
    T12[:3, :3], T12[:3, 3] = R, t
    Ts = poses(len(counts), pc.centred(pc.board_points(max(counts))), cams, (R, t), seed + sum(counts))
    if s["bad"]:
        Ts[4, :3, :3] = np.eye(3)
    objs, uv1s, uv2s = [], [], []
    for i, (n, T) in enumerate(zip(counts, Ts)):
        obj = pc.centred(pc.board_points(n))
        objs.append(obj)
        uv1s.append(pc.observe(obj, T, K1, D1, sigma, seed + 31 * i))
        uv2s.append(pc.observe(obj, T12 @ T, K2, D2, sigma, seed + 31 * i + 17))
    bad = {}
    if s["bad"]:
        objs[1], uv1s[1], uv2s[1] = objs[1][:3], uv1s[1][:3], uv2s[1][:3]
        uv2s[3] = uv2s[3].copy()
        uv2s[3][33, 1] = np.nan
        bad = dict(BAD_STATUS)
    if s["markers"]:
        keep =[np.concatenate([np.arange(70)[_marker_slice(m)] for m in MARKER_IDS if m not in MARKERS_MISSED.get(i, ())])
                for i in range(len(counts))]
        objs, uv1s, uv2s = [o[k] for o, k in zip(objs, keep)], [u[k] for u, k in zip(uv1s, keep)], [u[k] for u, k in zip(uv2s, keep)]
    return dict(name=name, obj=objs, uv1=uv1s, uv2=uv2s, counts=[len(o) for o in objs], T=Ts, K1=K1, D1=D1, K2=K2, D2=D2, R=R, t=t,
                bad=bad)


def _marker_slice(marker):
    at = MARKER_IDS.index(marker)
    edges = (0,) + MARKER_SPLIT + (70,)
    return slice(edges[at], edges[at + 1])


def marker_frames(objs, uv1s, uv2s):
    """the frames of a 70-corner case as the reference's id -> points dicts (camera 1: every id, in MARKER_IDS' order;
    camera 2 misses MARKERS_MISSED) -> (frames of camera 1, frames of camera 2), key -> dict(image_points, object_points)"""
    frames1, frames2 = {}, {}
    for i, (o, a, b) in enumerate(zip(objs, uv1s, uv2s)):
        key = "f%d" % i
        seen2 = [m for m in MARKER_IDS if m not in MARKERS_MISSED.get(i, ())]
        frames1[key] = dict(image_points={m: a[_marker_slice(m)] for m in MARKER_IDS},
                            object_points={m: o[_marker_slice(m)] for m in MARKER_IDS})
        frames2[key] = dict(image_points={m: b[_marker_slice(m)] for m in seen2}, object_points={m: o[_marker_slice(m)] for m in seen2})
    return frames1, frames2


def rows(c):
    """the ragged rows of a case: (object (N, 3), image 1 (N, 2), image 2 (N, 2), counts)"""
    return np.concatenate(c["obj"]), np.concatenate(c["uv1"]), np.concatenate(c["uv2"]), c["counts"]


def case_from_pixels(frames=5, n=70, seed=0):
    """Board frames whose image rows ARE float32 in both cameras.  One board cannot be made to project onto drawn float32
    pixels in two cameras at once (calibrate_cases.case_from_pixels' construction), so the board's projections rounded to
    float32 are the observations: the same numbers as float32 and as float64 rows, and noisy by up to half a float32
    ulp of a pixel (3e-5 px).  dict(obj (n, 3) shared, uv1, uv2 (frames, n, 2) float32, T, K1, D1, K2, D2, R, t)."""
    c = case("f%d-n%d" % (frames, n) if "f%d-n%d" % (frames, n) in SPECS else "f5-n70", seed=seed)
    return dict(c, obj=c["obj"][0], uv1=np.stack(c["uv1"]).astype(np.float32), uv2=np.stack(c["uv2"]).astype(np.float32))


def perturbed_rig(R, t, seed=0):
    """a start for CALIB_USE_EXTRINSIC_GUESS: ~1 degree and ~5 mm off the truth"""
    from calibrating_amd import geometry
    rng = np.random.default_rng([43, seed])
    return geometry.rodrigues(rng.uniform(-0.02, 0.02, 3)) @ R, t + rng.uniform(-0.005, 0.005, 3)
