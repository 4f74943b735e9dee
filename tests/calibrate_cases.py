"""Seeded synthetic cases of the calibration tests (tests/test_calibrate_cpu.py, tests/test_gpu_calibrate.py).  Only DATA
lives here.

The board, the camera (``camera(5)``: fx ~ 1000 at 1280 x 720, five lens coefficients) and ``observe`` are pnp_cases';
the poses are made for calibration: the board's centre 0.3 .. 1.0 m in front of the camera, the components of its
Rodrigues vector uniform in +-0.6, so that the frames together fix the focal lengths and the lens.  Frame counts on the
edges of the four-frame workgroup, 65 frames for the 64-lane stride over frames, point counts on the edges of the
64-lane stride over points."""
import numpy as np

import pnp_cases as pc


class cal:
    """cv2's flag values (the package exports the same names; kept apart so that the data needs no import of it)"""
    CALIB_USE_INTRINSIC_GUESS, CALIB_FIX_PRINCIPAL_POINT, CALIB_ZERO_TANGENT_DIST, CALIB_FIX_K3 = 1, 4, 8, 128
    UNDISTORTED_FLAGS = 8 + 32 + 64 + 128 + 2048 + 4096 + 8192  # the reference's undistorted=True: no lens at all


W, H = pc.W, pc.H
NOISE_SIGMA = pc.NOISE_SIGMA
# The seeds of the noise-free and of the noisy grid.  They were chosen on the CPU restatement (tests/calibrate_ref.py), as
# the poses decide two things: how far the homographies' focal lengths lie from the truth (0.7 % and 1.2 % at these
# seeds, up to 3.9 % at others), and whether the restatement agrees with itself under a change of summation order to
# below 1e-6 px in fx fy cx cy (tests/calibrate_tolerance.py asserts both for every case).
SEED, NOISY_SEED = 0, 4


def poses(frames, seed=0):
    from calibrating_amd import geometry
    rng = np.random.default_rng([29, seed, frames])
    out = []
    for _ in range(frames):
        z = rng.uniform(0.3, 1.0)
        T = np.eye(4)
        T[:3, :3] = geometry.rodrigues(rng.uniform(-0.6, 0.6, 3))
        T[:3, 3] = [rng.uniform(-0.2, 0.2) * z, rng.uniform(-0.1, 0.1) * z, z]
        out.append(T)
    return np.stack(out)


# name -> dict(counts: points per frame, flags, truth: how the true camera differs from camera(5), kind)
def _spec(counts, flags=0, truth="lens", kind="board", bad=False):
    return dict(counts=list(counts), flags=flags, truth=truth, kind=kind, bad=bad)


SPECS = {
    "f3-n70": _spec([70] * 3),
    "f4-n70": _spec([70] * 4),
    "f5-n70": _spec([70] * 5),
    "f9-n70": _spec([70] * 9),
    "f65-n12": _spec([12] * 65),
    "f5-n12": _spec([12] * 5),
    "f5-n63": _spec([63] * 5),
    "f5-n64": _spec([64] * 5),
    "f5-n65": _spec([65] * 5),
    "f5-n130": _spec([130] * 5),
    "ragged": _spec([12, 63, 64, 65, 130, 70]),
    "bad-frames": _spec([70] * 6, bad=True),  # frame 2 keeps 3 points, frame 3 holds a NaN
    "fix-k3": _spec([70] * 5, flags=cal.CALIB_FIX_K3, truth="k3=0"),
    "undistorted": _spec([70] * 5, flags=cal.UNDISTORTED_FLAGS, truth="no-lens"),
    "fix-principal-point": _spec([70] * 5, flags=cal.CALIB_FIX_PRINCIPAL_POINT, truth="centred"),
    "guess-cloud": _spec([65] * 5, flags=cal.CALIB_USE_INTRINSIC_GUESS, kind="cloud"),
}
NAMES = list(SPECS)
PARITY_FRAMES = "f9-n70"  # the case computed as ndarray, CUDA tensor and float32 rows


def true_camera(truth, seed=0):
    K, D = pc.camera(5, seed)
    D = np.array(D, np.float64).reshape(-1)
    if truth == "k3=0":
        D[4] = 0.0
    elif truth == "no-lens":
        D[:] = 0.0
    elif truth == "centred":
        K[0, 2], K[1, 2] = (W - 1) / 2, (H - 1) / 2
    return K, D


def case(name, sigma=0.0, seed=0):
    """dict(obj: [(n, 3)], uv: [(n, 2)], counts, T (f, 4, 4), K, D (5,), flags, xy, K_guess or None, bad: the frames that
    are not part of the joint problem -> their status word)."""
    s = SPECS[name]
    K, D = true_camera(s["truth"], seed)
    counts = s["counts"]
    Ts = poses(len(counts), seed + sum(counts))
    objs, uvs = [], []
    for i, (n, T) in enumerate(zip(counts, Ts)):
        obj = pc.centred(pc.board_points(n)) if s["kind"] == "board" else pc.cloud_points(n, seed)
        objs.append(obj)
        uvs.append(pc.observe(obj, T, K, D, sigma, seed + 31 * i))
    bad = {}
    if s["bad"]:
        objs[2], uvs[2] = objs[2][:3], uvs[2][:3]
        uvs[3] = uvs[3].copy()
        uvs[3][33, 0] = np.nan
        bad = {2: 1, 3: 2}
    guess = None
    if s["flags"] & cal.CALIB_USE_INTRINSIC_GUESS:
        guess = K.copy()
        guess[0, 0] *= 1.02
        guess[1, 1] *= 0.98
        guess[0, 2] += 6.0
        guess[1, 2] -= 5.0
    return dict(name=name, obj=objs, uv=uvs, counts=[len(o) for o in objs], T=Ts, K=K, D=D, flags=s["flags"], xy=(W, H),
                K_guess=guess, bad=bad)


def rows(c):
    """the ragged rows of a case: (object (N, 3), image (N, 2), counts)"""
    return np.concatenate(c["obj"]), np.concatenate(c["uv"]), c["counts"]


def case_from_pixels(frames=9, n=70, seed=0):
    """Noise-free board frames whose image rows ARE float32 (pnp_cases.case_from_pixels' construction under these poses):
    the pixels are drawn as float32 and the object points are where their rays meet the board's plane under the true
    pose.  dict(obj (frames, n, 3) float64, uv (frames, n, 2) float32, T, K, D)."""
    import points_ref
    K, D = true_camera("lens", seed)
    Ts = poses(frames, seed + n + 1)
    rng = np.random.default_rng([37, seed, n, frames])
    objs, uvs = [], []
    for T in Ts:
        centre = T[:3, 3] / T[2, 3]
        uv = (np.array([K[0, 0], K[1, 1]]) * (centre[:2] + rng.uniform(-0.12, 0.12, (n, 2))) + K[:2, 2]).astype(np.float32)
        rays = np.concatenate([points_ref.undistort_trace(uv, K, D, iters=50)[0], np.ones((n, 1))], 1)
        R, t = T[:3, :3], T[:3, 3]
        depth = (R[:, 2] @ t) / (rays @ R[:, 2])
        obj = (depth[:, None] * rays - t) @ R
        obj[:, 2] = 0.0
        objs.append(obj)
        uvs.append(uv)
    return dict(obj=np.stack(objs), uv=np.stack(uvs), T=Ts, K=K, D=D, xy=(W, H))
