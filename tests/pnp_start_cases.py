"""Seeded cases of the start stage of every solver here: ``camd_pnp_init`` (csrc/pnp.hip) and ``camd_calib_homography``
(csrc/calibrate.hip), both over ``direct_linear_transform`` + ``null_vector`` of csrc/pnp_common.hpp.  Only DATA lives
here; tests/golden/make_pnp_start_golden.py stores every case's rows in tests/golden/pnp_start_exact.npz next to its exact
answer, and the tests read them from there (tests/test_pnp_start_cpu.py checks that this file still generates them).

The generators are those of tests/pnp_cases.py.  The shapes are the smallest at which the kernels can go wrong: the fewest
points each start takes (4 and 5 on a plane, 6 and 7 in space) and the edges of the 64-lane stride (63, 64, 65, 128, 129);
1, 3, 4, 5 and 9 frames a call, around the four waves of a workgroup; every lens length the entry point accepts, at
``LENS_SCALE`` of pnp_cases' magnitudes so that the tenth undistortion round still moves the points; noise-free and
``pnp_cases.NOISE_SIGMA`` pixels of noise.  The planar targets beyond the centred board: a board at z = const != 0 off its
origin, a board tilted in its own object frame (``plane_of`` returns a rotation), and a board whose object origin lies
BEHIND the camera while the board is in front of it -- there H[8] has the wrong sign and only the centre term of the sign
test gives the right one; the same construction for the projection matrix.  The homography cases are the same boards
seen in raw pixels by a camera whose principal point lies in the thousands."""
import numpy as np

import pnp_cases as pc

LENS_SCALE = 12.0  # of pnp_cases.camera's coefficients: after nine rounds the points still move by more than their rounding
BEHIND_OFFSET = np.array([1.5, 0.9, 0.0])  # several board widths (0.225 m) between the object origin and the board
CLOUD_OFFSET = np.array([1.4, -0.8, 1.1])
HOMOGRAPHY_K = np.array([[3011.7, 0, 3100.5], [0, 2989.3, 2050.25], [0, 0, 1]])

# name: (target, points, frames, ndist, sigma)
PLANAR = {
    "planar-n4-f9-d0": ("board", 4, 9, 0, 0.0),
    "planar-n5-f5-d4-noisy": ("board", 5, 5, 4, pc.NOISE_SIGMA),
    "planar-n63-f3-d5-noisy": ("board", 63, 3, 5, pc.NOISE_SIGMA),
    "planar-n64-f1-d8": ("board", 64, 1, 8, 0.0),
    "planar-n65-f4-d12-noisy": ("board", 65, 4, 12, pc.NOISE_SIGMA),
    "planar-n128-f1-d14": ("board", 128, 1, 14, 0.0),
    "planar-n129-f1-d0-noisy": ("board", 129, 1, 0, pc.NOISE_SIGMA),
    "planar-z0-n20-f3-d5-noisy": ("z0", 20, 3, 5, pc.NOISE_SIGMA),
    "planar-tilted-n24-f3-d8-noisy": ("tilted", 24, 3, 8, pc.NOISE_SIGMA),
    "planar-behind-n12-f4-d0": ("behind", 12, 4, 0, 0.0),
    "planar-behind-n12-f4-d5-noisy": ("behind", 12, 4, 5, pc.NOISE_SIGMA),
}
CLOUD = {
    "cloud-n6-f9-d0": ("cloud", 6, 9, 0, 0.0),
    "cloud-n7-f5-d4-noisy": ("cloud", 7, 5, 4, pc.NOISE_SIGMA),
    "cloud-n63-f3-d5-noisy": ("cloud", 63, 3, 5, pc.NOISE_SIGMA),
    "cloud-n64-f1-d8": ("cloud", 64, 1, 8, 0.0),
    "cloud-n65-f4-d12-noisy": ("cloud", 65, 4, 12, pc.NOISE_SIGMA),
    "cloud-n128-f1-d14": ("cloud", 128, 1, 14, 0.0),
    "cloud-n129-f1-d0-noisy": ("cloud", 129, 1, 0, pc.NOISE_SIGMA),
    "cloud-behind-n16-f4-d0": ("cloud-behind", 16, 4, 0, 0.0),
    "cloud-behind-n16-f4-d5-noisy": ("cloud-behind", 16, 4, 5, pc.NOISE_SIGMA),
}
HOMOGRAPHY = {
    "homography-n4-f9": ("board", 4, 9, 0, 0.0),
    "homography-n5-f5-noisy": ("board", 5, 5, 0, pc.NOISE_SIGMA),
    "homography-n63-f1-noisy": ("board", 63, 1, 0, pc.NOISE_SIGMA),
    "homography-n64-f1": ("board", 64, 1, 0, 0.0),
    "homography-n65-f3-noisy": ("board", 65, 3, 0, pc.NOISE_SIGMA),
    "homography-n128-f1": ("board", 128, 1, 0, 0.0),
    "homography-n129-f1-noisy": ("board", 129, 1, 0, pc.NOISE_SIGMA),
    "homography-tilted-n24-f3-noisy": ("tilted", 24, 3, 0, pc.NOISE_SIGMA),
    "homography-behind-n12-f4-noisy": ("behind", 12, 4, 0, pc.NOISE_SIGMA),
}
SPEC = {**PLANAR, **CLOUD, **HOMOGRAPHY}
NAMES = list(SPEC)
OFF_ORIGIN = [n for n in NAMES if "behind" in n]
INPUT_KEYS = ("obj", "uv", "K", "D", "plane")


def kind_of(name):
    return name.split("-")[0]


def camera(ndist, seed=0):
    """(K, D) of pnp_cases.camera with a lens of any accepted length: the 12-coefficient lens cut to ``ndist``, or with
    tauX = tauY = 0 behind it, times LENS_SCALE"""
    K, D = pc.camera(12 if ndist else 0, seed)
    if ndist == 0:
        return K, np.zeros(0)
    return K, np.concatenate([D.reshape(-1)[:min(ndist, 12)] * LENS_SCALE, np.zeros(max(0, ndist - 12))])


def tilt(seed):
    from calibrating_amd import geometry
    return geometry.rodrigues(np.random.default_rng([29, seed]).uniform(-0.9, 0.9, 3))


def target(which, n, seed):
    """(local (n, 3): the target in the frame the poses act on, Rb, off): the caller's object points are local Rb^T + off"""
    I, o = np.eye(3), np.zeros(3)
    if which in ("cloud", "cloud-behind"):
        return pc.cloud_points(n, seed), I, (CLOUD_OFFSET if which == "cloud-behind" else o)
    B = pc.centred(pc.board_points(n))
    if which == "tilted":
        return B, tilt(seed), np.array([0.3, -0.2, 0.1])
    return B, I, {"board": o, "z0": np.array([0.07, -0.05, 0.4]), "behind": BEHIND_OFFSET}[which]


def behind_poses(frames, seed, offset):
    """poses that keep the target 0.5 .. 0.8 m in front of the camera and turn it so far that the object origin,
    ``offset`` away, has a negative depth"""
    from calibrating_amd import geometry
    rng = np.random.default_rng([31, seed, frames])
    out = []
    while len(out) < frames:
        T = np.eye(4)
        T[:3, :3] = geometry.rodrigues(rng.uniform(-0.6, 0.6, 3))
        z = rng.uniform(0.5, 0.8)
        T[:3, 3] = [rng.uniform(-0.1, 0.1) * z, rng.uniform(-0.05, 0.05) * z, z]
        if (T[:3, 3] - T[:3, :3] @ offset)[2] < -0.1:
            out.append(T)
    return np.stack(out)


def case(name, seed=9):
    """dict(name, kind, obj (n, 3) shared by the frames, uv (frames, n, 2) raw pixels, K (3, 3), D (ndist,), plane (3, 3),
    T (frames, 4, 4) the true poses in the caller's object frame)"""
    from calibrating_amd import pnp
    kind = kind_of(name)
    which, n, frames, ndist, sigma = SPEC[name]
    K, D = (HOMOGRAPHY_K, np.zeros(0)) if kind == "homography" else camera(ndist, seed)
    local, Rb, off = target(which, n, seed)
    obj = (local @ Rb.T + off).astype(np.float32).astype(np.float64)  # float32 values are the data: the fixture stores them so
    local = (obj - off) @ Rb
    Ts = behind_poses(frames, seed + n, off) if "behind" in which else pc.poses(max(frames, 4), seed + n)
    if frames == 1:  # the one of four that lies farthest from the optical axis, where the lens acts
        Ts = Ts[[np.argmax(np.hypot(Ts[:, 0, 3], Ts[:, 1, 3]) / Ts[:, 2, 3])]]
    Ts = Ts[:frames]
    uv = np.stack([pc.observe(local, T, K, D if len(D) else None, sigma, seed + 31 * i) for i, T in enumerate(Ts)])
    if sigma:  # a detector's pixels; the noise-free ones keep every bit of the projection
        uv = uv.astype(np.float32).astype(np.float64)
    true = Ts.copy()  # in the caller's frame: R local + t = R Rb^T (obj - off) + t
    true[:, :3, :3] = Ts[:, :3, :3] @ Rb.T
    true[:, :3, 3] = Ts[:, :3, 3] - true[:, :3, :3] @ off
    planar, plane = pnp.plane_of(obj)
    assert planar == (kind != "cloud"), name
    return dict(name=name, kind=kind, obj=obj, uv=uv, K=K, D=D, plane=np.ascontiguousarray(plane if planar else np.eye(3)), T=true)
