"""Seeded synthetic cases of the PnP tests (tests/test_pnp_cpu.py, tests/test_gpu_pnp.py).  Only DATA lives here.

A 7 x 10 planar board (25 mm squares) and a non-planar cloud, 0.3 .. 2 m in front of a 1280 x 720 camera with fx ~ 1000,
the points spread over the image; lenses of 0, 5, 8 and 12 coefficients with the magnitudes of
``camera_model_cases.stripe_rig``; point counts on the edges of the kernel's 64-lane stride; frame counts on the edges of
its four-frame workgroup."""
import numpy as np

import camera_model_cases
import points_ref

W, H = 1280, 720
NDISTS = (0, 5, 8, 12)
POINT_COUNTS = (4, 5, 6, 63, 64, 65, 130)  # fewer points than lanes, one stride exactly, one over, more than two strides
FRAME_COUNTS = (1, 3, 4, 5)                # a partial and a full workgroup, and one frame into the next
NOISE_SIGMA = 0.3
BOARD_COLS, BOARD_ROWS, SQUARE = 10, 7, 0.025


def camera(ndist, seed=0):
    """(K, D): fx ~ 1000 at 1280 x 720; D = None for ndist 0.  The lens magnitudes are stripe_rig's, scaled by a quarter:
    at fx ~ 1000 the image corner lies at a normalised radius of 0.73, where the full magnitudes fold the image."""
    K, D = camera_model_cases.stripe_rig(W, W, ndist, seed=seed)
    rng = np.random.default_rng([7, seed, ndist])
    K = np.array([[1000.0 + rng.uniform(-20, 20), 0, W / 2 + rng.uniform(-5, 5)],
                  [0, 1000.0 + rng.uniform(-20, 20), H / 2 + rng.uniform(-5, 5)], [0, 0, 1]])
    return K, (None if D is None else D * 0.25)


def board_points(n=BOARD_COLS * BOARD_ROWS):
    """The first ``n`` corners of the board's grid (z = 0), continued row by row beyond 70 for the larger counts; the first
    four are the corners of the whole board, so that 4 .. 6 points span it."""
    cols = BOARD_COLS
    rows = max(BOARD_ROWS, -(-n // cols))
    g = np.stack(np.meshgrid(np.arange(cols), np.arange(rows)), -1).reshape(-1, 2).astype(np.float64)
    corners = np.array([[0, 0], [cols - 1, 0], [cols - 1, rows - 1], [0, rows - 1]], np.float64)
    rest = np.array([p for p in g if not (p == corners).all(1).any()])
    pts = np.concatenate([corners, rest])[:n]
    return np.concatenate([pts * SQUARE, np.zeros((len(pts), 1))], 1)


def cloud_points(n, seed=0):
    rng = np.random.default_rng([11, seed, n])
    return rng.uniform(-0.12, 0.12, (n, 3))


def poses(frames, seed=0):
    """``frames`` poses of the target: its centre 0.3 .. 2 m in front of the camera, inside the image, tilted up to ~30
    degrees.  The rotation through Rodrigues' formula in float64."""
    from calibrating_amd import geometry
    rng = np.random.default_rng([13, seed, frames])
    out = []
    for _ in range(frames):
        z = rng.uniform(0.3, 2.0)
        T = np.eye(4)
        T[:3, :3] = geometry.rodrigues(rng.uniform(-0.35, 0.35, 3))
        T[:3, 3] = [rng.uniform(-0.2, 0.2) * z, rng.uniform(-0.1, 0.1) * z, z]
        out.append(T)
    return np.stack(out)


def observe(obj, T, K, D, sigma=0.0, seed=0):
    """Raw pixels (n, 2) float64 of the object points under the pose T, with seeded Gaussian noise of ``sigma`` pixels."""
    uv = points_ref.project_points(np.asarray(obj, np.float64), T[:3, :3], T[:3, 3], K, D)
    if sigma:
        uv = uv + np.random.default_rng([17, seed, len(obj)]).normal(0, sigma, uv.shape)
    return uv


def centred(obj):
    return obj - obj.mean(0)


def case(kind, n, frames, ndist, sigma=0.0, seed=0):
    """dict(obj (n, 3) shared by all frames, uv (frames, n, 2), T (frames, 4, 4), K, D)."""
    K, D = camera(ndist, seed)
    obj = centred(board_points(n)) if kind == "board" else cloud_points(n, seed)
    Ts = poses(frames, seed + n)
    uv = np.stack([observe(obj, T, K, D, sigma, seed + 31 * i) for i, T in enumerate(Ts)])
    return dict(obj=obj, uv=uv, T=Ts, K=K, D=D, kind=kind)


def case_from_pixels(kind, n, frames, ndist, seed=0):
    """Noise-free frames whose IMAGE rows are float32: the pixels are drawn as float32 first, and the object points are
    where their rays (cv2.undistortPoints' iteration run to its fixed point, 50 rounds) meet the target under the true pose
    -- the board's plane z = 0, or depths of a cloud.  dict(obj (frames, n, 3) float64, uv (frames, n, 2) float32, T, K, D)."""
    K, D = camera(ndist, seed)
    Ts = poses(frames, seed + n + 1)
    rng = np.random.default_rng([23, seed, n, frames])
    objs, uvs = [], []
    for T in Ts:
        centre = T[:3, 3] / T[2, 3]
        uv = (np.array([K[0, 0], K[1, 1]]) * (centre[:2] + rng.uniform(-0.12, 0.12, (n, 2))) + K[:2, 2]).astype(np.float32)
        rays = np.concatenate([points_ref.undistort_trace(uv, K, D, iters=50)[0], np.ones((n, 1))], 1)
        R, t = T[:3, :3], T[:3, 3]
        if kind == "board":
            depth = (R[:, 2] @ t) / (rays @ R[:, 2])  # the object's z = R[:, 2] . (depth ray - t) = 0
        else:
            depth = T[2, 3] * rng.uniform(0.85, 1.15, n)
        obj = (depth[:, None] * rays - t) @ R
        if kind == "board":
            obj[:, 2] = 0.0
        objs.append(obj)
        uvs.append(uv)
    return dict(obj=np.stack(objs), uv=np.stack(uvs), T=Ts, K=K, D=D, kind=kind)


def perturbed(T, seed=0):
    """A start pose for the tracking use: ~3 degrees and ~2 % of the distance off the truth."""
    from calibrating_amd import geometry
    rng = np.random.default_rng([19, seed])
    T0 = np.array(T, np.float64)
    T0[:3, :3] = geometry.rodrigues(rng.uniform(-0.03, 0.03, 3)) @ T0[:3, :3]
    T0[:3, 3] *= 1 + rng.uniform(-0.02, 0.02, 3)
    return T0


# every (kind, point count, lens) the noise-free tests run; the cloud needs 6 points
GRID = [(kind, n, ndist) for kind in ("board", "cloud") for n in POINT_COUNTS for ndist in NDISTS
        if not (kind == "cloud" and n < 6)]
