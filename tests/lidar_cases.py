"""The cases of tests/test_lidar_cpu.py and tests/test_gpu_lidar.py: seeded, small, one place (test infrastructure).
The CPU file checks that they stay within the kernels' caps and measures the round trip's reference error; the GPU file
compares the kernels with tests/lidar_ref.py on them."""
import numpy as np

GRIDS = ((24, 32), (37, 70))


# ---- 1a: 300 points ------------------------------------------------------------------------------------------------------
CLOUD_WH = (64, 48)
CLOUD_K = np.array([[50.0, 0.0, 32.0], [0.0, 50.0, 24.0], [0.0, 0.0, 1.0]])
CLOUD_K_FULL = np.array([[50.5, 0.25, 31.75], [0.125, 49.5, 24.5], [0.0, 0.0078125, 1.0]])  # all nine entries take part


def quarter_turn_T():
    """a quarter turn about z plus a dyadic shift: every product and sum of exact inputs stays exact"""
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [0.5, -0.25, 2.0]
    return T


def generic_T():
    a, b = 0.3, -0.2
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Rx, [0.11, -0.07, 0.4]
    return T


def cloud(exact=False, seed=0, n=300):
    """(n, 3) float64: points around the frustum of CLOUD_K, with z <= 0, NaN / inf rows, u exactly 0 and exactly w, v exactly
    h.  ``exact``: x, y multiples of 1/8 and z a power of two, so that the projection is exact in any order."""
    rng = np.random.default_rng(seed)
    if exact:
        z = 2.0 ** rng.integers(-1, 4, n)
        xy = rng.integers(-6, 7, (n, 2)) / 8.0 * z[:, None]
    else:
        z = rng.uniform(0.5, 9.0, n)
        xy = rng.uniform(-0.8, 0.8, (n, 2)) * z[:, None]
    P = np.concatenate([xy, z[:, None]], 1)
    P[5:25, 2] *= -1          # behind the camera
    P[30, 2] = 0.0            # p2 == 0: inf / NaN after the division
    P[31] = [0.0, 0.0, 0.0]
    P[40, 0], P[41, 1], P[42, 2] = np.nan, np.nan, np.nan
    P[43, 0], P[44, 2] = np.inf, np.inf
    P[50] = [-32.0, 0.0, 50.0]   # u == 0 exactly: kept
    P[51] = [32.0, 0.0, 50.0]    # u == w exactly: dropped
    P[52] = [0.0, 24.0, 50.0]    # v == h exactly: dropped
    P[53] = [0.0, -24.0, 50.0]   # v == 0 exactly: kept
    return P


def lost_cloud():
    """every row is lost: behind the camera, beside the image, or not finite"""
    P = cloud(seed=3, n=300)
    P[:100, 2] = -np.abs(P[:100, 2])
    P[100:200, 0] = 50.0 * np.abs(P[100:200, 2]) + 1
    P[200:] = np.nan
    return P


# ---- 1b: the hull of many samples ------------------------------------------------------------------------------------------
def hull_cases():
    """name -> (uvs (n, 2) float64, hw)"""
    rng = np.random.default_rng(11)
    out = {}
    for h, w in GRIDS:
        tag = "%dx%d" % (h, w)
        uv = rng.uniform((-6.0, -5.0), (w + 7.0, h + 4.0), (5000, 2))         # negative pixels and beyond the grid
        uv[:400] = np.floor(uv[:400]) + 0.5                                  # .5: half to even
        out["many_" + tag] = (uv, (h, w))
        disc = rng.normal((w / 2, h / 2), (w / 6, h / 6), (5000, 2))          # a round cloud: many hull vertices
        out["disc_" + tag] = (disc, (h, w))
        ys = rng.permutation(h)[: h // 2]
        out["single_" + tag] = (np.stack([rng.uniform(0, w, len(ys)), ys + rng.uniform(-0.4, 0.4, len(ys))], 1), (h, w))
        out["halves_" + tag] = (np.stack([rng.integers(0, w, 40) + 0.5, rng.integers(0, h, 40) + 0.5], 1), (h, w))
        small = rng.uniform((-3.0, -3.0), (w + 3.0, h + 3.0), (4096, 2))
        out["small_" + tag] = (small, (h, w))
    out["one_point"] = (np.array([[20.4, 17.6]]), GRIDS[0])
    out["collinear"] = (np.array([[3.0 + 7 * k, 4.0 + 2 * k] for k in range(-1, 5)] * 2), GRIDS[1])
    out["nobody"] = (np.array([[np.nan, 1.0], [2.0, np.inf], [2.0 ** 21, 3.0]]), GRIDS[0])
    out["tall"] = (tall(), (3001, 8))
    return out


def tall():
    """v over 0 .. 3000, two samples in each of the 3001 rows: 6002 candidates, more than one frame of the hull kernel"""
    rng = np.random.default_rng(12)
    v = np.repeat(np.arange(3001.0), 2) + rng.uniform(-0.3, 0.3, 6002)
    bulge = 3.5 - 3.5 * ((np.repeat(np.arange(3001.0), 2) - 1500.0) / 1500.0) ** 2  # an ellipse-like outline: many vertices
    u = 3.5 + np.tile([-1.0, 1.0], 3001) * bulge * rng.uniform(0.8, 1.0, 6002)
    return np.stack([u, v], 1)[rng.permutation(6002)]


def many_vertex_polygon(m=45):
    """(k, 2) float64, k > 4096: the corners of the convex lattice polygon whose edges are the primitive vectors (a, b) with
    |a|, |b| <= m in the order of their angle; consecutive edges differ in direction, so every corner is a strict vertex"""
    import math
    vec = [(a, b) for a in range(-m, m + 1) for b in range(-m, m + 1) if math.gcd(abs(a), abs(b)) == 1]
    vec.sort(key=lambda v: math.atan2(v[1], v[0]))
    return np.cumsum(np.array(vec, np.float64), 0)


# ---- 1c: the nearest fill inside the hull -------------------------------------------------------------------------------------
FILL_GRIDS = ((13, 8), (37, 70), (9, 257))
FILL_DISTANCES = (0.5, 2, 7)


def fill_case(hw, seed=21, n=400):
    """(n, 3) float64 samples whose hull misses the grid's first rows and its last columns; some outside the grid"""
    h, w = hw
    rng = np.random.default_rng(seed + w)
    uv = rng.uniform((-2.0, h * 0.3), (w * 0.8, h + 2.0), (n, 2))
    return np.concatenate([uv, rng.uniform(1.0, 9.0, (n, 1))], 1)


# ---- xyzs_to_dense_depth and the round trip -------------------------------------------------------------------------------------
DEPTH_WH = (162, 90)
DEPTH_K = np.array([[110.5, 0.0, 80.25], [0.0, 111.25, 44.5], [0.0, 0.0, 1.0]])
DEPTH_D = np.array([[-0.05, 0.01, 0.0005, -0.0003, 0.0]])


def lidar_pose():
    """the LiDAR's frame in the camera's: a few degrees and a few centimetres, as a rig mounts them"""
    a, b, c = np.radians([2.0, -3.0, 1.5])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, [0.06, -0.04, 0.03]
    return T


PLANE_N, PLANE_D = np.array([0.008, -0.01, 1.0]) / np.linalg.norm([0.008, -0.01, 1.0]), 6.0  # n . X = d, in the LiDAR's frame


def plane_hit(uvs, K):
    """the points of the plane under pixels ``uvs`` of a pinhole K at the LiDAR's origin"""
    rays = np.concatenate([np.asarray(uvs, np.float64), np.ones((len(uvs), 1))], 1) @ np.linalg.inv(K).T
    return rays * (PLANE_D / (rays @ PLANE_N))[:, None]


def plane_cloud(n, seed=5, dtype=np.float64):
    """a sweep over the plane, in the LiDAR's frame: rays through random pixels of a view somewhat wider than the camera's"""
    rng = np.random.default_rng(seed)
    w, h = DEPTH_WH
    uvs = rng.uniform((-12.0, -9.0), (w + 12.0, h + 9.0), (n, 2))
    return plane_hit(uvs, DEPTH_K).astype(dtype)


ANNOTATED = np.array([[20, 15], [140, 12], [81, 45], [25, 75], [135, 78], [60, 30], [100, 60], [45, 55], [120, 35]])


def annotated_pairs():
    """(uvs on the photo (float64), uvs on the depth picture (int)): the same points of the plane, seen by the camera (with
    its lens) and by the pinhole at the LiDAR's origin"""
    import pnp_ref
    X = plane_hit(ANNOTATED, DEPTH_K)
    T = lidar_pose()
    uv_img = pnp_ref.residuals(T[:3, :3], T[:3, 3], X, np.zeros((len(X), 2)), DEPTH_K, DEPTH_D.reshape(-1)).reshape(-1, 2)
    return uv_img, ANNOTATED


def pose_error(T, T_true):
    """(rotation angle in radians, |t - t_true|)"""
    dR = T[:3, :3] @ T_true[:3, :3].T
    axis = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2  # sin(angle) * the axis: fine near 0
    return float(np.arcsin(min(1.0, np.linalg.norm(axis)))), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


# What the NumPy restatement of the round trip reaches on this case (tests/test_lidar_cpu.py measures it and holds these
# figures to it): lidar_ref.xyzs_to_dense_depth (rate 0.5, the oracle's resize) -> lidar_ref.uvs_on_depth_to_xyzs ->
# pnp_ref.solve.  The GPU path may err at most twice as much.
REF_ROUNDTRIP = dict(angle=2.06592074e-06, shift=1.45255799e-05)  # radians, metres
