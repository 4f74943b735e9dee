"""Inputs of the point tests (tests/test_points_cpu.py, tests/test_gpu_points.py).  Only DATA lives here: cameras,
lenses and seeded point sets, regenerated from seeds on both sides of a comparison."""
import numpy as np

W, H = 640, 480
K = np.array([[410.0, 0, 322.25], [0, 407.5, 237.75], [0, 0, 1.0]])

# the issue's mild lens: project(undistort(p)) must return p
MILD = np.array([-0.1, 0.01, 1e-3, 1e-3])
# a full 12-coefficient lens (rational + thin prism); its prefixes are the shorter models
FULL12 = np.array([-0.11, 0.03, 8e-4, -6e-4, 0.004, 0.02, -0.003, 5e-4, 3e-4, -2e-4, 1e-4, 2e-4])
# 1 + k1 r^2 changes sign at r = 0.77: pixels toward the corners of the 640 x 480 image (r up to 0.98) take cv2's
# `icdist < 0` exit, the middle of the image does not
STRONG = np.array([-1.7, 0.0, 1e-3, -1e-3, 0.0])
TILTED = np.concatenate([FULL12, [0.01, -0.02]])
NDIST = (0, 4, 5, 8, 12, 14)
SIZES = (0, 1, 2, 255, 256, 257, 65537)


def lens(ndist):
    """FULL12 cut to cv2's model of ``ndist`` coefficients (14: zero tilt); None for 0."""
    if ndist == 0:
        return None
    return np.concatenate([FULL12, [0.0, 0.0]])[:ndist].copy()


def grid_pixels(step=1, dtype=np.float64):
    """Every ``step``-th pixel of the W x H image, (n, 2), row-major."""
    v, u = np.mgrid[0:H:step, 0:W:step]
    return np.stack([u.ravel(), v.ravel()], 1).astype(dtype)


def pixels(n, seed, dtype):
    """n seeded pixels inside (and a little around) the image."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n)], 1).astype(dtype)


def points3d(n, seed, dtype):
    """n seeded points in front of the camera that project near the image."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.5, 6.0, n)
    return np.stack([rng.uniform(-0.8, 0.8, n) * z, rng.uniform(-0.6, 0.6, n) * z, z], 1).astype(dtype)


def special_pixels(dtype):
    """Rows with NaN / inf among ordinary ones, the principal point, and far-away pixels."""
    return np.array([[322.25, 237.75], [0, 0], [np.nan, 10], [10, np.nan], [np.inf, 5], [5, -np.inf], [np.nan, np.nan],
                     [1e30, -1e30], [-0.0, 0.0], [639, 479], [1e5, 1e5]], dtype)


def special_points3d(dtype):
    """Z == 0 (+0 and -0), NaN / inf coordinates, points behind the camera, among ordinary ones."""
    return np.array([[0.1, -0.2, 1.0], [0.3, 0.2, 0.0], [-0.3, 0.1, -0.0], [0, 0, 0], [1, 1, -2.0], [np.nan, 0, 1],
                     [0, 0, np.nan], [np.inf, 0, 1], [1, 2, np.inf], [1e-300, 1e-300, 1e-300], [0.2, 0.1, 3.0]], dtype)


POSE = np.array([[0.9950371902, -0.0978433950, 0.0174249980, 0.11],   # a rotation by about 0.1 rad (not exactly orthonormal:
                 [0.0993346654, 0.9900332889, -0.0998334166, -0.05],  # T_to_r_t projects it onto SO(3) first, as cv2 does)
                 [-0.0074832182, 0.1010689891, 0.9948513645, 0.3],
                 [0, 0, 0, 1.0]])
