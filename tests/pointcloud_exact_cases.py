"""Inputs with a known exact answer for the point-cloud and z-buffer family (tests/test_pointcloud_oracle_cpu.py checks
the C oracle on them, tests/test_gpu_zbuffer_exact.py the kernels).  Only DATA lives here.  Every expected value follows
from exact arithmetic on powers of two -- no matrix product of NumPy's is involved."""
import numpy as np

XY = (320, 240)

# ---- half to even --------------------------------------------------------------------------------------------------
# X = k / 256, Y = m / 256, Z = 1 project to exactly (k + 100.5, m + 80.5): 256 * (k / 256) is exact, + c is exact.
HALF_K = np.array([[256.0, 0, 100.5], [0, 256.0, 80.5], [0, 0, 1]])
# (k, m, pixel (x, y) the point must own, or None when it must be dropped); every kept point owns a pixel of its own
HALF_CASES = [
    (0, 0, (100, 80)),        # 100.5 -> 100, 80.5 -> 80
    (1, 1, (102, 82)),        # 101.5 -> 102, 81.5 -> 82
    (2, 4, (102, 84)),        # 102.5 -> 102, 84.5 -> 84
    (-101, 10, (0, 90)),      # -0.5 -> -0.0: pixel 0, kept
    (10, -81, (110, 0)),      # the same for the row
    (-101, -81, (0, 0)),
    (218, 20, (318, 100)),    # 318.5 -> 318: the last but one column
    (219, 30, None),          # 319.5 -> 320 = w: dropped
    (30, 158, (130, 238)),    # 238.5 -> 238
    (40, 159, None),          # 239.5 -> 240 = h: dropped
    (-102, 50, None),         # -1.5 -> -2: dropped
    (50, -82, None),
]


def half_points():
    return np.array([[k / 256.0, m / 256.0, 1.0] for k, m, _ in HALF_CASES])


# ---- one pixel, many depths ----------------------------------------------------------------------------------------
# (0, 0, z) projects to exactly (100, 80) for every z != 0, negative and denormal included: xs = 100 * z, xs / z = 100
# (for the denormals 100 * z is rounded, the quotient is still within 1e-10 of 100).
CENTRE_K = np.array([[256.0, 0, 100.0], [0, 256.0, 80.0], [0, 0, 1]])
CENTRE_PIXEL = (100, 80)

# ascending: the z-buffer keeps the SMALLEST, so a negative z beats every positive one
Z_ASCENDING = [-np.nextafter(1.0, 2.0), -1.0, -1e-310, -5e-324, 5e-324, 1e-310, 1.0, np.nextafter(1.0, 2.0)]


def centre_points(zs):
    return np.array([[0.0, 0.0, z] for z in zs])


# ---- points that must be dropped -----------------------------------------------------------------------------------
# z = 0 (0 / 0 and x / 0), non-finite coordinates, and coordinates whose projection is far beyond an int
DROPPED = np.array([
    [0.0, 0.0, 0.0], [0.1, 0.1, 0.0], [-0.1, 0.1, -0.0],
    [np.inf, 0.0, 1.0], [0.0, -np.inf, 1.0], [0.0, 0.0, np.inf], [0.0, 0.0, -np.inf],
    [np.nan, 0.0, 1.0], [0.0, np.nan, 1.0], [0.0, 0.0, np.nan],
    [1e300, 0.0, 1.0], [0.0, -1e300, 1.0], [1.0, 1.0, 1e-300], [-1e300, 1e300, 1.0],
])
KEPT_AMONG_DROPPED = np.array([0.125, -0.25, 2.0])    # one ordinary point: (100 + 16, 80 - 32) = pixel (116, 48)
KEPT_PIXEL = (116, 48)


# ---- contention ----------------------------------------------------------------------------------------------------
CONTENTION_N = 65536
CONTENTION_LEVELS = 16


def contention_cloud(spread):
    """65 536 points whose z is drawn from 16 values: thousands of bit-equal ties per pixel.  ``spread`` False: all on
    CENTRE_PIXEL of an XY image; True: over the 4 x 4 image of ``SPREAD_K`` (X, Y in {0..3} / 4 * z, exact)."""
    rng = np.random.default_rng(65536)
    z = 1.0 + rng.integers(0, CONTENTION_LEVELS, CONTENTION_N) / 8.0
    if not spread:
        return np.stack([np.zeros_like(z), np.zeros_like(z), z], 1)
    cx, cy = rng.integers(0, 4, CONTENTION_N), rng.integers(0, 4, CONTENTION_N)
    return np.stack([cx * z, cy * z, z], 1)


SPREAD_K = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]])   # (c * z) / z = c exactly
SPREAD_XY = (4, 4)
