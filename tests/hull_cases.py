"""The cases of the hull fill (csrc/hull.hip; tests/test_hull_cpu.py, tests/test_gpu_hull.py, tests/test_gpu_board_depth.py)
and the reference's own distance from the exact answer on them.

Plane values follow the rule of the existing plane tests (tests/sparse_cases.py), kept as it stands: float32 ulps from
the exact least-squares plane (sparse_ref.plane_exact), and the kernel may lie at most max(1, 2 x the distance of the
reference's own formula), np.linalg.lstsq evaluated as sparse_ref.plane does.  REF_PLANE_ULPS holds that distance over the
pixels inside the hull, measured on the CPU by ``python tests/hull_cases.py`` (NumPy 2.x, LAPACK gelsd); the 1080p case is
measured on every 29th row and column, which is also where the GPU test looks.  tests/test_hull_cpu.py re-measures the
small cases and holds them to these figures.
"""
from fractions import Fraction

import numpy as np

import hull_ref
import sparse_ref

HW = (48, 64)


def _plane_z(uv, rng=None, noise=0.02):
    z = 0.013 * uv[:, 0] - 0.021 * uv[:, 1] + 2.7
    return z + (rng.normal(0, noise, len(uv)) if rng is not None else 0)


def _rows(uv, rng=None):
    uv = np.asarray(uv, np.float64)
    return np.concatenate([uv, _plane_z(uv, rng)[:, None]], 1)


def _seeded(seed, n, hw, spread=1.0):
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(0, hw[1] * spread, n), rng.uniform(0, hw[0] * spread, n)], 1)
    return _rows(uv, rng)


def lattice():
    """a fronto-parallel 11 x 8 lattice: every boundary sample is collinear with its neighbours"""
    gx, gy = np.meshgrid(10 + 4 * np.arange(11), 8 + 4 * np.arange(8))
    return _rows(np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float64), np.random.default_rng(7))


def clipped():
    return _rows([[-20.3, 10.2], [30.5, -15.5], [90.2, 20.7], [70.1, 70.4], [10.6, 60.2], [31.5, 24.5], [-5.0, 40.0]],
                 np.random.default_rng(8))


def duplicates():
    """three rows on pixel (20, 10) and two on (5, 30): with keep_last_per_pixel the last of each stays; a row outside the
    image (dropped with the flag, a hull vertex without it)"""
    uv = [[20.2, 10.1], [40.0, 12.0], [19.8, 9.7], [5.3, 30.2], [33.0, 40.0], [20.4, 10.4], [4.8, 29.9], [70.0, 20.0], [12.0, 5.0]]
    r = _rows(uv, np.random.default_rng(9))
    r[5, 2] += 0.5  # the last row of (20, 10) differs markedly, so that the fit shows which row stayed
    return r


def big_frame():
    return _seeded(11, 4096, (96, 128), 1.1) - np.array([6.0, 5.0, 0.0])


def borders_1080p():
    """88 samples whose hull touches all four borders of 1080 x 1920"""
    rng = np.random.default_rng(12)
    uv = np.stack([rng.uniform(200, 1700, 88), rng.uniform(150, 950, 88)], 1)
    uv[:4] = [[-0.4, 500.3], [1919.4, 610.2], [900.5, -0.3], [1000.2, 1079.3]]
    return _rows(uv, rng)


# name -> (rows, hw, keep_last_per_pixel): the frames with a unique plane
PLANE_FRAMES = {
    "seeded12": (_seeded(3, 12, HW), HW, False),
    "triangle": (_rows([[3, 2], [40, 5], [17, 41]]) + np.array([0.2, -0.3, 0.0]), HW, False),  # its edges cross no pixel centre
    "lattice": (lattice(), HW, False),
    "clipped": (clipped(), HW, False),
    "duplicates": (duplicates(), HW, False),
    "duplicates_keep_last": (duplicates(), HW, True),
    "big4096": (big_frame(), (96, 128), False),
    "borders1080p": (borders_1080p(), (1080, 1920), False),
}
SAMPLED = {"borders1080p": 29}  # plane ulps on every 29th row and column only
# name -> (rows, hw): no unique plane
DEGENERATE_FRAMES = {
    "one_point": (_rows([[20.4, 17.6]]), HW),
    "two_points": (_rows([[5.0, 40.0], [50.0, 7.0]]), HW),
    "horizontal": (_rows([[4, 9], [18, 9], [60, 9], [33, 9]]), HW),
    "vertical": (_rows([[31, 2], [31, 44], [31, 20]]), HW),
    "diagonal": (_rows([[2, 3], [12, 13], [40, 41], [25, 26]]), HW),
    "slope_2_7": (_rows([[3, 4], [10, 6], [24, 10], [45, 16]]), HW),
}
INVALID = np.array([[np.nan, 3.0, 1.0], [4.0, np.inf, 1.0], [5.0, 6.0, 0.0], [7.0, 8.0, np.nan], [3e6, 2.0, 1.0]])
RAGGED_COUNTS = (0, 1, 2, 3, 88)


def ragged():
    """(rows (94, 3), counts, hw): frames of 0, 1, 2, 3 and 88 rows"""
    frames = [np.zeros((0, 3)), DEGENERATE_FRAMES["one_point"][0], DEGENERATE_FRAMES["two_points"][0],
              PLANE_FRAMES["triangle"][0], lattice()]
    return np.concatenate(frames), np.array(RAGGED_COUNTS), HW, frames


def ulps_inside(img, abc, mask, step=1):
    """max over the pixels inside ``mask`` (every ``step``-th row and column) of |img - exact| in float32 ulps of the exact
    plane value -- sparse_ref.plane_ulps restricted to the hull"""
    a, b, c = abc
    worst = Fraction(0)
    for y in range(0, img.shape[0], step):
        for x in range(0, img.shape[1], step):
            if mask[y, x]:
                exact = a * x + b * y + c
                ulp = Fraction(float(np.spacing(np.float32(abs(float(exact))))))
                worst = max(worst, abs(Fraction(float(img[y, x])) - exact) / ulp)
    return float(worst)


def reference_ulps(name):
    rows, hw, keep = PLANE_FRAMES[name]
    part = rows[hull_ref.valid_rows(rows, hw, keep)]
    img, m = hull_ref.fill(rows, hw, keep)
    return ulps_inside(img, sparse_ref.plane_exact(part), m, SAMPLED.get(name, 1))


# python tests/hull_cases.py prints these
REF_PLANE_ULPS = {
    "seeded12": 0.499932,
    "triangle": 0.4976,
    "lattice": 0.499965,
    "clipped": 0.499971,
    "duplicates": 0.499987,
    "duplicates_keep_last": 0.499122,
    "big4096": 0.499977,
    "borders1080p": 0.499765,
}

# ---- the board as ground truth (tests/test_gpu_board_depth.py) ----
# With D = 0 and a known pose the board's inverse depth is affine in the pixel: 1 / z = n . K^-1 (x, y, 1) / (n . t) with n
# the board's normal in the camera.  REF_BOARD_RELERR[pose] is the largest relative error of the NumPy composition of the
# reference's lines (pixels rounded by the scatter, np.linalg.lstsq plane, float32) against that closed form inside the
# hull, for the tilted poses of tests/subpix_cases.py; the GPU is allowed twice that.  The error is the scatter's rounding
# of the pixels, not arithmetic.  (Pose 0 is fronto-parallel: its inverse depth is one constant, the composition's error
# there, 9.5e-9, is the luck of one float32 rounding and bounds nothing, so it is no case.)
REF_BOARD_RELERR = {
    1: 0.000461667,
    2: 0.000851984,
}


def board_rows(T, object_points, K):
    """(n, 3) float64 rows (u, v, z) of the board's points, farthest first: one rounding per product and sum, left to
    right -- the arithmetic of Cam._board_rows restated in NumPy"""
    o = np.asarray(object_points, np.float64)
    x, y, z = o[:, 0], o[:, 1], o[:, 2]
    cam = [T[i, 0] * x + T[i, 1] * y + T[i, 2] * z + T[i, 3] for i in range(3)]
    K = np.asarray(K, np.float64)
    p, q, s = (K[i, 0] * cam[0] + K[i, 1] * cam[1] + K[i, 2] * cam[2] for i in range(3))
    rows = np.stack([p / s, q / s, s], -1)
    return rows[np.argsort(-s, kind="stable")]


def board_composition(T, object_points, K, hw):
    """The reference's lines (camera.py:242-249) in NumPy -> (inverse-depth samples (m, 3), their plane inside the hull
    float32, mask): scatter with the last row winning, 1 / sparse, the non-zero finite pixels as rows, the plane in the hull"""
    rows = board_rows(T, object_points, K)
    sparse = sparse_ref.scatter(rows[:, :2], rows[:, 2], hw)
    with np.errstate(divide="ignore"):
        inv = 1 / sparse
    samples = sparse_ref.rows_of(inv, (inv != 0) & np.isfinite(inv))
    plane, m = hull_ref.fill(samples, hw)
    return samples, plane, m


def board_inverse_depth_exact(T, K, hw):
    """float64 (h, w): the closed form of 1 / z on the board's plane"""
    n, t = T[:3, 2], T[:3, 3]
    Kinv = np.linalg.inv(np.asarray(K, np.float64))
    ys, xs = np.mgrid[:hw[0], :hw[1]].astype(np.float64)
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ Kinv.T
    return (rays @ n) / (n @ t)


def board_reference_relerr(pose):
    import subpix_cases as sc
    T = sc.pose_T(pose)
    _, plane, m = board_composition(T, sc.object_points(), sc.K, (sc.H, sc.W))
    exact = board_inverse_depth_exact(T, sc.K, (sc.H, sc.W))
    return float((np.abs(plane.astype(np.float64) - exact) / np.abs(exact))[m != 0].max())


if __name__ == "__main__":
    print("REF_PLANE_ULPS = {")
    for k in PLANE_FRAMES:
        print('    "%s": %.6g,' % (k, reference_ulps(k)))
    print("}\nREF_BOARD_RELERR = {")
    for i in (1, 2):
        print("    %d: %.6g," % (i, board_reference_relerr(i)))
    print("}")
