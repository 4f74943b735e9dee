"""Inputs of the sparse <-> dense tests (tests/test_sparse_cpu.py, tests/test_gpu_sparse.py) and of the fixture maker
(tests/golden/make_sparse_golden.py).  Only DATA lives here: seeded sample sets on small grids (<= 240x320), a fake
feature matcher and two constants measured on the reference's own output.  Everything is regenerated from seeds on both
sides of a comparison.

Sample sets reach beyond the grid on every side, the scatter sets put several rows on one pixel and carry exact .5
coordinates (half-to-even), values come as uint8 / float32 / float64 with 1-3 channels, and there is an empty set."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_sparse.npz")

GAP = 1e-9  # what the bit-for-bit nearest tests rest on: no tie and no threshold decision closer than this (float64
            # rounding of a distance is ~1e-15)

# How far the REFERENCE's own float64 results lie from the exact ones, measured by tests/test_sparse_cpu.py
# (test_plane_reference_error / test_triangulation_reference_error print them) on tests/golden/reference_sparse.npz, i.e.
# on what np.linalg.lstsq (LAPACK gelsd) and normal_equation (np.linalg.inv + einsum) returned in the build container
# with NumPy 2.2.6.  The yardstick is the solution of the same least-squares problem in fractions.Fraction.
#   plane: max over the pixels of |reference - exact| in float32 ulps of the exact value (0.5 = correctly rounded)
#   triangulation: max over the matches and over zs1, zs2 of |reference - exact| / |exact|
# The GPU may lie at most twice as far (the normal equations square the condition number the SVD sees), and for the
# plane never less than one ulp is allowed.
REF_PLANE_ULPS = {"plane_small": 0.497789, "plane_f64": 0.499799}
REF_TRI_RELERR = {"tri_rig": 4.34604e-13, "tri_rectified": 3.76838e-13}


def samples(seed, n, hw, dtype=np.float64, margin=3.0):
    """(n, 3) rows (u, v, z): u, v uniform over the grid and ``margin`` pixels beyond it, z a smooth field plus noise."""
    rng = np.random.default_rng(seed)
    h, w = hw
    u = rng.uniform(-margin, w + margin, n)
    v = rng.uniform(-margin, h + margin, n)
    z = 20.0 + 8.0 * np.sin(u / 11.0) * np.cos(v / 7.0) + rng.normal(0, 0.3, n)
    return np.stack([u, v, z], 1).astype(dtype)


# name -> (seed, n, (h, w), dtype, distance)
NEAREST_CASES = {
    "n700_60x80": (11, 700, (60, 80), np.float64, 2),
    "f32_120x160": (12, 1500, (120, 160), np.float32, 2),
    "d3p5_70x90": (13, 600, (70, 90), np.float64, 3.5),
    "d1_48x64": (14, 200, (48, 64), np.float64, 1),
    "dense_240x320": (15, 40000, (240, 320), np.float64, 2),
}
NEAREST_HW_NONE = "n700_60x80"   # also run with hw=None: (int(max v) + 2, int(max u) + 2)
UPSIZE_CASES = {"up8_from_30x40": ("d1_48x64", (30, 40), (240, 320)), "up_odd_from_60x80": ("n700_60x80", (60, 80), (173, 251))}


def nearest_case(name):
    seed, n, hw, dtype, distance = NEAREST_CASES[name]
    return samples(seed, n, hw, dtype), hw, distance


def scale_case():
    """1920x1080, 200 000 samples, float64, distance 2 (the downscale=1 regime of the plugin)."""
    return samples(77, 200000, (1080, 1920), np.float64, margin=4.0), (1080, 1920), 2


# ---- scatter ---------------------------------------------------------------------------------------------------------
# name -> (seed, n, (h, w), value dtype, channels, bg_value)
SCATTER_CASES = {
    "u8_c1": (21, 2500, (30, 40), np.uint8, 1, 0),
    "u8_c3": (22, 2500, (30, 40), np.uint8, 3, 7),
    "f32_c1": (23, 1800, (30, 40), np.float32, 1, -1),
    "f32_c2": (24, 1800, (30, 40), np.float32, 2, 0),
    "f64_c1": (25, 900, (36, 28), np.float64, 1, 0),
    "f64_c3": (26, 900, (36, 28), np.float64, 3, -1),
    "empty_f32": (27, 0, (10, 12), np.float32, 1, 5),
}


def scatter_case(name):
    """(uvs (n, 2) float64, values (n,) or (n, C), hw, bg_value): every fifth coordinate sits exactly on k + 0.5."""
    seed, n, hw, dtype, channels, bg = SCATTER_CASES[name]
    rng = np.random.default_rng(seed)
    h, w = hw
    uv = np.stack([rng.uniform(-2, w + 2, n), rng.uniform(-2, h + 2, n)], 1)
    half = rng.random((n, 2)) < 0.2
    uv[half] = np.floor(uv[half]) + 0.5
    shape = (n,) if channels == 1 else (n, channels)
    values = rng.integers(0, 256, shape).astype(dtype) if dtype == np.uint8 else rng.normal(0, 10, shape).astype(dtype)
    return uv, values, hw, bg


def packed_case():
    """(n, 2 + 2) float64 rows without ``values`` and ``hw=None``: the reference's (max u + 1, max v + 1) quirk."""
    uv, values, _, _ = scatter_case("f64_c3")
    uv = np.abs(uv)
    return np.concatenate([uv, values[:, :2]], 1)


def image(seed, hw, dtype):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, hw).astype(np.uint8)
    return rng.normal(0, 5, hw).astype(dtype)


# name -> (seed, (h, w), dtype, mask kind)
ARR2D_CASES = {
    "f64_all": (31, (30, 40), np.float64, None),
    "f32_all": (32, (30, 40), np.float32, None),
    "u8_all": (33, (17, 23), np.uint8, None),
    "f64_bool": (34, (30, 40), np.float64, "bool"),
    "f32_u8mask": (35, (30, 40), np.float32, "uint8"),
    "u8_floatmask": (36, (17, 23), np.uint8, "float"),
}


def arr2d_case(name):
    seed, hw, dtype, kind = ARR2D_CASES[name]
    arr = image(seed, hw, dtype)
    if kind is None:
        return arr, None
    rng = np.random.default_rng(seed + 100)
    on = rng.random(hw) < 0.3
    if kind == "bool":
        return arr, on
    if kind == "uint8":
        return arr, (on * rng.integers(1, 200, hw)).astype(np.uint8)
    m = np.where(on, rng.normal(0, 1, hw) + 3.0, 0.0)
    m[0, 0] = np.nan  # NaN is True as a boolean
    return arr, m


def sparse_image(seed=41, hw=(60, 80)):
    """A float64 image that is 0 but for one pixel in ~70 % of its 5x5 blocks (a smooth field), with a few NaN / inf thrown
    in.  The non-zero pixels sit in the top-left 2x2 of their block, so any two are at least 4 apart along one axis and no
    pixel has two of them within distance 2: on an integer lattice equal distances are the rule, and which of two
    equidistant samples SciPy's KDTree returns is unspecified."""
    rng = np.random.default_rng(seed)
    img = np.zeros(hw)
    for by in range(0, hw[0], 5):
        for bx in range(0, hw[1], 5):
            if rng.random() < 0.7:
                y, x = by + rng.integers(0, 2), bx + rng.integers(0, 2)
                img[y, x] = 5.0 + 0.03 * x - 0.02 * y + 0.2 * np.sin(x / 9.0)
    img[3, 5], img[12, 73], img[53, 2] = np.nan, np.inf, -np.inf
    return img


# ---- plane fit -------------------------------------------------------------------------------------------------------
# name -> (seed, n, (h, w)); small enough for a fractions.Fraction solve
PLANE_CASES = {"plane_small": (51, 40, (12, 16)), "plane_f64": (52, 300, (60, 80))}
PLANE_DEGENERATE = {"two_points": np.array([[3.0, 4.0, 1.5], [10.0, 2.0, 2.5]]),
                    "collinear": np.array([[1.0, 1.0, 2.0], [2.0, 2.0, 3.0], [5.0, 5.0, 7.0], [9.0, 9.0, 4.0]])}


def plane_case(name):
    seed, n, hw = PLANE_CASES[name]
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, hw[1], n), rng.uniform(0, hw[0], n)
    z = 0.031 * u - 0.017 * v + 4.2 + rng.normal(0, 0.05, n)
    return np.stack([u, v, z], 1), hw


# ---- triangulation ---------------------------------------------------------------------------------------------------
def tri_case(name, n=200):
    """(uvs1, uvs2, K1, K2, T_1to2): ``tri_rig`` = the synthetic rig's cameras and pose, matches of points 1-4 m away with
    half a pixel of noise; ``tri_rectified`` = R = I, t = (-b, 0, 0), one K, uvs2 = uvs1 - (d, 0): zs1 = b fx / d."""
    from calibrating_amd import synthetic
    rec = synthetic.rig(640, 480)
    rng = np.random.default_rng(61 if name == "tri_rig" else 62)
    K1 = np.array(rec["cam1"]["K"], np.float64)
    if name == "tri_rectified":
        K2, R, t = K1.copy(), np.eye(3), np.array([-0.12, 0.0, 0.0])
        uvs1 = np.stack([rng.uniform(80, 600, n), rng.uniform(20, 460, n)], 1)
        d = rng.uniform(15.0, 70.0, n)
        uvs2 = uvs1 - np.stack([d, np.zeros(n)], 1)
    else:
        K2, R, t = np.array(rec["cam2"]["K"], np.float64), np.array(rec["R"], np.float64), np.array(rec["t"], np.float64).reshape(3)
        X1 = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.4, 0.4, n), rng.uniform(1.0, 4.0, n)], 1)
        p1, p2 = X1 @ K1.T, (X1 @ R.T + t) @ K2.T
        uvs1 = p1[:, :2] / p1[:, 2:] + rng.normal(0, 0.5, (n, 2))
        uvs2 = p2[:, :2] / p2[:, 2:] + rng.normal(0, 0.5, (n, 2))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return uvs1, uvs2, K1, K2, T


# ---- the plugin ------------------------------------------------------------------------------------------------------
class FakeFeatureMatcher:
    """Stands in for a learned matcher: ``n`` matches drawn from a known smooth disparity field (pixels of a ``width``
    wide image), normalised to [0, 1) like the reference expects.  ``device``: hand the matches out as CUDA tensors.
    ``seen`` records the types it was called with."""

    def __init__(self, seed=71, n=1500, width=320, cfg=None, device=None):
        self.cfg = {} if cfg is None else cfg
        self.seed, self.n, self.width, self.device = seed, n, width, device
        self.seen = []

    def matches(self):
        rng = np.random.default_rng(self.seed)
        uvs1 = rng.uniform(0.0, 1.0, (self.n, 2))
        d = 12.0 + 6.0 * np.sin(3.0 * uvs1[:, 0]) * np.cos(2.0 * uvs1[:, 1])
        uvs2 = uvs1 - np.stack([d / self.width, np.zeros(self.n)], 1)
        return uvs1, uvs2

    def __call__(self, img1, img2):
        self.seen.append((type(img1), type(img2)))
        uvs1, uvs2 = self.matches()
        if self.device is not None:
            import torch
            uvs1, uvs2 = torch.from_numpy(uvs1).to(self.device), torch.from_numpy(uvs2).to(self.device)
        return dict(uvs1=uvs1, uvs2=uvs2)


# plugin __call__ alone: name -> (image (h, w), matcher kwargs)
PLUGIN_CASES = {"fm_240x320": ((240, 320), dict(seed=71, n=1500, width=320)),
                "fm_cfg_shape": ((240, 320), dict(seed=72, n=900, width=320, cfg={"shape": (200, 264)}))}
# Stereo.get_depth with the plugin: a case in the spelling of tests/golden/reference_cases.py
GET_DEPTH_CASE = dict(name="fm_get_depth", wh=(320, 240), setm=dict(max_depth=3.0), scene=((0.2, 0.1, 1.0), 1.8, 10),
                      matcher=dict(seed=73, n=2000, width=320))


def load_fixture():
    if not os.path.exists(FIXTURE):
        return None
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
