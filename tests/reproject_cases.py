"""Inputs of the re-projection tests (tests/test_reproject_cpu.py, tests/test_gpu_reproject.py) and of the fixture maker
(tests/golden/make_reproject_golden.py).  Only DATA lives here: the rig of tests/test_gpu_pointcloud.py::
test_project_cam2_depth (K1 420/424, K2 380, 300x220 -> 320x240), its depth scene, deterministic images and a coloured
cloud.  Everything is regenerated from seeds on both sides of a comparison."""
import os

import numpy as np

from calibrating_amd import geometry

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_reproject.npz")

K1 = np.array([[420.0, 0, 161.3], [0, 424.0, 118.9], [0, 0, 1]])
XY1 = (320, 240)
K2 = np.array([[380.0, 0, 150.0], [0, 380.0, 110.0], [0, 0, 1]])
XY2 = (300, 220)
RATE_NATIVE = 420 / 380 * 1.5     # what get_appropriate_interpolation_rate gives this rig at interpolation=1.5
PRECONDITION_RATES = (1, 1.5, RATE_NATIVE)
GPU_RATES = (1, 1.5, 0.75)
GOLDEN_RATES = (1, 1.5)           # the two rates the reference itself was run at (tests/golden/reference_reproject.npz)
CAP = 0.9999                      # share of pixels that must be bit-equal with a NUMPY restatement, and only with one:
                                  # its matrix products are NumPy's BLAS, whose rounding belongs to the machine.  The
                                  # kernels are held to the exact C oracle (oracle/pointcloud_ref.c) on every pixel.


def scene_depth(seed, h, w, holes=0.2):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    z = 1.5 + 0.5 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 0.3 * (xx > w // 2)
    z[rng.random((h, w)) < holes] = 0
    return z


def depth2(seed=3, xy=XY2):
    return scene_depth(seed, xy[1], xy[0])


def pose(rotated=True):
    """T_2in1: the rotated pose of test_project_cam2_depth, or the same translation with R = I."""
    T = np.eye(4)
    if rotated:
        T[:3, :3] = geometry.rodrigues(np.array([0.01, 0.03, -0.02]))
    T[:3, 3] = [-0.05, 0.0, 0.01]
    return T


def image(seed, xy=XY2, cn=3):
    """A uint8 picture with structure at every scale (so that bilinear weights matter) -- (h, w) or (h, w, 3)."""
    rng = np.random.default_rng(1000 + seed)
    w, h = xy
    yy, xx = np.mgrid[:h, :w]
    base = 120 + 70 * np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0) + 30 * ((xx // 16 + yy // 12) % 2)
    img = np.stack([base + 20 * c + rng.integers(-12, 13, (h, w)) for c in range(max(cn, 1))], -1)
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img[..., 0] if cn == 1 else np.ascontiguousarray(img[..., :cn])


def coloured_cloud(seed=5):
    """(points (N, 3) in camera 1's frame, values uint8 (N, 3)): camera 2's depth and picture as a coloured cloud moved
    into camera 1 -- ``values = img[mask]``."""
    from oracle import pointcloud_ref
    d = depth2(seed)
    img = image(seed)
    cloud = pointcloud_ref.apply_T_to_point_cloud(pose(), pointcloud_ref.depth_to_point_cloud(d, K2))
    return cloud, img[d != 0]


def load_fixture():
    return np.load(FIXTURE) if os.path.exists(FIXTURE) else None
