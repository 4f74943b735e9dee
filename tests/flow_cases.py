"""Inputs of the warp_flow tests (tests/test_flow_cpu.py, tests/test_gpu_flow.py) and of the fixture maker
(tests/golden/make_flow_golden.py).  Only DATA lives here: seeded flows and pictures, regenerated on both sides of a
comparison.  Flows are normalised (2, h, w): x in units of w, y in units of h."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_flow.npz")

H, W = 64, 96
INTER_NEAREST, INTER_LINEAR, INTER_LANCZOS4 = 0, 1, 4


def image(seed, hw=(H, W), cn=3):
    """A uint8 picture with structure at every scale (so that interpolation weights matter) -- (h, w) or (h, w, 3)."""
    rng = np.random.default_rng(2000 + seed)
    h, w = hw
    yy, xx = np.mgrid[:h, :w]
    base = 120 + 70 * np.sin(xx / 9.0 + seed) * np.cos(yy / 7.0) + 30 * ((xx // 16 + yy // 12) % 2)
    img = np.stack([base + 20 * c + rng.integers(-12, 13, (h, w)) for c in range(max(cn, 1))], -1)
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img[..., 0] if cn == 1 else np.ascontiguousarray(img)


def _normal(px_x, px_y, dtype, hw):
    h, w = hw
    return np.ascontiguousarray(np.stack([px_x / w, px_y / h]).astype(dtype))


def smooth_flow(dtype, hw=(H, W), seed=0):
    """A few pixels of smooth motion; along the borders some targets leave the image."""
    h, w = hw
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    px_x = 3.7 * np.sin(yy / 11.0 + seed) + 2.3 * np.cos(xx / 7.0) + 1.1
    px_y = 2.9 * np.cos(xx / 13.0 + seed) - 1.7 * np.sin(yy / 5.0) - 0.6
    return _normal(px_x, px_y, dtype, hw)


def contracting_flow(dtype, hw=(H, W)):
    """Every pixel moves half-way to the centre: about four sources per hit target."""
    h, w = hw
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    return _normal(-0.5 * (xx - (w - 1) / 2.0) + 0.2, -0.5 * (yy - (h - 1) / 2.0) - 0.3, dtype, hw)


def zero_blocks_flow(dtype, hw=(H, W), seed=1):
    """Random motion of a few pixels with a block of exact zeros and a block of -0.0 (neither takes part), plus rows
    where only one component is zero (those do)."""
    h, w = hw
    rng = np.random.default_rng(seed)
    f = _normal(rng.uniform(-4, 4, (h, w)), rng.uniform(-4, 4, (h, w)), dtype, hw)
    f[:, 5:20, 10:40] = 0.0
    f[:, 30:45, 50:80] = -0.0
    f[0, 50:55, :] = 0.0
    f[1, 58:62, :] = -0.0
    return f


def outside_flow(dtype, hw=(H, W), seed=2):
    """A shift of (+20, -15) pixels with noise: a third of the targets fall outside the image."""
    h, w = hw
    rng = np.random.default_rng(seed)
    return _normal(20 + rng.uniform(-2, 2, (h, w)), -15 + rng.uniform(-2, 2, (h, w)), dtype, hw)


def half_flow(hw=(H, W), seed=3):
    """float64 flow whose targets land exactly on .5 or on integers: flow_x = j / 64 with w = 96 gives 1.5 j pixels,
    flow_y = j / 128 with h = 64 gives j / 2 pixels, all exact in float64 -- np.round's half-to-even decides."""
    h, w = hw
    assert (h, w) == (64, 96)
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([rng.integers(-3, 4, (h, w)) / 64.0, rng.integers(-7, 8, (h, w)) / 128.0]))


BIG, SMALL, DOUBLE = (80, 120), (40, 60), (128, 192)

# name -> (flow, image, interpolation); the image is img2 for "b_*" (backward) and img1 for "f_*" (forward)
def backward_cases():
    return {
        "b_gray_f32_linear": (smooth_flow(np.float32), image(1, cn=1), INTER_LINEAR),
        "b_rgb_f64_linear": (smooth_flow(np.float64, seed=1), image(2, cn=3), INTER_LINEAR),
        "b_rgb_f32_nearest": (smooth_flow(np.float32, seed=2), image(3, cn=3), INTER_NEAREST),
        "b_gray_f64_nearest": (smooth_flow(np.float64, seed=3), image(4, cn=1), INTER_NEAREST),
        "b_rgb_f32_linear_resize": (smooth_flow(np.float32), image(5, DOUBLE, cn=3), INTER_LINEAR),
        "b_gray_f64_nearest_resize": (smooth_flow(np.float64), image(6, DOUBLE, cn=1), INTER_NEAREST),
    }


def forward_inputs():
    """name -> (flow, img1); every forward case is run with INTER_LINEAR and with INTER_NEAREST."""
    return {
        "f_contract": (contracting_flow(np.float32), image(7, cn=1)),
        "f_zero_blocks": (zero_blocks_flow(np.float64), image(8, cn=3)),
        "f_outside": (outside_flow(np.float32), image(9, cn=3)),
        "f_half": (half_flow(), image(10, cn=1)),
        "f_big_img1": (smooth_flow(np.float32, seed=4), image(11, BIG, cn=3)),
        "f_small_img1": (contracting_flow(np.float64), image(12, SMALL, cn=1)),
    }


FORWARD_INTERPOLATIONS = (("linear", INTER_LINEAR), ("nearest", INTER_NEAREST))


def load_fixture():
    return np.load(FIXTURE) if os.path.exists(FIXTURE) else None
