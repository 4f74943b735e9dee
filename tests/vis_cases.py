"""Inputs of the picture tests (tests/test_vis_cpu.py, tests/test_gpu_vis.py) and of the fixture maker
(tests/golden/make_vis_golden.py).  Only DATA lives here: seeded depths and pictures, regenerated on both sides of a
comparison.  Shapes are the smallest at which the kernels can still go wrong: 1 x 1; 37 x 53, whose colour bar is 0 wide;
72 x 131, bar 2 wide; 131 x 257, several workgroups with ragged edges."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_vis.npz")

BARS = ("u", "d", "l", "r", "auto")
MAX_L1S = (None, 0, -1, -0.2, -0.999, 0.03)


def depth_pair(hw, seed=0, dtype=np.float64, holes=0.06, agree=True):
    """(re, gt): a smooth scene and an estimate of it with noise, a block where they agree exactly, holes in both."""
    h, w = hw
    rng = np.random.default_rng(500 + seed)
    yy, xx = np.mgrid[:h, :w]
    gt = 1.5 + 0.8 * np.sin(xx / 17.0 + seed) + 0.5 * np.cos(yy / 11.0)
    re = gt + rng.normal(0, 0.04, (h, w)) + 0.05 * np.sin(xx / 5.0)
    if agree:
        re[h // 3:h // 2, w // 4:w // 2] = gt[h // 3:h // 2, w // 4:w // 2]
    re[rng.random((h, w)) < holes] = 0
    gt[rng.random((h, w)) < holes] = 0
    return np.ascontiguousarray(re.astype(dtype)), np.ascontiguousarray(gt.astype(dtype))


def l1_cases():
    """name -> (re, gt, kwargs) that the reference itself can run (no max_l1=None with a bar, no limit of 0)."""
    c = {}
    c["p1x1"] = (np.array([[2.0]]), np.array([[1.5]]), dict(max_l1=-0.2, colorbar="auto"))
    re, gt = depth_pair((37, 53), 1)
    for bar in BARS:
        c["p37x53_fixed_" + bar] = (re, gt, dict(max_l1=0.03, colorbar=bar))
    re, gt = depth_pair((72, 131), 2)
    for bar in BARS:
        c["p72x131_top20_" + bar] = (re, gt, dict(max_l1=-0.2, colorbar=bar))  # the odd bar; it takes part in the selection
    c["p72x131_fixed_u"] = (re, gt, dict(max_l1=0.03, colorbar="u"))
    c["p72x131_gtnum"] = (re, 1.7, dict(max_l1=-0.2, colorbar="auto"))
    c["p72x131_noover"] = (re, gt, dict(max_l1=0.03, overexposed=False, colorbar="auto"))
    c["p72x131_noover_none"] = (re, gt, dict(overexposed=False, colorbar=None))
    c["p72x131_zero_r"] = (re, gt, dict(max_l1=0, colorbar="r"))
    re, gt = depth_pair((131, 257), 3)
    c["p131x257_none_nobar"] = (re, gt, dict(colorbar=None))
    c["p131x257_m1_auto"] = (re, gt, dict(max_l1=-1, colorbar="auto"))
    c["p131x257_top999_l"] = depth_pair((131, 257), 3, agree=False) + (dict(max_l1=-0.999, colorbar="l"),)  # (no |l1| of 0)
    re, gt = depth_pair((72, 131), 4, np.float32)
    c["p72x131_f32"] = (re, gt, dict(max_l1=-0.2, colorbar="d"))  # the reference is fed the widened copy
    for name, (re, gt) in selection_inputs().items():
        if name != "no_valid":
            c["sel_" + name] = (re, gt, dict(max_l1=-0.2, colorbar=None))
    return c


def selection_inputs(hw=(37, 53)):
    """name -> (re, gt) whose |l1| stress the radix select."""
    h, w = hw
    rng = np.random.default_rng(77)
    out = {}
    re, gt = depth_pair(hw, 5)
    out["quantised"] = (np.round(re * 1024) / 1024, np.round(gt * 1024) / 1024)  # many |l1| tie
    gt = np.full(hw, 1.0)
    low = rng.integers(0, 128, hw).astype(np.uint64)
    re = (np.float64(1.5).view(np.uint64) + low).view(np.float64).reshape(hw)     # |l1| = 0.5 + 2 j ulp: the lowest byte
    out["lowest_byte"] = (re, gt.copy())
    e = rng.integers(-20, 20, hw)
    l1 = np.ldexp(rng.uniform(1, 2, hw), e) * rng.choice([-1.0, 1.0], hw)         # 40 binades
    l1[rng.random(hw) < 0.1] = 0                                                   # exact zeros: re == gt
    gt = np.ldexp(1.0, 21) * np.ones(hw)
    re = gt + l1
    sub = rng.random(hw) < 0.1                                                     # subnormal errors next to tiny depths
    gt[sub] = 3e-310
    re[sub] = gt[sub] + rng.integers(1, 1000, sub.sum()) * 5e-324
    out["binades"] = (re, gt)
    out["no_valid"] = (np.zeros(hw), depth_pair(hw, 6)[1])
    few = np.zeros(hw)
    few[3, 4:8] = [1.0, 1.25, 0.5, 2.0]                                            # valid_num = 4: k = int(0.2 * 4) = 0
    out["k_zero"] = (few, np.where(few != 0, 1.1, 0.0))
    return out


def depth_image(hw, seed=0, dtype=np.float64):
    h, w = hw
    rng = np.random.default_rng(900 + seed)
    yy, xx = np.mgrid[:h, :w]
    d = 2.5 + 1.8 * np.sin(xx / 23.0 + seed) * np.cos(yy / 19.0) + rng.uniform(0, 0.05, (h, w))
    d[rng.random((h, w)) < 0.05] = 0
    d[h // 5, :] = 6.5  # beyond every fix_range used here
    if dtype == np.uint16:
        return np.ascontiguousarray((d * 1000).astype(np.uint16))
    return np.ascontiguousarray(d.astype(dtype))


def depth_cases():
    """name -> (depth, kwargs) the reference can run (ids for colour maps; no constant image under norma)."""
    c = {}
    for tag, dtype in (("f64", np.float64), ("f32", np.float32), ("u16", np.uint16)):
        d = depth_image((37, 53), 1, dtype)
        c["d37x53_%s_range5" % tag] = (d, dict(fix_range=5))
        c["d37x53_%s_pair_s10" % tag] = (d, dict(fix_range=(0.5, 4.25), slicen=10))
        c["d37x53_%s_norma" % tag] = (d, dict())
    d = depth_image((131, 257), 2)
    c["d131x257_norma_s30"] = (d, dict(slicen=30))
    c["d131x257_range_jet_s10"] = (d, dict(fix_range=4.0, slicen=10, colormap=2))
    c["d1x1"] = (np.array([[1.25]]), dict(fix_range=2.0))
    return c


def picture(hw, seed, cn):
    h, w = hw
    rng = np.random.default_rng(1300 + seed)
    yy, xx = np.mgrid[:h, :w]
    base = 120 + 60 * np.sin(xx / 6.0 + seed) * np.cos(yy / 5.0)
    img = np.clip(np.stack([base + 25 * c + rng.integers(-10, 11, (h, w)) for c in range(3)], -1), 0, 254).astype(np.uint8)
    return np.ascontiguousarray(img[..., 0] if cn == 1 else img)


def line_cases():
    """name -> (img1, img2, n_line): 40 x 60 and 61 x 40, gray and RGB mixed, a float depth as the second image."""
    c = {}
    for hw in ((40, 60), (61, 40)):
        for n_line in (1, 5, 21):
            tag = "%dx%d_n%d" % (hw + (n_line,))
            c["gray_rgb_" + tag] = (picture(hw, 1, 1), picture(hw, 2, 3), n_line)
        c["rgb_gray_%dx%d" % hw] = (picture(hw, 3, 3), picture(hw, 4, 1), 21)
        c["rgb_depth_%dx%d" % hw] = (picture(hw, 5, 3), depth_image(hw, 3), 5)
    return c


def load_fixture():
    return np.load(FIXTURE) if os.path.exists(FIXTURE) else None
