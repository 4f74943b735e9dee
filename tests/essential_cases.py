"""The fixtures of the RANSAC 8-point estimator (tests/test_essential_cpu.py, tests/test_gpu_essential.py): matches of the
rotated-and-translated 720p rig of tests/epipolar_cases.py, contaminated with uniformly random wrong pairs.  Only DATA
lives here; everything is regenerated from seeds, and the restatement's answer is computed once per case."""
import functools

import numpy as np

import epipolar_cases as ec
import essential_ref as er

RIG = ec.POSE_CASES["scene_720p_noise"]  # r = (0.02, -0.11, 0.03), t = (-0.30, 0.02, 0.04), 0.3 px noise
THRESHOLD = 1.0   # pixels: the default of find_essential_matrix
MASK_LIMIT = 0.02  # the share of rows on which the returned mask may differ from the true matrix' mask


@functools.lru_cache(maxsize=None)
def scene(n=1000, noise=0.3, wrong=0.0, seed=4101):
    """dict(uvs1, uvs2 (n, 2) float64, K1, K2, xy1, xy2, R, t, X1, wrong (n,) bool): n matches of the rig; the share
    ``wrong`` of them (chosen by the seed) has its pixel in image 2 replaced by a uniformly random one."""
    K1, K2 = ec._K(*RIG["wh1"], RIG["f1"], 3.1, -2.2), ec._K(*RIG["wh2"], RIG["f2"], -4.3, 1.7)
    R, t = ec._rodrigues(RIG["r"]), np.array(RIG["t"], np.float64)
    uvs1, uvs2, X1 = ec._scene(seed, K1, K2, RIG["wh1"], RIG["wh2"], R, t, 2 * n + 64, noise)
    assert len(uvs1) >= n
    uvs1, uvs2, X1 = uvs1[:n].copy(), uvs2[:n].copy(), X1[:n].copy()
    rng = np.random.default_rng(seed + 1)
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[: int(round(wrong * n))]] = True
    uvs2[bad] = np.stack([rng.uniform(0, RIG["wh2"][0], int(bad.sum())), rng.uniform(0, RIG["wh2"][1], int(bad.sum()))], 1)
    return dict(uvs1=uvs1, uvs2=uvs2, K1=K1, K2=K2, xy1=RIG["wh1"], xy2=RIG["wh2"], R=R, t=t, X1=X1, wrong=bad, n=n)


# the three end-to-end scenes: name -> scene arguments
END_TO_END = {"wrong_30": dict(n=1000, noise=0.3, wrong=0.3), "clean": dict(n=1000, noise=0.3, wrong=0.0),
              "eight_exact": dict(n=8, noise=0.0, wrong=0.0)}


def end_to_end(name):
    return scene(**END_TO_END[name])


# stage cases: (matches, hypotheses, dtype).  n crosses the wave (64), the workgroup (256) and the four-rows-a-lane pass
# (1024 is not crossed by 1000: the last rows of the pass are absent); hypotheses cross stage 1's 64 a workgroup
STAGE_CASES = [(8, 4, "float64"), (9, 5, "float64"), (63, 63, "float32"), (64, 64, "float64"), (65, 65, "float64"),
               (256, 1, "float32"), (257, 5, "float64"), (1000, 1024, "float64"), (1000, 65, "float32")]
STAGE_SEED = 7


def stage_inputs(n, dtype):
    """matches of the contaminated scene (20 % wrong where there are enough to leave 8 good ones) in ``dtype``"""
    s = scene(n=n, noise=0.3, wrong=0.2 if n >= 63 else 0.0, seed=4200 + n)
    return s["uvs1"].astype(dtype), s["uvs2"].astype(dtype), s["K1"], s["K2"]


@functools.lru_cache(maxsize=None)
def stage_reference(n, hypotheses, dtype):
    """the restatement's whole answer for a stage case (computed once, shared, never written to)"""
    uvs1, uvs2, K1, K2 = stage_inputs(n, dtype)
    return er.find(uvs1, uvs2, K1, K2, THRESHOLD, hypotheses, STAGE_SEED)


def degenerate_inputs():
    """eight copies of one match"""
    s = scene(n=8, noise=0.0)
    return np.repeat(s["uvs1"][:1], 8, 0), np.repeat(s["uvs2"][:1], 8, 0), s["K1"], s["K2"]


def true_mask(s, threshold=THRESHOLD):
    """the inliers of the scene's TRUE essential matrix at the threshold"""
    thr2 = er.ray_threshold2(s["K1"], s["K2"], threshold)
    return er.inliers(er.true_E(s["R"], s["t"]).reshape(9), er.rays(s["uvs1"], s["K1"]), er.rays(s["uvs2"], s["K2"]), thr2)
