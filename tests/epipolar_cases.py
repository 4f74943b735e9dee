"""Inputs of the epipolar tests (tests/test_epipolar_cpu.py, tests/test_gpu_epipolar.py) and of the fixture maker
(tests/golden/make_epipolar_golden.py).  Only DATA lives here: seeded scenes, point sets, flows and masks; everything
is regenerated from seeds on both sides of a comparison, and the fixture carries the SHA-256 of every input."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_epipolar.npz")
SENS_RUNS = 16        # reruns of the reference with every input coordinate moved by one ulp
SENS_FACTOR = 4       # margin for estimating a maximum from SENS_RUNS samples
R_ULP = 2.0 ** -24    # floor of the rotation's allowance: its entries are float32-rounded, so sens_R is 0 until an entry sits
                      # on a rounding tie, where another CPU / BLAS moves it by one float32 ulp (2^-24 below 1)
ZS_SAMPLE = 200       # matches per pose case solved exactly in fractions.Fraction
MEAN_FLOOR = 1e-6     # generator condition: no candidate mean closer to 0 than this fraction of the case's largest
IDX_STEP = 64         # long index vectors are stored as SHA-256 + every IDX_STEP-th entry


def _rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _K(w, h, f, dx=0.0, dy=0.0):
    return np.array([[f * w, 0, w / 2 + dx], [0, f * w * 1.01, h / 2 + dy], [0, 0, 1.0]])


# name -> scene parameters.  r, t: the pose X2 = R X1 + t; n: scene points drawn (the matches are those both cameras see)
POSE_CASES = {
    "scene_720p_clean": dict(seed=101, wh1=(1280, 720), wh2=(1280, 720), f1=0.80, f2=0.74, r=(0.02, -0.11, 0.03),
                             t=(-0.30, 0.02, 0.04), n=21000, noise=0.0, baseline=0.3),
    "scene_720p_noise": dict(seed=102, wh1=(1280, 720), wh2=(1280, 720), f1=0.80, f2=0.74, r=(0.02, -0.11, 0.03),
                             t=(-0.30, 0.02, 0.04), n=21000, noise=0.3, baseline=0.3),
    "small_n60": dict(seed=103, wh1=(640, 480), wh2=(640, 480), f1=0.9, f2=0.85, r=(-0.03, 0.08, 0.01), t=(0.2, -0.03, 0.02),
                      n=66, noise=0.0, baseline=1),
    "mid_n150": dict(seed=104, wh1=(640, 480), wh2=(800, 600), f1=0.9, f2=0.8, r=(0.01, 0.06, -0.02), t=(0.25, 0.01, -0.03),
                     n=170, noise=0.05, baseline=2.5),
    "later_winner": dict(seed=105, wh1=(640, 480), wh2=(640, 480), f1=0.9, f2=0.85, r=(0.04, 0.09, -0.02), t=(0.05, 0.22, 0.03),
                         n=900, noise=0.1, baseline=1),
    "same_K": dict(seed=106, wh1=(640, 480), wh2=(640, 480), f1=0.85, f2=None, r=(0.0, -0.07, 0.015), t=(-0.15, 0.0, 0.01),
                   n=3000, noise=0.1, baseline=0.15),
}
# EssentialMatrixStereo.from_stereo on a rig record that carries distortion (the matches are of the undistorted pixels)
FROM_STEREO_CASE = "from_stereo_distorted"
FROM_STEREO = dict(seed=107, wh1=(448, 336), wh2=(560, 420), n=4000, noise=0.1)
LATER_WINNER_SEEDS = range(105, 140)  # the generator takes the first seed whose winner is not candidate 0 and stores it


def from_stereo_record():
    (w1, h1), (w2, h2) = FROM_STEREO["wh1"], FROM_STEREO["wh2"]
    return dict(R=_rodrigues([0.012, -0.018, 0.006]).tolist(), t=[[-0.12], [0.002], [-0.001]],
                cam1=dict(fx=0.8 * w1, fy=0.81 * w1, cx=w1 / 2 + 3.3, cy=h1 / 2 - 2.1, D=[[-0.12, 0.05, 1e-3, -5e-4, 0.01]],
                          xy=[w1, h1], name="wide"),
                cam2=dict(fx=0.78 * w2, fy=0.79 * w2, cx=w2 / 2 - 5.2, cy=h2 / 2 + 4.4, D=[[0.08, -0.03, -8e-4, 6e-4, 0.002]],
                          xy=[w2, h2], name="fine"))


def _scene(seed, K1, K2, wh1, wh2, R, t, n, noise, zrange=(1.5, 6.0)):
    """Scene points in camera 1's frame seen by both cameras, and their pixels (plus seeded Gaussian noise)."""
    rng = np.random.default_rng(seed)
    px = np.stack([rng.uniform(0, wh1[0], n), rng.uniform(0, wh1[1], n), np.ones(n)], 1)
    X1 = (px @ np.linalg.inv(K1).T) * rng.uniform(*zrange, n)[:, None]
    X2 = X1 @ R.T + t
    p1, p2 = X1 @ K1.T, X2 @ K2.T
    uvs1, uvs2 = p1[:, :2] / p1[:, 2:], p2[:, :2] / p2[:, 2:]
    seen = (X2[:, 2] > 0.2) & (uvs2[:, 0] >= 0) & (uvs2[:, 0] < wh2[0]) & (uvs2[:, 1] >= 0) & (uvs2[:, 1] < wh2[1])
    uvs1, uvs2, X1 = uvs1[seen], uvs2[seen], X1[seen]
    if noise:
        uvs1 = uvs1 + rng.normal(0, noise, uvs1.shape)
        uvs2 = uvs2 + rng.normal(0, noise, uvs2.shape)
    return np.ascontiguousarray(uvs1), np.ascontiguousarray(uvs2), X1


def pose_case(name, seed=None):
    """dict(uvs1, uvs2, K1, K2 (None = K1), xy1, xy2, baseline, X1, R, t, noise)."""
    if name == FROM_STEREO_CASE:
        rec, c = from_stereo_record(), FROM_STEREO
        Ks = [np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1.0]]) for cam in (rec["cam1"], rec["cam2"])]
        R, t = np.array(rec["R"]), np.array(rec["t"]).reshape(3)
        uvs1, uvs2, X1 = _scene(c["seed"], Ks[0], Ks[1], c["wh1"], c["wh2"], R, t, c["n"], c["noise"])
        return dict(uvs1=uvs1, uvs2=uvs2, K1=Ks[0], K2=Ks[1], xy1=c["wh1"], xy2=c["wh2"], baseline=None, X1=X1, R=R, t=t,
                    noise=c["noise"], record=rec)
    c = POSE_CASES[name]
    K1 = _K(*c["wh1"], c["f1"], 3.1, -2.2)
    K2 = K1 if c["f2"] is None else _K(*c["wh2"], c["f2"], -4.3, 1.7)
    R, t = _rodrigues(c["r"]), np.array(c["t"], np.float64)
    uvs1, uvs2, X1 = _scene(c["seed"] if seed is None else seed, K1, K2, c["wh1"], c["wh2"], R, t, c["n"], c["noise"])
    return dict(uvs1=uvs1, uvs2=uvs2, K1=K1, K2=None if c["f2"] is None else K2, xy1=c["wh1"], xy2=c["wh2"],
                baseline=c["baseline"], X1=X1, R=R, t=t, noise=c["noise"])


ALL_POSE_CASES = list(POSE_CASES) + [FROM_STEREO_CASE]


def nudged(a, rng):
    """Every entry moved by one ulp in a seeded random direction."""
    return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))


def zs_sample(n, seed=7):
    return np.sort(np.random.default_rng(seed).choice(n, min(n, ZS_SAMPLE), replace=False))


# ---- three cameras: two rigs that share camera "a" ---------------------------------------------------------------------
def trio_case():
    """Rig A = cameras (a, b) at its true baseline, rig B = (a, c) to be brought to A's scale.  The same scene points (at most one per pixel
    of camera a), B sees a permuted subset; no noise.  -> dict(A=..., B=..., true_ratio = |t_B| / |t_A|, theta_min)."""
    wh = (960, 720)
    Ka, Kb, Kc = _K(*wh, 0.85, 2.0, -1.0), _K(*wh, 0.8, -3.0, 2.0), _K(*wh, 0.9, 1.0, 4.0)
    Rb, tb = _rodrigues((0.01, -0.08, 0.02)), np.array([-0.25, 0.01, 0.02])
    Rc, tc = _rodrigues((-0.05, 0.03, 0.01)), np.array([0.03, 0.31, -0.02])
    rng = np.random.default_rng(201)
    gy, gx = np.mgrid[4:wh[1]:8, 4:wh[0]:8]  # one point per 8 x 8 pixels, jittered: no two share a cell of camera a
    n = gx.size
    px = np.stack([gx.ravel() + rng.uniform(-3, 3, n), gy.ravel() + rng.uniform(-3, 3, n), np.ones(n)], 1)
    X = (px @ np.linalg.inv(Ka).T) * rng.uniform(2.0, 5.0, n)[:, None]

    def see(K, R, t):
        p = (X @ R.T + t) @ K.T
        uv = p[:, :2] / p[:, 2:]
        return uv, (uv[:, 0] >= 0) & (uv[:, 0] < wh[0]) & (uv[:, 1] >= 0) & (uv[:, 1] < wh[1])

    ua = (X @ Ka.T)[:, :2] / X[:, 2:]
    ub, okb = see(Kb, Rb, tb)
    uc, okc = see(Kc, Rc, tc)
    ia = np.flatnonzero(okb)
    ic = rng.permutation(np.flatnonzero(okc))[: int(okc.sum() * 0.8)]
    A = dict(uvs1=np.ascontiguousarray(ua[ia]), uvs2=np.ascontiguousarray(ub[ia]), K1=Ka, K2=Kb, xy1=wh, xy2=wh,
             baseline=float(np.linalg.norm(tb)), name1="a", name2="b")
    B = dict(uvs1=np.ascontiguousarray(ua[ic]), uvs2=np.ascontiguousarray(uc[ic]), K1=Ka, K2=Kc, xy1=wh, xy2=wh, baseline=1,
             name1="a", name2="c")
    return dict(A=A, B=B, true_ratio=float(np.linalg.norm(tc) / np.linalg.norm(tb)),
                theta_min=float(min(np.linalg.norm(tb), np.linalg.norm(tc)) / 5.0 / 1.2))


# ---- matching ----------------------------------------------------------------------------------------------------------
# name -> (builder, MAX_DISTANCE, MIN_MATCHED_PIXELS)
def _uniform_sets(seed, n, wh, dtype=np.float64):
    rng = np.random.default_rng(seed)
    uvs1 = np.stack([rng.uniform(0, wh[0], n), rng.uniform(0, wh[1], n)], 1)
    third = uvs1[rng.permutation(n)[: n // 3]] + rng.normal(0, 0.2, (n // 3, 2))
    other = np.stack([rng.uniform(0, wh[0], n // 6), rng.uniform(0, wh[1], n // 6)], 1)
    uvs2 = np.concatenate([third, other])[rng.permutation(n // 3 + n // 6)]
    return uvs1.astype(dtype), np.ascontiguousarray(uvs2.astype(dtype))


def _half_and_negative(seed=302, n=6000):
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-40, 60, (n, 2)), rng.uniform(-40, 60, (n, 2))
    for s in (a, b):
        half = rng.random(s.shape) < 0.4
        s[half] = np.floor(s[half]) + 0.5
    return a, b


def _duplicates(seed=303, n=20000):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 50, (n, 2)), rng.uniform(-5, 45, (n // 2, 2))


def _too_few(seed=304):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 100, (5, 2)), rng.uniform(0, 100, (5, 2))


MATCH_CASES = {
    "uniform_300k_d1": (lambda: _uniform_sets(301, 300000, (1280, 720)), 1, 10),
    "uniform_300k_d0p5": (lambda: _uniform_sets(301, 300000, (1280, 720)), 0.5, 10),
    "uniform_300k_d3": (lambda: _uniform_sets(301, 300000, (1280, 720)), 3, 10),
    "half_and_negative": (_half_and_negative, 1, 10),
    "half_and_negative_d0p5": (_half_and_negative, 0.5, 10),
    "duplicates": (_duplicates, 1, 10),
    "too_few": (_too_few, 1, 10),
    "float32_100k": (lambda: _uniform_sets(305, 100000, (1280, 720), np.float32), 1, 10),
    "float32_100k_d0p3": (lambda: _uniform_sets(305, 100000, (1280, 720), np.float32), 0.3, 10),
}


def match_case(name):
    build, d, k = MATCH_CASES[name]
    uvs1, uvs2 = build()
    return uvs1, uvs2, d, k


def match_scale_case():
    """1920x1080, 2 000 000 points per set."""
    rng = np.random.default_rng(399)
    n = 2000000
    uvs1 = np.stack([rng.uniform(0, 1920, n), rng.uniform(0, 1080, n)], 1)
    uvs2 = uvs1[rng.permutation(n)] + rng.normal(0, 0.3, (n, 2))
    return uvs1, np.ascontiguousarray(uvs2)


# ---- overlap filter ----------------------------------------------------------------------------------------------------
def overlap_case(name):
    if name in ("reversed", "reversed_f32"):
        uvs1 = _uniform_sets(401, 300000, (1280, 720))[0]
        uvs1 = uvs1.astype(np.float32) if name.endswith("f32") else uvs1
        return uvs1, np.ascontiguousarray(uvs1[::-1])
    if name == "no_overlap":
        ys, xs = np.mgrid[:60, :80]
        rng = np.random.default_rng(402)
        g = np.stack([xs.ravel(), ys.ravel()], 1) + rng.uniform(-0.3, 0.3, (4800, 2))
        return g[rng.permutation(4800)], g - 7.0
    rng = np.random.default_rng(403)  # every_point_overlaps
    g = rng.uniform(-10, 30, (500, 2)).astype(np.float32)
    return np.concatenate([g, g]), np.concatenate([g + np.float32(100), g + np.float32(200)])


OVERLAP_CASES = ("reversed", "reversed_f32", "no_overlap", "every_point_overlaps")


# ---- flow ------------------------------------------------------------------------------------------------------------
def flow_abs(seed, hw):
    rng = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[:h, :w]
    f = np.stack([9.0 * np.sin(yy / 41.0) + 0.01 * xx, 5.0 * np.cos(xx / 29.0) - 0.02 * yy], 2) + rng.normal(0, 0.3, (h, w, 2))
    return f.astype(np.float32)


def flow_mask(seed, hw, density):
    if density in (0, 1):
        return np.full(hw, bool(density))
    return np.random.default_rng(seed).random(hw) < density


# name -> (flow seed, (h, w), mask density)
FLOW_CASES = {"vga_empty": (501, (480, 640), 0), "vga_third": (502, (480, 640), 0.3), "vga_full": (503, (480, 640), 1),
              "k1_empty": (504, (1024, 1024), 0), "k1_third": (505, (1024, 1024), 0.3), "k1_full": (506, (1024, 1024), 1)}


def flow_case(name):
    seed, hw, density = FLOW_CASES[name]
    return flow_abs(seed, hw), flow_mask(seed + 50, hw, density)


def flow_scale_case():
    return flow_abs(599, (1080, 1920)), np.ones((1080, 1920), bool)


def flowds_case(name):
    """(viewds, flowds): ``two_way`` = views 0 <-> 1 with flow_abs one way and flow_normal (view mask of another size)
    the other, plus 1 -> 2 alone whose mask has 10 pixels (skipped: the pair vanishes) and 0 -> 2 one way;
    ``normal_no_view_mask`` = a flow_normal whose target view has no mask."""
    hw = (120, 160)
    few = np.zeros(hw, bool)
    few[5, 3:13] = True
    if name == "two_way":
        viewds = {0: dict(mask=np.ones((240, 320), bool)), 1: dict(mask=np.ones(hw, bool)), 2: {}}
        n10 = flow_abs(611, hw).transpose(2, 0, 1) / np.float32(150.0)
        flowds = {(0, 1): dict(flow_abs=flow_abs(610, hw), common_fov_mask=flow_mask(620, hw, 0.4)),
                  (1, 0): dict(flow_normal=np.ascontiguousarray(n10.astype(np.float32)), common_fov_mask=flow_mask(621, hw, 0.25)),
                  (1, 2): dict(flow_abs=flow_abs(612, hw), common_fov_mask=few),
                  (2, 0): dict(flow_abs=flow_abs(613, hw), common_fov_mask=flow_mask(623, hw, 0.1))}
        return viewds, flowds
    viewds = {0: {}, 1: {}}
    n01 = flow_abs(614, hw).transpose(2, 0, 1) / np.float32(150.0)
    return viewds, {(0, 1): dict(flow_normal=np.ascontiguousarray(n01.astype(np.float32)), common_fov_mask=flow_mask(624, hw, 0.3))}


FLOWDS_CASES = ("two_way", "normal_no_view_mask")
CONVERT_CASES = {"vga": (701, (480, 640), None), "odd_to_other": (702, (37, 53), (111, 75))}  # name -> (seed, hw, target hw)


def load_fixture():
    if not os.path.exists(FIXTURE):
        return None
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
