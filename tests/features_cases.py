"""The fixtures of the feature matcher (tests/features_ref.py, csrc/features.hip): scenes rendered by analytic ray casting,
so the true correspondence of every pixel is known.  A random-block texture lies on two planes that meet at an edge (a
single plane would make the 8-point fit degenerate): the surface Z = Z0 + SLOPE |X| in camera 1's frame, textured by its
arc length across the edge and by Y.  The texture is a hashed integer per 9 x 9 block of texels, a texel about a pixel
wide; every pixel is the mean of 3 x 3 rays, plus seeded Gaussian noise of sigma 2.  Only DATA lives here; everything is
regenerated from seeds and computed once."""
import functools

import numpy as np

import epipolar_cases as ec

W, H = 320, 240
F = 0.9 * W                      # focal length in pixels
K = np.array([[F, 0, W / 2 - 0.5], [0, F, H / 2 - 0.5], [0, 0, 1.0]])
Z0, SLOPE = 2.6, 0.55            # the edge lies at X = 0, Z = Z0; both planes recede from it
TEXEL = Z0 / F                   # metres: a texel is about a pixel at the edge
BLOCK = 9
R_POSE, T_POSE = (0.03, -0.06, 0.02), (-0.22, 0.015, 0.02)  # X2 = R X1 + t: a few degrees and a baseline apart
T_RECT = (-0.12, 0.0, 0.0)       # the rectified pair: R = I, so disparity = F * 0.12 / Z
SEED = 20


def _hash(bu, bv, seed):
    """a hashed byte per block (plain integer mixing in uint64, wrapping)"""
    z = (bu.astype(np.int64) * 73856093 ^ bv.astype(np.int64) * 19349663 ^ (seed * 83492791)).astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return ((z ^ (z >> np.uint64(31))) & np.uint64(255)).astype(np.float64)


def cast(uv, R, t):
    """The scene points X (n, 3), in camera 1's frame, that the pixels uv (n, 2) of the camera X_cam = R X + t see."""
    uv = np.asarray(uv, np.float64)
    d = np.concatenate([uv, np.ones((len(uv), 1))], 1) @ np.linalg.inv(K).T @ R  # directions in camera 1's frame (R^T d)
    c = -R.T @ np.asarray(t, np.float64)                                         # the camera's centre
    best = np.full(len(uv), np.inf)
    for sign in (-1.0, 1.0):  # the plane Z = Z0 + sign * SLOPE * X, valid where sign * X >= 0
        den = d[:, 2] - sign * SLOPE * d[:, 0]
        s = (Z0 + sign * SLOPE * c[0] - c[2]) / den
        ok = (s > 0) & (sign * (c[0] + s * d[:, 0]) >= 0)
        best = np.where(ok & (s < best), s, best)
    return c + best[:, None] * d


def project(X, R, t):
    p = (X @ R.T + np.asarray(t, np.float64)) @ K.T
    return p[:, :2] / p[:, 2:]


def render(R, t, seed=SEED, noise_seed=0):
    """the (H, W) uint8 picture of the camera X_cam = R X + t"""
    sub = (np.arange(3) - 1) / 3.0
    ys, xs = np.mgrid[0:H, 0:W]
    acc = np.zeros((H, W))
    for oy in sub:
        for ox in sub:
            X = cast(np.stack([xs.ravel() + ox, ys.ravel() + oy], 1), R, t)
            u = X[:, 0] * np.sqrt(1 + SLOPE * SLOPE) / TEXEL
            v = X[:, 1] / TEXEL
            acc += _hash(np.floor(u / BLOCK), np.floor(v / BLOCK), seed).reshape(H, W)
    img = acc / 9 + np.random.default_rng(1000 + noise_seed).normal(0, 2.0, (H, W))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pose_pair():
    """dict(img1, img2, K, R, t): two pinhole views a few degrees and a baseline apart"""
    R, t = ec._rodrigues(R_POSE), np.array(T_POSE)
    return dict(img1=render(np.eye(3), np.zeros(3), noise_seed=1), img2=render(R, t, noise_seed=2), K=K, R=R, t=t)


@functools.lru_cache(maxsize=None)
def rectified_pair():
    """dict(img1, img2, K, R, t): the same scene seen by a rectified pair"""
    R, t = np.eye(3), np.array(T_RECT)
    return dict(img1=render(np.eye(3), np.zeros(3), noise_seed=1), img2=render(R, t, noise_seed=3), K=K, R=R, t=t)


def truth(pair, uvs1):
    """where camera 2 sees the scene points behind camera 1's pixels uvs1"""
    return project(cast(uvs1, np.eye(3), np.zeros(3)), pair["R"], pair["t"])


def colour_of(gray, seed=5):
    """an (h, w, 3) picture whose channels are the gray image under three seeded gains and offsets"""
    rng = np.random.default_rng(seed)
    g = gray.astype(np.float64)[..., None] * rng.uniform(0.6, 1.0, 3) + rng.uniform(0, 40, 3)
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def noise_image(h, w, seed, sigma=20.0):
    return np.clip(np.rint(128 + np.random.default_rng(seed).normal(0, sigma, (h, w))), 0, 255).astype(np.uint8)


def dots_image(h=96, w=96, period=8, value=200, base=50):
    """identical bright dots on a flat field, one per period x period: every dot scores alike, so only the key's pixel index
    tells them apart"""
    img = np.full((h, w), base, np.uint8)
    img[period // 2::period, period // 2::period] = value
    return img


def turned_patches(n=32, size=49, seed=3):
    """(n, size, size) uint8: one smooth random patch turned through a circle in n steps about its centre (bilinear, on the
    host), with a bright blob off centre so that the intensity centroid turns with it"""
    rng = np.random.default_rng(seed)
    big = 4 * size
    base = rng.uniform(60, 120, (big // 8 + 2, big // 8 + 2))
    yy, xx = np.mgrid[0:big, 0:big] / 8.0
    y0, x0 = np.floor(yy).astype(int), np.floor(xx).astype(int)
    fy, fx = yy - y0, xx - x0
    tex = (base[y0, x0] * (1 - fy) * (1 - fx) + base[y0, x0 + 1] * (1 - fy) * fx + base[y0 + 1, x0] * fy * (1 - fx) +
           base[y0 + 1, x0 + 1] * fy * fx)
    c = big / 2
    tex += 120 * np.exp(-(((xx * 8 - c - 7) ** 2 + (yy * 8 - c) ** 2) / (2 * 4.0 ** 2)))
    out = np.empty((n, size, size), np.uint8)
    py, px = np.mgrid[0:size, 0:size] - size // 2
    for k in range(n):
        a = 2 * np.pi * k / n
        sx = c + px * np.cos(a) + py * np.sin(a)  # the source of a pixel: the picture turns by +a (towards +y)
        sy = c - px * np.sin(a) + py * np.cos(a)
        ix, iy = np.floor(sx).astype(int), np.floor(sy).astype(int)
        gx, gy = sx - ix, sy - iy
        v = (tex[iy, ix] * (1 - gy) * (1 - gx) + tex[iy, ix + 1] * (1 - gy) * gx + tex[iy + 1, ix] * gy * (1 - gx) +
             tex[iy + 1, ix + 1] * gy * gx)
        out[k] = np.clip(np.rint(v), 0, 255)
    return out


def random_descriptors(n, seed, duplicates=True):
    """(n, 32) uint8 random rows; with ``duplicates`` some rows repeat earlier ones exactly or up to a few bits"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if duplicates and n >= 4:
        for k in range(n // 4):
            src, dst = rng.integers(0, n, 2)
            d[dst] = d[src]
            if k % 2:
                for bit in rng.integers(0, 256, int(rng.integers(1, 6))):
                    d[dst, bit // 8] ^= np.uint8(1 << (bit % 8))
    return d


def planted_sets(n1, n2, seed):
    """two descriptor sets of which the second holds noisy copies of rows of the first (up to 40 flipped bits), the rest
    random, with exact duplicates planted inside each"""
    rng = np.random.default_rng(seed)
    d1 = random_descriptors(n1, seed)
    d2 = random_descriptors(n2, seed + 1)
    for k in range(min(n1, n2) // 2):
        src, dst = int(rng.integers(0, n1)), int(rng.integers(0, n2))
        d2[dst] = d1[src]
        for bit in rng.integers(0, 256, int(rng.integers(0, 40))):
            d2[dst, bit // 8] ^= np.uint8(1 << (bit % 8))
    return d1, d2
