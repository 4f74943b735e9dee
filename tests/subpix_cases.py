"""Rendered checkerboards with analytic corners for the sub-pixel refinement (tests/subpix_ref.py, csrc/subpix.hip).

A board of 5 x 4 squares of 25 mm -- 4 x 3 inner corners, ``Chessboard((4, 3))`` -- seen by a pinhole camera of 128 x 96
pixels under a pose: every pixel is the mean of SS x SS samples taken through the inverse of the plane's homography
(supersampled inverse mapping), so an edge is as sharp as the pixel grid allows and a corner's true place is the
homography of its board coordinates, known to float64.  Seeds are the true corners moved by up to +-2 px.

What the restatement (tests/subpix_ref.py, either summation order) does on these frames with the reference's arguments
-- window (4, 4), criteria (30, 0.01) --, measured, for nobody to rely on anything tighter: every seed, up to 2.83 px
from its corner, ends closer to it than it started, after 2 to 5 rounds; the largest distance left is 0.114, 0.108,
0.097, 0.132 and 0.073 px on frames 0 .. 4.  That remainder is the method's own bias on a perspective view of 18 px
squares box-filtered to the pixel grid, not rounding.  tests/test_subpix_cpu.py asserts "closer than it started" only.
"""
import functools
import os

import numpy as np

H, W, SS = 96, 128, 8
COLS, ROWS, SQUARE = 4, 3, 0.025  # inner corners and the square's side in metres
DARK, BRIGHT, PAPER = 40, 215, 235
K = np.array([[150.0, 0, 63.5], [0, 150.0, 47.5], [0, 0, 1]])
# (rotation vector, translation) of the board's centre in the camera
POSES = [((0.0, 0.0, 0.05), (0.002, -0.001, 0.21)),
         ((0.42, -0.1, -0.08), (-0.004, 0.003, 0.22)),
         ((-0.15, 0.45, 0.12), (0.003, 0.002, 0.23)),
         ((-0.38, -0.33, -0.04), (0.0, -0.002, 0.22)),
         ((0.3, 0.36, 0.3), (-0.002, 0.0, 0.24))]
FRAMES = 3  # the refinement's own cases; all of POSES feed the calibration chain
MAX_SEED_OFFSET = 2.0


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pose_T(i):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rodrigues(POSES[i][0]), POSES[i][1]
    return T


def object_points():
    """the inner corners in metres, the board's centre at the origin, x fastest: what ``Chessboard((4, 3))`` holds"""
    xy = np.mgrid[:COLS, :ROWS].T.reshape(-1, 2) * SQUARE
    return np.concatenate([xy - xy.mean(0), np.zeros((len(xy), 1))], 1)


def homography(i):
    """board metres (x, y, 1) -> pixel, homogeneous"""
    T = pose_T(i)
    return K @ np.stack([T[:3, 0], T[:3, 1], T[:3, 3]], 1)


def render(Hm, h, w, cols=COLS, rows=ROWS, ss=SS):
    """the board of (cols + 1) x (rows + 1) squares under the homography Hm (board metres -> pixels): (h, w) uint8"""
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    xs = (np.arange(w)[:, None] + sub[None]).reshape(-1)
    ys = (np.arange(h)[:, None] + sub[None]).reshape(-1)
    gx, gy = np.meshgrid(xs, ys)
    q = np.stack([gx, gy, np.ones_like(gx)], -1) @ np.linalg.inv(Hm).T
    u = q[..., 0] / q[..., 2] / SQUARE + (cols + 1) / 2  # in squares, from the board's corner
    v = q[..., 1] / q[..., 2] / SQUARE + (rows + 1) / 2
    inside = (u >= 0) & (u < cols + 1) & (v >= 0) & (v < rows + 1)
    value = np.where((np.floor(u) + np.floor(v)) % 2 == 0, DARK, BRIGHT)
    value = np.where(inside, value, PAPER).astype(np.float64)
    return np.rint(value.reshape(h, ss, w, ss).mean((1, 3))).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def frame(i):
    """dict(img (H, W) uint8, truth (12, 2) float64, seeds (12, 2) float32) of pose i; the arrays are read-only"""
    Hm = homography(i)
    o = object_points()
    p = np.concatenate([o[:, :2], np.ones((len(o), 1))], 1) @ Hm.T
    truth = p[:, :2] / p[:, 2:]
    img = render(Hm, H, W)
    rng = np.random.default_rng(100 + i)
    off = rng.uniform(-MAX_SEED_OFFSET, MAX_SEED_OFFSET, truth.shape)
    off[0], off[1] = (MAX_SEED_OFFSET, -MAX_SEED_OFFSET), (-MAX_SEED_OFFSET, MAX_SEED_OFFSET)  # the far ends, always
    out = dict(img=img, truth=truth, seeds=(truth + off).astype(np.float32))
    for a in out.values():
        a.setflags(write=False)
    return out


def colour(img):
    """an RGB picture whose channels differ, so that a swapped weight shows: the gray image tinted"""
    g = img.astype(np.int64)
    return np.stack([np.clip(g + 17, 0, 255), np.clip(g - 9, 0, 255), 255 - g], -1).astype(np.uint8)


def batch(n=FRAMES):
    """(images (n, H, W), seeds (n, 12, 2) float32, truth (n, 12, 2))"""
    fr = [frame(i) for i in range(n)]
    return np.stack([f["img"] for f in fr]), np.stack([f["seeds"] for f in fr]), np.stack([f["truth"] for f in fr])


# ---- the two summation orders of the restatement against each other (tests/golden/subpix_order.json) ----
ORDER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "subpix_order.json")
ORDER_WINDOWS = [(4, 4), (5, 3), (11, 11)]


def measure_order():
    """The restatement's switches against each other on every fixture corner and window: order="wave" against
    order="cv2", and bilinear="running" against bilinear="four_tap"  -- whether iteration counts
    and status agree and the largest difference of a refined coordinate in pixels.  ``python tests/subpix_cases.py``
    writes the file; tests/test_subpix_cpu.py compares a fresh measurement with it."""
    import subpix_ref as ref
    worst, same_iterations, corners = 0.0, True, 0
    bilinear_worst, bilinear_same = 0.0, True
    for i in range(len(POSES)):
        f = frame(i)
        for win in ORDER_WINDOWS:
            a = ref.corner_sub_pix(f["img"], f["seeds"], win=win, order="cv2")
            b = ref.corner_sub_pix(f["img"], f["seeds"], win=win, order="wave")
            worst = max(worst, float(np.abs(a[0].astype(np.float64) - b[0]).max()))
            same_iterations = same_iterations and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            r = ref.corner_sub_pix(f["img"], f["seeds"], win=win, order="cv2", bilinear="running")
            bilinear_worst = max(bilinear_worst, float(np.abs(a[0].astype(np.float64) - r[0]).max()))
            bilinear_same = bilinear_same and np.array_equal(a[1], r[1]) and np.array_equal(a[2], r[2])
            corners += len(f["seeds"])
    return dict(corner_disagreement=worst, same_iterations=bool(same_iterations), corners=corners,
                bilinear_disagreement=bilinear_worst, bilinear_same_iterations=bool(bilinear_same))


# ---- 13 x 13 pictures, cv2's smallest for a window of (4, 4): every patch reads across a border ----
def _render13(value):
    sub = (np.arange(SS) + 0.5) / SS - 0.5
    xs = (np.arange(13)[:, None] + sub[None]).reshape(-1)
    gx, gy = np.meshgrid(xs, xs)
    return np.rint(value(gx, gy).astype(np.float64).reshape(13, SS, 13, SS).mean((1, 3))).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def small_corner():
    """(img, starts): one checker corner at (6.3, 6.6), turned by 0.2 rad; starts beside every border and near the corner"""
    th = 0.2
    img = _render13(lambda x, y: np.where((((x - 6.3) * np.cos(th) + (y - 6.6) * np.sin(th)) > 0)
                                           ^ ((-(x - 6.3) * np.sin(th) + (y - 6.6) * np.cos(th)) > 0), DARK, BRIGHT))
    starts = np.array([[0.2, 6], [12.7, 6], [6, 0.1], [6, 12.9], [0, 0], [12.9, 12.9], [6, 6], [3.5, 9.25], [8.75, 4.5]], np.float32)
    return img, starts


@functools.lru_cache(maxsize=None)
def slanted_edge():
    """(img, starts): one straight edge, 0.1 x + y = 6.5 -- a nearly singular window, whose step runs along the edge: the
    first two starts leave the image on the left (status 2), the next two drift further than the window (4 too)"""
    img = _render13(lambda x, y: np.where(0.1 * x + y > 6.5, 200, 60))
    return img, np.array([[1, 4], [1, 6], [3, 4], [3, 8]], np.float32)


if __name__ == "__main__":
    import json
    m = measure_order()
    with open(ORDER_PATH, "w") as fh:
        json.dump(m, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(m)
