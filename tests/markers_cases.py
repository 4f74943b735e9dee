"""The fixtures of the marker detector (tests/markers_ref.py, csrc/markers.hip): stand-alone markers rendered as
tests/charuco_cases.py renders its boards -- a pinhole view under a pose, every pixel the mean of SS x SS samples taken
through the inverse of the marker's homography -- on white paper, with the analytic place of every marker's four corners
(its own top-left, top-right, bottom-right, bottom-left).  Frames of 160 x 120 and of 157 x 93, markers of 4 x 4 bits with
sides of 24 .. 70 px; one frame of 300 x 260 holds a marker over 200 px, whose mask is a hollow ring.  Masks that stress
the labelling, and a frame of dense blobs that overflows the candidate list.
"""
import functools

import numpy as np

from calibrating_amd import boards

import subpix_cases as sc
from chessboard_cases import rot_z

SS = 4
DARK, BRIGHT, PAPER = sc.DARK, sc.BRIGHT, sc.PAPER
FOCAL, Z = 300.0, 0.3  # a marker of side L metres at Z shows L * 1000 px frontally
HW, ODD_HW, BIG_HW = (120, 160), (93, 157), (260, 300)
DICT4 = boards.make_marker_dictionary(12, 4, seed=3)
DICT6 = boards.make_marker_dictionary(6, 6, seed=4)

# The greatest per-axis distance of a coarse corner from the analytic corner over every marker of SCENES, measured on the
# CPU with the restatement (tests/test_markers_cpu.py prints it; the recording below included): 1.452 px (the corner pixel of a rotated outline is the
# last one dark enough, and a coarse corner is a pixel centre INSIDE the outline).  The bound is that, rounded up to the next
# half pixel; it may not pass 2 px, what corner_sub_pix converges from.
MEASURED_COARSE, MAX_COARSE_OFFSET = 1.452, 1.5
# The same of the corners refined by corner_sub_pix with a (3, 3) window, measured on the first run on the MI355X
# (tests/test_gpu_markers.py prints it): 0.435 px; the bound is that rounded up to the next half pixel, and not above the coarse one.
MEASURED_REFINED, MAX_REFINED_OFFSET = 0.435, 0.5


def homography(hw, side, centre, turn=0.0, rvec=(0.0, 0.0, 0.0)):
    """the marker's own square (u, v, 1), u, v in 0 .. 1 from its top-left corner -> pixels, homogeneous: a marker of
    ``side`` px (seen frontally) whose centre shows at ``centre``, turned ``turn`` degrees in the image after ``rvec``"""
    h, w = hw
    K = np.array([[FOCAL, 0, (w - 1) / 2], [0, FOCAL, (h - 1) / 2], [0, 0, 1]])
    R = rot_z(turn) @ sc.rodrigues(rvec)
    L = side / 1000.0
    t = np.array([(centre[0] - K[0, 2]) * Z / FOCAL, (centre[1] - K[1, 2]) * Z / FOCAL, Z])
    return K @ np.stack([R[:, 0], R[:, 1], t], 1) @ np.array([[L, 0, -L / 2], [0, L, -L / 2], [0, 0, 1]])


def corners_of(Hm):
    p = np.array([[0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1.0]]) @ Hm.T
    return p[:, :2] / p[:, 2:]


def render(hw, placed, dictionary):
    """``placed``: [(id, homography)] -> (h, w) uint8"""
    h, w = hw
    c = dictionary.shape[1] + 2
    sub = (np.arange(SS) + 0.5) / SS - 0.5
    value = np.full((h * SS, w * SS), float(PAPER))
    for i, Hm in placed:
        box = corners_of(Hm)  # (only the pixels the marker can reach are sampled)
        x0, y0 = np.clip(np.floor(box.min(0)).astype(int) - 1, 0, (w, h))
        x1, y1 = np.clip(np.ceil(box.max(0)).astype(int) + 2, 0, (w, h))
        if x1 <= x0 or y1 <= y0:
            continue
        gx, gy = np.meshgrid((np.arange(x0, x1)[:, None] + sub[None]).reshape(-1), (np.arange(y0, y1)[:, None] + sub[None]).reshape(-1))
        q = np.stack([gx, gy, np.ones_like(gx)], -1) @ np.linalg.inv(Hm).T
        u, v = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
        inside = (u >= 0) & (u < 1) & (v >= 0) & (v < 1)
        cells = np.zeros((c, c), np.uint8)
        cells[1:-1, 1:-1] = dictionary[i]
        white = cells[np.clip(np.floor(v * c).astype(int), 0, c - 1), np.clip(np.floor(u * c).astype(int), 0, c - 1)] == 1
        part = value[y0 * SS:y1 * SS, x0 * SS:x1 * SS]
        part[...] = np.where(inside, np.where(white, BRIGHT, DARK), part)
    return np.rint(value.reshape(h, SS, w, SS).mean((1, 3))).astype(np.uint8)


TILT = (0.5, -0.4, 0.0)
# name -> (frame size, dictionary, [(id, side, centre, turn, rvec)], noise sigma)
SCENES = {
    "frontal": (HW, DICT4, [(3, 40, (80, 60), 0.0, (0, 0, 0))], 0),
    "rot30": (HW, DICT4, [(4, 44, (76, 58), 30.0, (0, 0, 0))], 0),
    "rot45": (HW, DICT4, [(0, 42, (84, 61), 45.0, (0, 0, 0))], 0),
    "tilted": (HW, DICT4, [(7, 52, (80, 60), 8.0, TILT)], 0),
    "turn90": (HW, DICT4, [(3, 36, (70, 55), 90.0, (0, 0, 0))], 0),
    "turn180": (HW, DICT4, [(3, 36, (90, 62), 180.0, (0.1, 0, 0))], 0),
    "turn270": (HW, DICT4, [(3, 36, (81, 64), 270.0, (0, 0.1, 0))], 0),
    "two": (HW, DICT4, [(1, 30, (42, 60), 5.0, (0, 0, 0)), (5, 34, (114, 56), -12.0, (0.2, 0.1, 0))], 0),
    "twice": (HW, DICT4, [(2, 28, (40, 70), 0.0, (0, 0, 0)), (2, 36, (112, 50), 20.0, (0, 0, 0))], 0),
    "tiles": (HW, DICT4, [(9, 70, (80, 60), 10.0, (0, 0, 0))], 0),
    "small24": (HW, DICT4, [(6, 24, (81, 60), 3.0, (0, 0, 0))], 0),
    "noisy": (HW, DICT4, [(7, 52, (80, 60), 8.0, TILT)], 4),
    "six": (HW, DICT6, [(2, 64, (80, 60), -7.0, (0.1, 0.1, 0))], 0),
    "odd": (ODD_HW, DICT4, [(8, 38, (60, 45), 17.0, (0, 0, 0)), (10, 30, (120, 50), 0.0, (0, 0.3, 0))], 0),
    "odd_tilted": (ODD_HW, DICT4, [(11, 46, (78, 46), -30.0, (0.3, 0.3, 0))], 0),
    "big": (BIG_HW, DICT4, [(5, 210, (150, 130), 4.0, (0, 0, 0))], 0),
}
# frames in which no marker may be seen: cut by the image's edge, smaller than min_side, none at all
NO_MARKER = {
    "cut": (HW, DICT4, [(3, 40, (150, 60), 0.0, (0, 0, 0))], 0),
    "tiny": (HW, DICT4, [(3, 10, (80, 60), 0.0, (0, 0, 0))], 0),
    "blank": (HW, DICT4, [], 0),
    "noise": (HW, DICT4, [], 4),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """dict(img, dictionary, truth {id: [(4, 2), ...]} -- one entry per copy of a marker)"""
    hw, dictionary, markers, sigma = SCENES[name] if name in SCENES else NO_MARKER[name]
    placed = [(i, homography(hw, side, centre, turn, rvec)) for i, side, centre, turn, rvec in markers]
    img = render(hw, placed, dictionary)
    if sigma:
        noisy = img.astype(np.float64) + np.random.default_rng(5).normal(0, sigma, img.shape)
        img = np.clip(np.rint(noisy), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    truth = {}
    if name in SCENES:
        for i, Hm in placed:
            truth.setdefault(i, []).append(corners_of(Hm))
    return dict(img=img, dictionary=dictionary, truth=truth)


def batch(hw=HW, dictionary=DICT4):
    """(images (f, h, w), names): every scene of that size and dictionary, those without a marker included"""
    both = dict(SCENES, **NO_MARKER)
    names = [k for k, v in both.items() if v[0] == hw and v[1] is dictionary]
    return np.stack([scene(k)["img"] for k in names]), names


def offsets(name, seen, corners):
    """the per-axis distances (k, 4, 2) of a scene's seen corners from the analytic ones; asserts that exactly the scene's
    markers are seen, each at one of its copies"""
    truth = scene(name)["truth"]
    assert sorted(np.flatnonzero(seen).tolist()) == sorted(truth), (name, np.flatnonzero(seen), sorted(truth))
    out = [min((np.abs(corners[i] - t) for t in copies), key=lambda d: d.max()) for i, copies in truth.items()]
    return np.stack(out) if out else np.zeros((0, 4, 2))


# ---- masks for the labelling alone: 70 x 100, several tiles of 32 x 32 each way ----
def label_masks():
    h, w = 70, 100
    serpentine = np.zeros((h, w), np.uint8)
    serpentine[::2] = 1
    serpentine[1::4, -1] = 1
    serpentine[3::4, 0] = 1
    comb = np.zeros((h, w), np.uint8)
    comb[0] = 1
    comb[:, ::2] = 1
    spiral = np.zeros((h, w), np.uint8)
    a, b, c, d = 0, h - 1, 0, w - 1
    while a <= b and c <= d:  # a square spiral two pixels apart, one component
        spiral[a, c:d + 1] = 1
        spiral[a:b + 1, d] = 1
        spiral[b, c + 2:d + 1] = 1 if c + 2 <= d else 0
        spiral[a + 2:b + 1, c + 2] = 1 if c + 2 <= d else 0
        a, b, c, d = a + 2, b - 2, c + 2, d - 2
    checker = (np.add.outer(np.arange(h), np.arange(w)) % 2).astype(np.uint8)
    touch = np.zeros((h, w), np.uint8)  # blocks that meet only at the tiles' corners: apart under 4-connectivity
    for ty in range(3):
        for tx in range(4):
            if (tx + ty) % 2 == 0:
                touch[32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32] = 1
    names = ["serpentine", "comb", "spiral", "all_dark", "checker", "touch"]
    return np.stack([serpentine, comb, spiral, np.ones((h, w), np.uint8), checker, touch]), names


def overflow_frame():
    """blobs of 5 x 5 every 7 px on paper, 41 x 36 of them: with min_side = 4 more than 1024 candidates"""
    img = np.full(BIG_HW, PAPER, np.uint8)
    for y in range(4, BIG_HW[0] - 9, 7):
        for x in range(4, BIG_HW[1] - 9, 7):
            img[y:y + 5, x:x + 5] = DARK
    return img


# ---- a recording of a 4 x 3 grid board: 12 frames of 320 x 240, some with covered markers ----
GRID, GRID_LENGTH_MM, GRID_SEPARATION_MM, REC_HW, REC_FOCAL = (4, 3), 30.0, 6.0, (240, 320), 300.0
REC_DICT = boards.make_marker_dictionary(12, 4, seed=7)
REC_K = np.array([[REC_FOCAL, 0, (REC_HW[1] - 1) / 2], [0, REC_FOCAL, (REC_HW[0] - 1) / 2], [0, 0, 1]])
# (rotation vector, the board centre's place in metres, the ids painted over)
RECORDING = [((0.0, 0.0, 0.02), (0.0, 0.0, 0.17), ()),
             ((0.3, 0.0, -0.02), (-0.004, 0.004, 0.19), ()),
             ((-0.28, 0.1, 0.03), (0.0, 0.004, 0.18), (0,)),
             ((0.1, 0.32, 0.0), (0.005, -0.004, 0.19), ()),
             ((0.0, -0.35, 0.05), (-0.005, 0.0, 0.2), (5, 6)),
             ((0.25, 0.25, -0.05), (0.004, 0.003, 0.2), ()),
             ((-0.2, -0.25, 0.08), (0.0, 0.0, 0.21), (11,)),
             ((0.33, -0.1, 0.0), (0.002, -0.003, 0.2), ()),
             ((-0.1, 0.3, -0.1), (-0.004, 0.0, 0.2), (3, 7)),
             ((0.2, -0.3, 0.1), (0.0, -0.002, 0.18), ()),
             ((-0.3, 0.0, 0.0), (-0.003, -0.002, 0.18), ()),
             ((0.15, 0.15, 0.2), (0.0, 0.002, 0.21), (8,))]


def grid_points():
    """{id: (4, 3)} float64 metres of the grid, stated apart from boards.py: marker j * gx + i at (i, j) * pitch, centred"""
    gx, gy = GRID
    L, P = GRID_LENGTH_MM / 1000, (GRID_LENGTH_MM + GRID_SEPARATION_MM) / 1000
    pts = {j * gx + i: np.array([[i * P, j * P, 0], [i * P + L, j * P, 0], [i * P + L, j * P + L, 0], [i * P, j * P + L, 0]])
           for j in range(gy) for i in range(gx)}
    centre = np.concatenate(list(pts.values())).mean(0)
    return {k: p - centre for k, p in pts.items()}


@functools.lru_cache(maxsize=None)
def recording():
    """(images (12, 240, 320), truth (12, 12, 4, 2), shown (12, 12) bool)"""
    pts = grid_points()
    images, truths, shown = [], [], []
    for rvec, t, covered in RECORDING:
        R = sc.rodrigues(rvec)
        placed, tr = [], []
        for i in sorted(pts):
            p = pts[i]
            L = GRID_LENGTH_MM / 1000
            Hm = REC_K @ np.stack([R[:, 0], R[:, 1], R @ p[0] + np.array(t)], 1) @ np.diag([L, L, 1.0])
            tr.append(corners_of(Hm))
            if i not in covered:
                placed.append((i, Hm))
        images.append(render(REC_HW, placed, REC_DICT))
        truths.append(np.stack(tr))
        shown.append([i not in covered for i in sorted(pts)])
    out = np.stack(images), np.stack(truths), np.array(shown)
    for a in out:
        a.setflags(write=False)
    return out
