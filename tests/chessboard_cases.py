"""The fixtures of the chessboard detector (tests/chessboard_ref.py, csrc/chessboard.hip): the rendered boards of
tests/subpix_cases.py and further renders of the same kind, all 128 x 96, each with its analytic corners in the order
the detector's rule gives them; frames without a board; a hand-made response plane with ties.
"""
import functools

import numpy as np

import subpix_cases as sc

PATTERN = (sc.COLS, sc.ROWS)
SQUARE_PATTERN = (4, 4)
MAX_OFFSET = sc.MAX_SEED_OFFSET  # per axis, of a detected corner from the analytic one: what the refinement converges from


def rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def view(pose, turn=0.0, cols=sc.COLS, rows=sc.ROWS, shift=(0.0, 0.0), z=None):
    """(img (96, 128) uint8, truth (rows, cols, 2) float64 in the board's own numbering) of POSES[pose] turned by ``turn``
    degrees about the optical axis, moved by ``shift`` metres across the view, at depth ``z`` if given"""
    T = sc.pose_T(pose)
    R = rot_z(turn) @ T[:3, :3]
    t = T[:3, 3] + np.array([shift[0], shift[1], 0.0])
    if z is not None:
        t[2] = z
    Hm = sc.K @ np.stack([R[:, 0], R[:, 1], t], 1)
    xy = np.mgrid[:cols, :rows].T.reshape(-1, 2) * sc.SQUARE
    o = np.concatenate([xy - xy.mean(0), np.ones((len(xy), 1))], 1)
    p = o @ Hm.T
    return sc.render(Hm, sc.H, sc.W, cols, rows), (p[:, :2] / p[:, 2:]).reshape(rows, cols, 2)


def rule_order(grid, w=sc.W):
    """The analytic corners (down, across, 2) numbered as the detector's rule numbers them: of the turns of the board
    that keep its shape (a half turn; a square board: the quarter turns too) -- all right-handed, a mirrored numbering is
    not -- the one whose corner 0 has the lowest y * w + x -> (n, 2)"""
    turns = [grid, grid[::-1, ::-1]]
    if grid.shape[0] == grid.shape[1]:
        turns += [grid.transpose(1, 0, 2)[::-1], grid.transpose(1, 0, 2)[:, ::-1]]
    for g in turns:
        sc_, sr_ = (g[:, -1] - g[:, 0]).sum(0), (g[-1] - g[0]).sum(0)
        assert sc_[0] * sr_[1] - sc_[1] * sr_[0] > 0
    keys = [np.floor(g[0, 0, 1] + 0.5) * w + g[0, 0, 0] for g in turns]
    assert np.diff(np.sort([g[0, 0, 1] for g in turns])).min() > 2 * MAX_OFFSET  # (no fixture leaves the choice to a pixel)
    return turns[int(np.argmin(keys))].reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def boards():
    """name -> (img, truth (12, 2) in rule order): the frames a (4, 3) board is found in"""
    out = {}
    for i in range(len(sc.POSES)):
        f = sc.frame(i)
        out["pose%d" % i] = (f["img"], rule_order(f["truth"].reshape(sc.ROWS, sc.COLS, 2)))
    for name, pose, turn in (("quarter_turn", 1, 93.0), ("half_turn", 2, 177.0), ("quarter_turn_back", 3, -88.0)):
        img, truth = view(pose, turn)
        out[name] = (img, rule_order(truth))
    noisy = sc.frame(1)["img"].astype(np.float64) + np.random.default_rng(4).normal(0, 4, (sc.H, sc.W))
    out["noise"] = (np.clip(np.rint(noisy), 0, 255).astype(np.uint8), out["pose1"][1])
    for img, truth in out.values():
        img.setflags(write=False)
        truth.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def square_board():
    """(img, truth (16, 2) in rule order) of a 4 x 4 board, further away so that its 5 x 5 squares fit the view"""
    img, truth = view(4, 20.0, 4, 4, z=0.27)
    img.setflags(write=False)
    return img, rule_order(truth)


@functools.lru_cache(maxsize=None)
def blank():
    return np.full((sc.H, sc.W), sc.PAPER, np.uint8)


@functools.lru_cache(maxsize=None)
def cut_board():
    """pose 0 moved right until the image edge cuts the board's last columns of corners off"""
    img, truth = view(0, shift=(0.06, 0.0))
    assert (truth[..., 0] > sc.W).any() and (truth[..., 0] < sc.W - 10).any()
    return img


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """(images (f, 96, 128), names) -- found and unfound frames of a (4, 3) pattern side by side"""
    b = boards()
    names = list(b) + ["blank", "cut", "square"]
    return np.stack([b[k][0] for k in b] + [blank(), cut_board(), square_board()[0]]), names


def fine_checker(side=256, square=12):
    """a checker of 12 px squares all over the image: 20 x 20 corners at 256 x 256, and 42 x 42 at 512 x 512, more than the
    1024 candidates a frame keeps"""
    y, x = np.mgrid[:side, :side]
    return np.where(((x // square) + (y // square)) % 2 == 0, sc.DARK, sc.BRIGHT).astype(np.uint8)


def tie_plane():
    """(response (1, 12, 16) int16, rmax, the candidates (x, y) with relative 8 and radius 1 / radius 2): plateaus of
    equal responses, a peak beside the border, a peak below the relative threshold"""
    r = np.zeros((1, 12, 16), np.int16)
    r[0, 2, 2:5] = 800            # a horizontal plateau: its first pixel stays
    r[0, 5:8, 9] = 640            # a vertical plateau: its top pixel stays
    r[0, 6, 10] = 640             # ... which also comes before this one
    r[0, 0, 15] = 500             # a corner of the plane: the window is clipped
    r[0, 10, 1], r[0, 11, 2] = 300, 300  # diagonal neighbours: the upper one
    r[0, 10, 8] = 99              # 8 * 99 < 800
    r[0, 9, 13], r[0, 9, 15] = 100, 101  # two apart: both peaks at radius 1, only the stronger at radius 2
    r[0, 4, 13] = -5
    rmax = np.array([800], np.int32)
    radius1 = [(15, 0), (2, 2), (9, 5), (13, 9), (15, 9), (1, 10)]
    radius2 = [(15, 0), (2, 2), (9, 5), (15, 9), (1, 10)]
    return r, rmax, radius1, radius2
