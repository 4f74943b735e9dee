"""CPU restatement of flow_utils.warp_flow (flow_utils.py:98-129) -- TEST INFRASTRUCTURE ONLY.

The reference's own NumPy restated step by step -- the float64 position of every pixel, the float32 maps of the
backward branch, the rounding, mask and scatter of the forward branch -- with cv2.remap and boxx.resize behind it
through the oracle's restatements (oracle.remap_u8, oracle.resize_linear).  The scatter is written as a reduction
(the largest row-major source index per target) instead of NumPy's fancy assignment, so that this file states the rule
rather than inheriting it; tests/golden/reference_flow.npz, made by the reference's own code, pins the two together.
"""
import numpy as np

import oracle

OUTSIDE = np.float32(-1e4)  # a map value no image reaches: the oracle's remap gives the border there


def positions(flow):
    """(2, h, w) float64: x + float64(flow_x) * w, y + float64(flow_y) * h, product and sum each rounded once."""
    flow = np.asarray(flow)
    assert flow.ndim == 3 and flow.shape[0] == 2 and flow.dtype in (np.float32, np.float64)
    _, h, w = flow.shape
    yy, xx = np.mgrid[:h, :w]
    f = flow.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([xx.astype(np.float64) + f[0] * np.float64(w), yy.astype(np.float64) + f[1] * np.float64(h)])


def backward_maps(flow):
    """The float32 maps of the backward branch; where cvRound(map * 32) leaves int32 on x86 (NaN, infinities, huge
    values: INT_MIN, a cell outside every image) the map is replaced by one that is plainly outside."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = positions(flow).astype(np.float32)
        v = m * np.float32(32)
        ok = (v >= np.float32(-2.0 ** 31)) & (v < np.float32(2.0 ** 31))
    ok = ok[0] & ok[1]
    return np.where(ok, m[0], OUTSIDE), np.where(ok, m[1], OUTSIDE)


def forward_winner(flow, first_wins=False):
    """(h, w) int64: the row-major index of the source pixel each target shows, -1 where nobody lands.  Sources:
    flow_x != 0 or flow_y != 0 (-0.0 is zero, NaN is not), target = round-half-even of the position inside the image.
    Of several sources on a target the LAST in row-major order stays (``first_wins`` = the opposite rule, for the
    test that tells them apart)."""
    flow = np.asarray(flow)
    _, h, w = flow.shape
    with np.errstate(invalid="ignore"):
        t = np.rint(positions(flow))
        takes_part = (flow[0] != 0) | (flow[1] != 0)
        inside = (t[0] >= 0) & (t[0] < w) & (t[1] >= 0) & (t[1] < h)  # in double: NaN and infinities fail here
    src = np.flatnonzero(takes_part & inside)
    target = t[1].ravel()[src].astype(np.int64) * w + t[0].ravel()[src].astype(np.int64)
    if first_wins:
        winner = np.full(h * w, h * w, np.int64)
        np.minimum.at(winner, target, src)
        winner[winner == h * w] = -1
    else:
        winner = np.full(h * w, -1, np.int64)
        np.maximum.at(winner, target, src)
    return winner.reshape(h, w)


def forward_maps(flow, first_wins=False):
    """The float32 maps of the forward branch: the identity, overwritten by the winners' own coordinates."""
    winner = forward_winner(flow, first_wins)
    h, w = winner.shape
    s = np.where(winner >= 0, winner, np.arange(h * w).reshape(h, w))
    return np.float32(s % w), np.float32(s // w)


def warp_flow(flow, img1=None, img2=None, interpolation=oracle.INTER_LINEAR, first_wins=False):
    """One flow (2, h, w), one image (H, W) or (H, W, 3) uint8 -> (h, w[, 3]) uint8."""
    _, h, w = np.asarray(flow).shape
    if img1 is not None:
        mapx, mapy = forward_maps(flow, first_wins)
        return oracle.remap_u8(img1, mapx, mapy, interpolation)
    if tuple(img2.shape[:2]) != (h, w):
        img2 = oracle.resize_linear(img2, (h, w))
    mapx, mapy = backward_maps(flow)
    return oracle.remap_u8(img2, mapx, mapy, interpolation)
