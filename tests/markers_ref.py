"""NumPy restatement of the marker detector's stages 1 to 6 (csrc/markers.hip): dark mask, connected components,
candidates, quadrilateral, decode, the winner per id -- integers end to end, so the kernels are pinned to it bit for bit
(tests/test_gpu_markers.py) and it is pinned to rendered markers with analytic corners (tests/test_markers_cpu.py).  The
sampling and matching of a marker are tests/charuco_ref.py's ``decode`` with the marker filling its cell (ratio 1 / 1).
The contract is this package's own, not cv2.aruco's.
"""
import numpy as np

import charuco_ref as cref

CAPACITY = 1024
MAX_SIDE, MAX_RADIUS, MAX_BOX, MIN_SIDE, MAX_BITS, MAX_IDS = 16384, 32, 1024, 4, 8, 1024
OVERFLOW = 2
PIX = (1 << 28) - 1
CROSS_BIAS = 1 << 22


def check_arguments(dictionary, block_radius=8, offset=7, min_side=12, max_side=512, max_errors=0):
    d = np.asarray(dictionary)
    if any(int(v) != v for v in (block_radius, offset, min_side, max_side, max_errors)):
        raise ValueError("integers")
    if not 1 <= block_radius <= MAX_RADIUS or not -255 <= offset <= 255:
        raise ValueError("mask")
    if not MIN_SIDE <= min_side <= max_side <= MAX_BOX:
        raise ValueError("sides")
    if d.ndim != 3 or d.shape[1] != d.shape[2] or not 4 <= d.shape[1] <= MAX_BITS or not 1 <= len(d) <= MAX_IDS:
        raise ValueError("dictionary")
    if not 0 <= max_errors <= d.shape[1] ** 2:
        raise ValueError("max_errors")


def dark_mask(gray, r=8, offset=7):
    """(h, w) uint8 -> uint8: 1 iff (gray + offset) * A < S over the (2r + 1)^2 window clipped to the image"""
    g = np.asarray(gray).astype(np.int64)
    h, w = g.shape
    c = np.zeros((h + 1, w + 1), np.int64)
    c[1:, 1:] = g.cumsum(0).cumsum(1)
    ya, yb = np.clip(np.arange(h) - r, 0, h)[:, None], np.clip(np.arange(h) + r + 1, 0, h)[:, None]
    xa, xb = np.clip(np.arange(w) - r, 0, w)[None], np.clip(np.arange(w) + r + 1, 0, w)[None]
    S = c[yb, xb] - c[ya, xb] - c[yb, xa] + c[ya, xa]
    A = (yb - ya) * (xb - xa)
    return ((g + offset) * A < S).astype(np.uint8)


def label(mask):
    """(h, w) -> int32: the least y * w + x of a pixel's 4-connected component of mask != 0, -1 where mask == 0.  Runs of a
    row joined to the runs above that they overlap, by union-find on run numbers (a lower number starts at a lower index)."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    parent, start = [], []
    run_of = np.full((h, w), -1, np.int64)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for y in range(h):
        d = np.diff(np.concatenate([[0], m[y].astype(np.int8), [0]]))
        for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)):
            k = len(parent)
            parent.append(k)
            start.append(y * w + a)
            run_of[y, a:b] = k
            if y:
                for q in np.unique(run_of[y - 1, a:b]):
                    if q >= 0:
                        ra, rb = find(int(q)), find(k)
                        if ra != rb:
                            parent[max(ra, rb)] = min(ra, rb)
    out = np.full((h, w), -1, np.int32)
    if parent:
        root_start = np.array([start[find(k)] for k in range(len(parent))], np.int32)
        out[m] = root_start[run_of[m]]
    return out


def candidates(labels, min_side=12, max_side=512):
    """-> (rows (m, 6) int32 of (root, x0, y0, x1, y1, pixels) in the order of the roots, all of them)"""
    L = np.asarray(labels)
    h, w = L.shape
    ys, xs = np.nonzero(L >= 0)
    lab = L[ys, xs]
    roots, inverse, count = np.unique(lab, return_inverse=True, return_counts=True)
    x0 = np.full(len(roots), w)
    y0, x1, y1 = np.full(len(roots), h), np.full(len(roots), -1), np.full(len(roots), -1)
    np.minimum.at(x0, inverse, xs), np.minimum.at(y0, inverse, ys), np.maximum.at(x1, inverse, xs), np.maximum.at(y1, inverse, ys)
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    keep = (bw >= min_side) & (bw <= max_side) & (bh >= min_side) & (bh <= max_side) & (x0 > 0) & (y0 > 0) & (x1 < w - 1) & (y1 < h - 1)
    return np.stack([roots, x0, y0, x1, y1, count], 1)[keep].astype(np.int32).reshape(-1, 6)


def quad(labels, cand, min_side=12):
    """the outline's four extreme pixels, clockwise in image coordinates: (4, 2) int64 of (x, y), or None where rejected"""
    L = np.asarray(labels)
    w = L.shape[1]
    root, x0, y0, x1, y1 = (int(v) for v in cand[:5])
    ys, xs = np.nonzero(L[y0:y1 + 1, x0:x1 + 1] == root)
    ys, xs = ys.astype(np.int64) + y0, xs.astype(np.int64) + x0
    p = ys * w + xs

    def far(d):
        return int(PIX - (((d << 28) | (PIX - p)).max() & PIX))
    pa = far((2 * xs - (x0 + x1)) ** 2 + (2 * ys - (y0 + y1)) ** 2)
    ax, ay = pa % w, pa // w
    pb = far((xs - ax) ** 2 + (ys - ay) ** 2)
    bx, by = pb % w, pb // w
    cr = (bx - ax) * (ys - ay) - (by - ay) * (xs - ax)
    kc, kd = int((((cr + CROSS_BIAS) << 28) | (PIX - p)).max()), int((((cr + CROSS_BIAS) << 28) | p).min())
    pc, pd = PIX - (kc & PIX), kd & PIX
    if (kc >> 28) - CROSS_BIAS <= 0 or (kd >> 28) - CROSS_BIAS >= 0:
        return None
    q = np.array([[ax, ay], [pd % w, pd // w], [bx, by], [pc % w, pc // w]], np.int64)
    for k in range(4):
        e, f = q[(k + 1) % 4] - q[k], q[(k + 2) % 4] - q[(k + 1) % 4]
        if e[0] * f[1] - e[1] * f[0] <= 0 or int(e @ e) < min_side * min_side:
            return None
    return q


def decode(gray, q, s, words, max_errors=0):
    """the marker inside the clockwise quadrilateral q -> (errors, id, turn) or None"""
    for e in range(max_errors + 1):  # (charuco_ref.decode keeps the least (errors, id, turn) and does not say the errors)
        got = cref.decode(gray, (q[0], q[1], q[3], q[2]), s, 1, 1, words, e)
        if got is not None:
            return (e,) + got
    return None


def find_one(gray, dictionary, words, block_radius=8, offset=7, min_side=12, max_side=512, max_errors=0):
    g = np.asarray(gray)
    n_ids, s = len(dictionary), np.shape(dictionary)[1]
    mask = dark_mask(g, block_radius, offset)
    labels = label(mask)
    cand = candidates(labels, min_side, max_side)
    out = dict(mask=mask, labels=labels, counts=np.int32(len(cand)), status=np.int32(OVERFLOW if len(cand) > CAPACITY else 0),
               candidates=np.full((CAPACITY, 6), -1, np.int32), quads=np.full((CAPACITY, 4, 2), -1, np.int32),
               id_turn=np.full(CAPACITY, -1, np.int32), seen=np.zeros(n_ids, bool), corners=np.full((n_ids, 4, 2), np.nan, np.float32))
    out["candidates"][:min(len(cand), CAPACITY)] = cand[:CAPACITY]
    if len(cand) > CAPACITY:
        return out
    best = {}
    for k, c in enumerate(cand):
        q = quad(labels, c, min_side)
        if q is None:
            continue
        out["quads"][k] = q
        got = decode(g, q, s, words, max_errors)
        if got is None:
            continue
        err, i, turn = got
        out["id_turn"][k] = i << 2 | turn
        best[i] = min(best.get(i, (err, k)), (err, k))
    for i, (_, k) in best.items():
        out["seen"][i] = True
        out["corners"][i] = np.roll(out["quads"][k], -(int(out["id_turn"][k]) & 3), axis=0)
    return out


def find(gray, dictionary, **kw):
    """every stage on gray (f, h, w) or (h, w): dict of arrays with a leading frame axis"""
    check_arguments(dictionary, **kw)
    g = np.asarray(gray)
    g = g[None] if g.ndim == 2 else g
    words = cref.words(dictionary)
    frames = [find_one(f, dictionary, words, **kw) for f in g]
    return {k: np.stack([f[k] for f in frames]) for k in frames[0]}
