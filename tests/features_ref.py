"""NumPy restatement of the feature detector, descriptor and matcher (csrc/features.hip, calibrating_amd/features.py):
every stage in integer arrays and plain loops, as include/calibrating_amd.h states it.  Test infrastructure only; it calls
none of the package's kernels.  The pattern table comes from ``features.brief_pattern``, which is host Python."""
import numpy as np

from calibrating_amd import imgproc
from calibrating_amd.features import brief_pattern

BORDER = 16
RING = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
        (-2, -2), (-1, -3)]
COS = [int(np.rint(16384 * np.cos(2 * np.pi * k / 32))) for k in range(32)]
SIN = [int(np.rint(16384 * np.sin(2 * np.pi * k / 32))) for k in range(32)]
POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int32)


def gray_of(img, code="rgb"):
    """cvt_gray's formula on the host: (c0 k0 + c1 k1 + c2 k2 + half) >> bits; gray input comes back as it is"""
    img = np.asarray(img)
    if img.shape[-1] != 3 or img.ndim < 3:
        return img
    by, gy, ry = imgproc.GRAY_WEIGHTS[imgproc.GRAY_BITS]
    k = (by, gy, ry) if code == "bgr" else (ry, gy, by)
    c = img.astype(np.int64)
    return ((c[..., 0] * k[0] + c[..., 1] * k[1] + c[..., 2] * k[2] + (1 << (imgproc.GRAY_BITS - 1))) >> imgproc.GRAY_BITS).astype(np.uint8)


def score_plane(gray, threshold=20):
    """(h, w) uint8: the FAST-9 score, 0 below the threshold and within BORDER of an edge"""
    g = np.asarray(gray).astype(np.int32)
    h, w = g.shape
    out = np.zeros((h, w), np.uint8)
    if h < 2 * BORDER + 1 or w < 2 * BORDER + 1:
        return out
    c = g[BORDER:h - BORDER, BORDER:w - BORDER]
    d = np.stack([g[BORDER + dy:h - BORDER + dy, BORDER + dx:w - BORDER + dx] - c for dx, dy in RING])
    best = np.zeros_like(c)
    for s in range(16):
        arc = d[[(s + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), -arc.max(0)))
    out[BORDER:h - BORDER, BORDER:w - BORDER] = np.where(best >= threshold, best, 0)
    return out


def keys_of(score):
    h, w = score.shape
    index = np.arange(h * w, dtype=np.uint64).reshape(h, w)
    return (score.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - index)


def keypoints(score, cell=8):
    """(xy (n, 2) int32, scores (n,) int32) of one score plane, in row-major order of the blocks"""
    h, w = score.shape
    key = keys_of(score)
    pad = np.zeros((h + 2, w + 2), np.uint64)
    pad[1:-1, 1:-1] = key
    peak = score != 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                peak &= key > pad[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
    xy, scores = [], []
    for cy in range(-(-h // cell)):
        for cx in range(-(-w // cell)):
            best, at = 0, None
            for y in range(cy * cell, min(h, (cy + 1) * cell)):
                for x in range(cx * cell, min(w, (cx + 1) * cell)):
                    if peak[y, x] and int(key[y, x]) > best:
                        best, at = int(key[y, x]), (x, y)
            if at is not None:
                xy.append(at)
                scores.append(best >> 32)
    return np.array(xy, np.int32).reshape(-1, 2), np.array(scores, np.int32)


def orientation(gray, x, y):
    """the bin 0 .. 31 of the intensity centroid over the disc of radius 13"""
    m10 = m01 = 0
    for dy in range(-13, 14):
        for dx in range(-13, 14):
            if dx * dx + dy * dy <= 169:
                v = int(gray[y + dy, x + dx])
                m10 += dx * v
                m01 += dy * v
    vals = [m10 * COS[k] + m01 * SIN[k] for k in range(32)]
    return vals.index(max(vals))  # the lowest of equals


def box_plane(gray):
    """B(p): the 5 x 5 sums, int32, valid 2 px inside the image (0 elsewhere)"""
    g = np.asarray(gray).astype(np.int32)
    h, w = g.shape
    B = np.zeros((h, w), np.int32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            B[2:h - 2, 2:w - 2] += g[2 + dy:h - 2 + dy, 2 + dx:w - 2 + dx]
    return B


def describe(gray, xy, seed=0):
    """(descriptors (n, 32) uint8, bins (n,) int32) of the keypoints xy of one gray image; a point nearer than BORDER to an
    edge gets zeros and -1"""
    gray = np.asarray(gray)
    h, w = gray.shape
    table = brief_pattern(seed).astype(np.int64)
    B = box_plane(gray) if h >= 5 and w >= 5 else None
    desc, bins = np.zeros((len(xy), 32), np.uint8), np.full(len(xy), -1, np.int32)
    for n, (x, y) in enumerate(np.asarray(xy).tolist()):
        if not (BORDER <= x < w - BORDER and BORDER <= y < h - BORDER):
            continue
        k = orientation(gray, x, y)
        t = table[k]
        bits = B[y + t[:, 1], x + t[:, 0]] < B[y + t[:, 3], x + t[:, 2]]
        desc[n] = np.packbits(bits.astype(np.uint8), bitorder="little")
        bins[n] = k
    return desc, bins


def detect_and_describe(img, threshold=20, cell=8, seed=0):
    """dict(xy, scores, descriptors, bins) of one image (colour through gray_of)"""
    gray = gray_of(img)
    xy, scores = keypoints(score_plane(gray, threshold), cell)
    desc, bins = describe(gray, xy, seed)
    return dict(xy=xy, scores=scores, descriptors=desc, bins=bins)


def distances(d1, d2):
    """(n1, n2) int32 Hamming distances"""
    d1, d2 = np.asarray(d1, np.uint8).reshape(-1, 32), np.asarray(d2, np.uint8).reshape(-1, 32)
    out = np.zeros((len(d1), len(d2)), np.int32)
    for b in range(32):
        out += POPCOUNT[d1[:, b, None] ^ d2[None, :, b]]
    return out


def search(d1, d2):
    """(best (n1,) int32, d_best, d_second): the train row of the smallest (distance, index) -- -1 and 257 without one --
    and the smallest distance among the other rows, 257 where there is none"""
    D = distances(d1, d2)
    n1, n2 = D.shape
    best, dbest, dsecond = np.full(n1, -1, np.int32), np.full(n1, 257, np.int32), np.full(n1, 257, np.int32)
    if n2:
        best = D.argmin(1).astype(np.int32)  # the first of equals
        dbest = D[np.arange(n1), best].astype(np.int32)
    if n2 > 1:
        E = D.copy()
        E[np.arange(n1), best] = 257
        dsecond = E.min(1).astype(np.int32)
    return best, dbest, dsecond


def match(d1, d2, max_distance=64, ratio=(4, 5), cross_check=True):
    """(matches (m, 2) int32, distances (m,) int32) in query order"""
    best, dbest, dsecond = search(d1, d2)
    back = search(d2, d1)[0]
    rows, dist = [], []
    for q in range(len(best)):
        if best[q] < 0 or dbest[q] > max_distance or int(dbest[q]) * ratio[1] > ratio[0] * int(dsecond[q]):
            continue
        if cross_check and back[best[q]] != q:
            continue
        rows.append((q, int(best[q])))
        dist.append(int(dbest[q]))
    return np.array(rows, np.int32).reshape(-1, 2), np.array(dist, np.int32)


def match_images(img1, img2, threshold=20, cell=8, seed=0, max_distance=64, ratio=(4, 5), cross_check=True):
    """(uvs1, uvs2 float64 (m, 2), distances) as features.match_images gives them"""
    a, b = detect_and_describe(img1, threshold, cell, seed), detect_and_describe(img2, threshold, cell, seed)
    m, d = match(a["descriptors"], b["descriptors"], max_distance, ratio, cross_check)
    return a["xy"][m[:, 0]].astype(np.float64), b["xy"][m[:, 1]].astype(np.float64), d
