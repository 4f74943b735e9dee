"""NumPy restatement of the ChArUco stages (csrc/charuco.hip): partial lattice, marker decode, vote and numbering --
integers end to end, so the kernel is pinned to it bit for bit (tests/test_gpu_charuco.py) and it is pinned to rendered
boards with analytic corners (tests/test_charuco_cpu.py).  Stages 1 and 2 are tests/chessboard_ref.py's ``response``
and ``peaks``.  The contract is this package's own, not cv2.aruco's.
"""
import numpy as np

import chessboard_ref as cref

CAPACITY = cref.CAPACITY
MAX_SQUARES, MIN_SQUARES = 16, 3      # of a board, each way
RANGE = 15                            # lattice labels run -15 .. 15 about the seed
MAX_LABELS = 320                      # corners one lattice holds
SEED_SCAN, SEED_TRIES, NEIGHBOURS = 32, 4, 16
MIN_CONTRAST = 40                     # gray levels between a marker's darkest and brightest cell
MAX_RATIO_DEN, MAX_IDS = 64, 1024
FOUND, FEW, OVERFLOW, NO_LATTICE, NO_CONSENSUS = 0, 1, 2, 4, 8  # status
MIN_PEAKS = 5
NONE = -1


def words(bits):
    """(n_ids, s, s) bits -> python ints, bit (r, c) of weight 2^(s*s - 1 - (r*s + c))"""
    b = np.asarray(bits)
    return [int("".join(str(int(v)) for v in m.ravel()), 2) for m in b]


def marker_square(rank, sx, sy):
    """the square (x, y) of the marker of that rank in row-major order of the squares with x % 2 != y % 2, or None"""
    if rank < 0:
        return None
    pair, rem = divmod(rank, sx)
    x, y = (2 * rem + 1, 2 * pair) if rem < sx // 2 else (2 * (rem - sx // 2), 2 * pair + 1)
    return (x, y) if y < sy else None


def _least_key(d, take, after=-1):
    """the least distance << 10 | index above ``after`` among the candidates ``take``, or None"""
    key = (d.astype(np.int64) << 10) | np.arange(len(d))
    key = key[take & (key > after)]
    return int(key.min()) if len(key) else None


def _dist(P, q):
    return ((P - np.asarray(q, np.int64)) ** 2).sum(1)


def find_basis(P, s, verify):
    """the two steps (u, v) of a seed: u to one of its 16 nearest neighbours, v to one of the 16 nearest at 30
    degrees or more from the line of u, ordered so that cross(u, v) > 0 -- the first pair whose fourth corner s + u + v
    is present within a quarter of the shorter step and whose cell ``verify(c00, c10, c01, c11)`` holds a marker of the
    board.  None where there is no such pair."""
    m = len(P)
    idx = np.arange(m)
    ds = _dist(P, P[s])
    others = idx != s
    a_after = -1
    for _ in range(NEIGHBOURS):
        ka = _least_key(ds, others, a_after)
        if ka is None:
            break
        a_after, a = ka, ka & 1023
        u = P[a] - P[s]
        uu = int(u @ u)
        d = P - P[s]
        cr = u[0] * d[:, 1] - u[1] * d[:, 0]
        wide = others & (4 * cr * cr >= uu * ds)
        b_after = -1
        for _ in range(NEIGHBOURS):
            kb = _least_key(ds, wide, b_after)
            if kb is None:
                break
            b_after, b = kb, kb & 1023
            v = P[b] - P[s]
            vv = int(v @ v)
            kc = _least_key(_dist(P, P[s] + u + v), others & (idx != a) & (idx != b))
            if kc is None or 16 * (kc >> 10) > min(uu, vv):
                continue
            flip = u[0] * v[1] - u[1] * v[0] < 0
            if verify(s, b if flip else a, a if flip else b, kc & 1023):
                return (v, u) if flip else (u, v)
    return None


def grow(P, used, s, u, v):
    """breadth first from the seed, cell (0, 0): -> (queue [(candidate, i, j)], grid {(i, j): candidate}); marks ``used``"""
    grid = {(0, 0): s}
    queue = [(s, 0, 0)]
    used[s] = True
    head = 0
    while head < len(queue) and len(queue) < MAX_LABELS:
        p, i, j = queue[head]
        head += 1
        for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            if len(queue) >= MAX_LABELS:
                break
            if abs(i + di) > RANGE or abs(j + dj) > RANGE or (i + di, j + dj) in grid:
                continue
            step = (u if di else v) * (di + dj)
            if (i - di, j - dj) in grid:
                step = P[p] - P[grid[(i - di, j - dj)]]
            else:
                for o in (-1, 1):
                    oi, oj = (0, o) if di else (o, 0)
                    if (i + oi, j + oj) in grid and (i + oi + di, j + oj + dj) in grid:
                        step = P[grid[(i + oi + di, j + oj + dj)]] - P[grid[(i + oi, j + oj)]]
                        break
            key = _least_key(_dist(P, P[p] + step), ~used)
            if key is not None and 64 * (key >> 10) <= int(step @ step):  # within an eighth of the step
                c = key & 1023
                grid[(i + di, j + dj)] = c
                used[c] = True
                queue.append((c, i + di, j + dj))
    return queue, grid


def sample_weights(s, num, den):
    """(D, A): the centre of bit cell a of the s + 2 across a marker lies A[a] / D of the way across its square"""
    c = s + 2
    return 2 * den * c, [den * c + num * (2 * a + 1 - c) for a in range(c)]


def decode(gray, quad, s, num, den, dictionary, max_errors=0):
    """the marker in the lattice cell with corners quad = (P00, P10, P01, P11) -> (id, turn) or None"""
    h, w = gray.shape
    c = s + 2
    D, A = sample_weights(s, num, den)
    p00, p10, p01, p11 = (np.asarray(p, np.int64) for p in quad)
    val = np.zeros((c, c), np.int64)
    for b in range(c):
        for a in range(c):
            wx, wy = A[a], A[b]
            n = (D - wx) * (D - wy) * p00 + wx * (D - wy) * p10 + (D - wx) * wy * p01 + wx * wy * p11
            px, py = (n + D * D // 2) // (D * D)
            px, py = min(max(int(px), 1), w - 2), min(max(int(py), 1), h - 2)
            val[b, a] = int(gray[py - 1:py + 2, px - 1:px + 2].astype(np.int64).sum())
    lo, hi = int(val.min()), int(val.max())
    if hi - lo < 9 * MIN_CONTRAST:
        return None
    bits = (2 * val > lo + hi).astype(np.uint8)
    if bits[0].any() or bits[-1].any() or bits[:, 0].any() or bits[:, -1].any():
        return None
    best = None
    for k in range(4):
        word = int("".join(str(int(x)) for x in np.rot90(bits[1:-1, 1:-1], k).ravel()), 2)
        for i, dw in enumerate(dictionary):
            err = bin(word ^ dw).count("1")
            if err <= max_errors:
                key = err << 16 | i << 2 | k
                best = key if best is None or key < best else best
    return None if best is None else ((best >> 2) & 0x3fff, best & 3)


def board_corner(turn, ox, oy, i, j):
    """the board corner (cx, cy) of lattice corner (i, j): corner (cx, cy) is the top-left one of square (cx, cy)"""
    x, y = ((i, j), (j, -i), (-i, -j), (-j, i))[turn]
    return x + ox, y + oy


def offset(turn, qx, qy, i, j):
    """the offset under which the lattice cell whose least corner is (i, j) is board square (qx, qy)"""
    return ((qx - i, qy - j), (qx - j, qy + i + 1), (qx + i + 1, qy + j + 1), (qx + j + 1, qy - i))[turn]


def detect_one(cand, gray, squares, dictionary, s, ratio=(1, 2), first_id=0, min_markers=2, max_errors=0):
    """the candidates (m, 2) of one frame, m <= CAPACITY -> (corners (n, 2) float32 with NaN, marker_ids (sx * sy,), status)"""
    sx, sy = squares
    n = (sx - 1) * (sy - 1)
    corners = np.full((n, 2), np.nan, np.float32)
    marker_ids = np.full(sx * sy, -1, np.int32)
    P = np.asarray(cand, np.int64).reshape(-1, 2)
    m = len(P)
    if m < MIN_PEAKS:
        return corners, marker_ids, FEW
    cd = ((m * P - P.sum(0)) ** 2).sum(1)
    dead = np.zeros(m, bool)
    every = np.ones(m, bool)
    seed_after, grown = -1, 0

    def verify(c00, c10, c01, c11):
        got = decode(gray, [P[c00], P[c10], P[c01], P[c11]], s, ratio[0], ratio[1], dictionary, max_errors)
        return got is not None and marker_square(got[0] - first_id, sx, sy) is not None
    for _ in range(SEED_SCAN):
        key = _least_key(cd, every, seed_after)
        if key is None:
            break
        seed_after, seed = key, key & 1023
        if dead[seed]:
            continue
        basis = find_basis(P, seed, verify)
        if basis is None:
            continue
        grown += 1
        used = np.zeros(m, bool)
        queue, grid = grow(P, used, seed, *basis)
        votes = []
        for c00, i, j in queue:
            rest = [grid.get(k) for k in ((i + 1, j), (i, j + 1), (i + 1, j + 1))]
            if any(r is None for r in rest):
                continue
            got = decode(gray, [P[c00]] + [P[r] for r in rest], s, ratio[0], ratio[1], dictionary, max_errors)
            if got is None:
                continue
            square = marker_square(got[0] - first_id, sx, sy)
            if square is None:
                continue
            ox, oy = offset(got[1], square[0], square[1], i, j)
            votes.append((got[1] << 12 | (ox + 32) << 6 | (oy + 32), got[0], square))
        if votes:
            keys = [v[0] for v in votes]
            agree, neg = max((keys.count(k), -k) for k in keys)
            if agree >= min_markers and len(votes) - agree <= agree:
                key = -neg
                turn, ox, oy = key >> 12, ((key >> 6) & 63) - 32, (key & 63) - 32
                for c, i, j in queue:
                    cx, cy = board_corner(turn, ox, oy, i, j)
                    if 1 <= cx <= sx - 1 and 1 <= cy <= sy - 1:
                        corners[(cy - 1) * (sx - 1) + cx - 1] = P[c]
                for k, mid, (qx, qy) in votes:
                    if k == key:
                        marker_ids[qy * sx + qx] = mid
                return corners, marker_ids, FOUND
        dead |= used
        if grown == SEED_TRIES:
            break
    return corners, marker_ids, NO_CONSENSUS if grown else NO_LATTICE


def check_arguments(squares, dictionary, ratio, first_id, relative, nms_radius, min_markers, max_errors=0):
    sx, sy = squares
    d = np.asarray(dictionary)
    if any(int(v) != v for v in (sx, sy, ratio[0], ratio[1], first_id, relative, nms_radius, min_markers, max_errors)):
        raise ValueError("integers")
    if not (MIN_SQUARES <= sx <= MAX_SQUARES and MIN_SQUARES <= sy <= MAX_SQUARES):
        raise ValueError("squares")
    if d.ndim != 3 or d.shape[1] != d.shape[2] or not 4 <= d.shape[1] <= 7 or not 1 <= len(d) <= MAX_IDS:
        raise ValueError("dictionary")
    if not 0 < ratio[0] < ratio[1] <= MAX_RATIO_DEN:
        raise ValueError("ratio")
    if first_id < 0 or first_id + (sx * sy) // 2 > len(d):
        raise ValueError("first_id")
    if min_markers < 1 or not 0 <= max_errors <= d.shape[1] ** 2:
        raise ValueError("min_markers / max_errors")
    cref.check_arguments((2, 2), relative, nms_radius)


def find(gray, squares, dictionary, ratio=(1, 2), first_id=0, relative=8, nms_radius=3, min_markers=2, max_errors=0):
    """every stage on gray (f, h, w): dict(peaks, counts, corners, marker_ids, status, found)"""
    check_arguments(squares, dictionary, ratio, first_id, relative, nms_radius, min_markers, max_errors)
    g = np.asarray(gray)
    g = g[None] if g.ndim == 2 else g
    r, rmax = cref.response(g)
    cand, counts = cref.peaks(r, rmax, relative, nms_radius)
    sx, sy = squares
    f = len(g)
    corners = np.full((f, (sx - 1) * (sy - 1), 2), np.nan, np.float32)
    marker_ids = np.full((f, sx * sy), -1, np.int32)
    status = np.zeros(f, np.int32)
    dw = words(dictionary)
    for k in range(f):
        if counts[k] > CAPACITY:
            status[k] = OVERFLOW
            continue
        corners[k], marker_ids[k], status[k] = detect_one(cand[k, :counts[k]], g[k], squares, dw, np.shape(dictionary)[1], ratio,
                                                          first_id, min_markers, max_errors)
    return dict(peaks=cand, counts=counts, corners=corners, marker_ids=marker_ids, status=status, found=status == 0)
