"""NumPy restatement of the chessboard detector (csrc/chessboard.hip): response, peaks, lattice -- integers end to end,
so the kernels are pinned to it bit for bit (tests/test_gpu_chessboard.py) and it is pinned to rendered boards with
analytic corners (tests/test_chessboard_cpu.py).  The contract is this package's own, not cv2.findChessboardCorners'.
"""
import numpy as np

RING = ((5, 0), (5, 2), (4, 4), (2, 5), (0, 5), (-2, 5), (-4, 4), (-5, 2),
        (-5, 0), (-5, -2), (-4, -4), (-2, -5), (0, -5), (2, -5), (4, -4), (5, -2))  # (dx, dy) of I[0 .. 15]
BORDER = 5
CAPACITY = 1024
MAX_CORNERS, MAX_NMS_RADIUS, MAX_RELATIVE = 512, 8, 64
FOUND, FEW, OVERFLOW, INCOMPLETE = 0, 1, 2, 4  # status


def response(gray):
    """gray (f, h, w) or (h, w) uint8 -> (r int16 of the same shape, rmax int32 (f,) or a scalar): r = 5 sr - 5 dr -
    |5 ring - 16 local|, the ChESS response times 5; 0 within 5 px of a border."""
    g = np.asarray(gray)
    assert g.dtype == np.uint8 and g.ndim in (2, 3)
    one = g.ndim == 2
    g = (g[None] if one else g).astype(np.int32)
    f, h, w = g.shape
    r = np.zeros((f, h, w), np.int32)
    B = BORDER
    if h > 2 * B and w > 2 * B:
        def at(dx, dy):
            return g[:, B + dy:h - B + dy, B + dx:w - B + dx]
        ring = [at(dx, dy) for dx, dy in RING]
        sr = sum(np.abs(ring[n] + ring[n + 8] - ring[n + 4] - ring[n + 12]) for n in range(4))
        dr = sum(np.abs(ring[n] - ring[n + 8]) for n in range(8))
        total = sum(ring)
        local = at(0, 0) + at(1, 0) + at(-1, 0) + at(0, 1) + at(0, -1)
        r[:, B:h - B, B:w - B] = 5 * sr - 5 * dr - np.abs(5 * total - 16 * local)
    assert r.min() >= -30600 and r.max() <= 10200
    rmax = r.reshape(f, -1).max(1).astype(np.int32)
    r = r.astype(np.int16)
    return (r[0], rmax[0]) if one else (r, rmax)


def peak_mask(r, rmax, relative=8, nms_radius=3):
    """the candidates of response planes r (f, h, w) with their maxima rmax (f,): a bool mask"""
    r = np.asarray(r).astype(np.int32)
    f, h, w = r.shape
    R = int(nms_radius)
    on = (r > 0) & (relative * r >= np.asarray(rmax, np.int32).reshape(f, 1, 1))
    pad = np.full((f, h + 2 * R, w + 2 * R), -(1 << 20), np.int32)  # below every response: the window is clipped
    pad[:, R:R + h, R:R + w] = r
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dx == 0 and dy == 0:
                continue
            q = pad[:, R + dy:R + dy + h, R + dx:R + dx + w]
            on &= (r > q) if (dy < 0 or (dy == 0 and dx < 0)) else (r >= q)  # q of a lower pixel index: strictly above
    return on


def peaks(r, rmax, relative=8, nms_radius=3):
    """-> (list (f, CAPACITY, 2) int32 of (x, y) in pixel-index order, -1 beyond a frame's candidates; counts (f,)
    int32, in full whatever the capacity)"""
    on = peak_mask(r, rmax, relative, nms_radius)
    f = on.shape[0]
    out = np.full((f, CAPACITY, 2), -1, np.int32)
    counts = np.zeros(f, np.int32)
    for k in range(f):
        y, x = np.nonzero(on[k])  # (row-major: pixel-index order)
        counts[k] = len(x)
        m = min(len(x), CAPACITY)
        out[k, :m, 0], out[k, :m, 1] = x[:m], y[:m]
    return out, counts


def _nearest(P, q, free):
    """index of the candidate among ``free`` nearest q, the lowest index on a tie; its squared distance"""
    d = ((P - q) ** 2).sum(1)
    d = np.where(free, d, np.iinfo(np.int64).max)
    k = int(np.argmin(d))  # (the first of equal minima)
    return k, int(d[k])


def lattice_one(cand, w, across, down):
    """the candidates (m, 2) of one frame, m <= CAPACITY -> (corners (n, 2) int64 in the board's order or None, status)"""
    n = across * down
    P = np.asarray(cand, np.int64).reshape(-1, 2)
    m = len(P)
    if m < n:
        return None, FEW
    every = np.ones(m, bool)
    # 1: the seed, nearest the centroid
    s, _ = _nearest(m * P, P.sum(0), every)
    # 2, 3: its nearest neighbour, and the nearest at 30 degrees or more from that line
    others = every.copy()
    others[s] = False
    a, _ = _nearest(P, P[s], others)
    u = P[a] - P[s]
    d = P - P[s]
    cross = u[0] * d[:, 1] - u[1] * d[:, 0]
    wide = others & (4 * cross * cross >= (u * u).sum() * (d * d).sum(1))
    if not wide.any():
        return None, INCOMPLETE
    b, _ = _nearest(P, P[s], wide)
    v = P[b] - P[s]
    # 4: breadth first
    cell = {(0, 0): s}
    label = {s: (0, 0)}
    queue = [s]
    free = every.copy()
    free[s] = False
    head = 0
    while head < len(queue) and len(queue) <= n:
        p = queue[head]
        head += 1
        i, j = label[p]
        for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            if len(queue) > n:
                break
            if (i + di, j + dj) in cell:
                continue
            step = None
            if (i - di, j - dj) in cell:
                step = P[p] - P[cell[(i - di, j - dj)]]
            else:
                for o in (-1, 1):
                    oi, oj = (0, o) if di else (o, 0)
                    if (i + oi, j + oj) in cell and (i + oi + di, j + oj + dj) in cell:
                        step = P[cell[(i + oi + di, j + oj + dj)]] - P[cell[(i + oi, j + oj)]]
                        break
            if step is None:
                step = (u if di else v) * (di + dj)
            if not free.any():
                continue
            c, dist = _nearest(P, P[p] + step, free)
            if 4 * dist <= int((step * step).sum()):
                cell[(i + di, j + dj)] = c
                label[c] = (i + di, j + dj)
                free[c] = False
                queue.append(c)
    # 5: exactly the board
    if len(queue) != n:
        return None, INCOMPLETE
    ii = np.array([label[c][0] for c in queue])
    jj = np.array([label[c][1] for c in queue])
    ni, nj = ii.max() - ii.min() + 1, jj.max() - jj.min() + 1
    if (ni, nj) not in ((across, down), (down, across)):
        return None, INCOMPLETE
    G = np.zeros((ni, nj, 2), np.int64)
    G[ii - ii.min(), jj - jj.min()] = P[queue]  # (n distinct cells in a box of n: no hole)
    # 6: the board's order -- the right-handed labelings of its shape, corner 0 at the lowest pixel index
    best = None
    for swap in (0, 1):
        if (ni, nj) != ((down, across) if swap else (across, down)):
            continue
        for fi in (0, 1):
            for fj in (0, 1):
                A = G[::-1] if fi else G
                A = A[:, ::-1] if fj else A
                A = A if swap else A.transpose(1, 0, 2)  # -> (down, across, 2)
                sc = (A[:, -1] - A[:, 0]).sum(0)
                sr = (A[-1] - A[0]).sum(0)
                if sc[0] * sr[1] - sc[1] * sr[0] <= 0:
                    continue
                key = int(A[0, 0, 1]) * w + int(A[0, 0, 0])
                if best is None or key < best[0]:
                    best = (key, A.reshape(n, 2))
    if best is None:
        return None, INCOMPLETE
    return best[1], FOUND


def lattice(cands, counts, w, pattern):
    """-> (corners (f, n, 2) float32, NaN where not found; status (f,) int32)"""
    across, down = pattern
    n = across * down
    f = len(counts)
    corners = np.full((f, n, 2), np.nan, np.float32)
    status = np.zeros(f, np.int32)
    for k in range(f):
        if counts[k] > CAPACITY:
            status[k] = OVERFLOW
            continue
        got, status[k] = lattice_one(cands[k, :counts[k]], w, across, down)
        if got is not None:
            corners[k] = got
    return corners, status


def check_arguments(pattern, relative, nms_radius):
    across, down = pattern
    if any(int(v) != v for v in (across, down, relative, nms_radius)):
        raise ValueError("integers")
    if across < 2 or down < 2 or across * down > MAX_CORNERS:
        raise ValueError("pattern")
    if not 1 <= relative <= MAX_RELATIVE or not 1 <= nms_radius <= MAX_NMS_RADIUS:
        raise ValueError("relative / nms_radius")


def find(gray, pattern, relative=8, nms_radius=3):
    """all three stages on gray (f, h, w): dict(response, rmax, peaks, counts, corners, status, found)"""
    check_arguments(pattern, relative, nms_radius)
    g = np.asarray(gray)
    g = g[None] if g.ndim == 2 else g
    r, rmax = response(g)
    cand, counts = peaks(r, rmax, relative, nms_radius)
    corners, status = lattice(cand, counts, g.shape[2], pattern)
    return dict(response=r, rmax=rmax, peaks=cand, counts=counts, corners=corners, status=status, found=status == 0)
