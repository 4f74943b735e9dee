"""NumPy restatement of the one-pass detector of several ChArUco boards (csrc/charuco.hip, k_charuco_multi) and of the
Laplacian's sums (csrc/sharpness.hip) -- integers end to end, so the kernels are pinned to it bit for bit
(tests/test_gpu_multiboard.py) and it is pinned to rendered scenes with analytic corners (tests/test_multiboard_cpu.py).
The lattice, the decode and the numbering are tests/charuco_ref.py's, by import; what is stated here is what several boards
add: which seed cell qualifies, which peaks a lattice may take, who votes, when the loop ends and the status per board.
With one board every rule is ``charuco_ref.detect_one``'s.
"""
import numpy as np

import charuco_ref as cref
import chessboard_ref

from charuco_ref import FEW, FOUND, NO_CONSENSUS, NO_LATTICE, OVERFLOW  # noqa: F401

MAX_BOARDS = 8


def board_of(mid, first_ids, sx, sy):
    """(board, square) of the board of the set whose id range holds marker ``mid``, or None"""
    for b, first in enumerate(first_ids):
        square = cref.marker_square(mid - first, sx, sy)
        if square is not None:
            return b, square
    return None


def detect_one(cand, gray, squares, dictionary, s, first_ids, ratio=(1, 2), min_markers=2, max_errors=0):
    """the candidates (m, 2) of one frame, m <= CAPACITY -> (corners (B, n, 2) float32 with NaN, marker_ids (B, sx * sy),
    status (B,))"""
    sx, sy = squares
    nb, n = len(first_ids), (sx - 1) * (sy - 1)
    corners = np.full((nb, n, 2), np.nan, np.float32)
    marker_ids = np.full((nb, sx * sy), -1, np.int32)
    P = np.asarray(cand, np.int64).reshape(-1, 2)
    m = len(P)
    if m < cref.MIN_PEAKS:
        return corners, marker_ids, np.full(nb, FEW, np.int32)
    cd = ((m * P - P.sum(0)) ** 2).sum(1)
    dead = np.zeros(m, bool)    # labelled in some lattice, accepted or not: seeds no more
    taken = np.zeros(m, bool)   # labelled in an accepted lattice: labelled no more
    found, tried = [False] * nb, [False] * nb
    seed_after, grown = -1, 0
    seed_board = [None]

    def open_board(got):
        """(board, square) of a decoded marker (id, turn) where its board is of the set and not yet found, else None"""
        hit = None if got is None else board_of(got[0], first_ids, sx, sy)
        return None if hit is None or found[hit[0]] else hit

    def verify(c00, c10, c01, c11):
        hit = open_board(cref.decode(gray, [P[c00], P[c10], P[c01], P[c11]], s, ratio[0], ratio[1], dictionary, max_errors))
        seed_board[0] = None if hit is None else hit[0]
        return hit is not None
    for _ in range(cref.SEED_SCAN * nb):
        if all(found):
            break
        key = cref._least_key(cd, np.ones(m, bool), seed_after)
        if key is None:
            break
        seed_after, seed = key, key & 1023
        if dead[seed]:
            continue
        basis = cref.find_basis(P, seed, verify)
        if basis is None:
            continue
        grown += 1
        used = taken.copy()
        queue, grid = cref.grow(P, used, seed, *basis)
        votes = []
        for c00, i, j in queue:
            rest = [grid.get(k) for k in ((i + 1, j), (i, j + 1), (i + 1, j + 1))]
            if any(r is None for r in rest):
                continue
            got = cref.decode(gray, [P[c00]] + [P[r] for r in rest], s, ratio[0], ratio[1], dictionary, max_errors)
            hit = open_board(got)
            if hit is None:
                continue
            b, square = hit
            ox, oy = cref.offset(got[1], square[0], square[1], i, j)
            votes.append((b << 14 | got[1] << 12 | (ox + 32) << 6 | (oy + 32), got[0], square))
        dead |= used
        if votes:
            keys = [v[0] for v in votes]
            agree, neg = max((keys.count(k), -k) for k in keys)
            if agree >= min_markers and len(votes) - agree <= agree:
                key = -neg
                b, turn, ox, oy = key >> 14, (key >> 12) & 3, ((key >> 6) & 63) - 32, (key & 63) - 32
                for c, i, j in queue:
                    cx, cy = cref.board_corner(turn, ox, oy, i, j)
                    if 1 <= cx <= sx - 1 and 1 <= cy <= sy - 1:
                        corners[b, (cy - 1) * (sx - 1) + cx - 1] = P[c]
                for k, mid, (qx, qy) in votes:
                    if k == key:
                        marker_ids[b, qy * sx + qx] = mid
                found[b] = True
                taken = used
                continue
        tried[seed_board[0]] = True
        if grown == cref.SEED_TRIES * nb:
            break
    status = [FOUND if found[b] else NO_CONSENSUS if tried[b] else NO_LATTICE for b in range(nb)]
    return corners, marker_ids, np.array(status, np.int32)


def check_arguments(squares, dictionary, first_ids, ratio, relative, nms_radius, min_markers, max_errors=0):
    ids = list(first_ids)
    if not 1 <= len(ids) <= MAX_BOARDS:
        raise ValueError("boards")
    markers = squares[0] * squares[1] // 2
    for k, a in enumerate(ids):
        cref.check_arguments(squares, dictionary, ratio, a, relative, nms_radius, min_markers, max_errors)
        if any(a < b + markers and b < a + markers for b in ids[:k]):
            raise ValueError("id ranges overlap")


def find(gray, squares, dictionary, first_ids, ratio=(1, 2), relative=8, nms_radius=3, min_markers=2, max_errors=0):
    """every stage on gray (f, h, w): dict(peaks, counts, corners (f, B, n, 2), marker_ids (f, B, sx * sy), status (f, B),
    seen (f, B, n))"""
    check_arguments(squares, dictionary, first_ids, ratio, relative, nms_radius, min_markers, max_errors)
    g = np.asarray(gray)
    g = g[None] if g.ndim == 2 else g
    r, rmax = chessboard_ref.response(g)
    cand, counts = chessboard_ref.peaks(r, rmax, relative, nms_radius)
    sx, sy = squares
    f, nb = len(g), len(first_ids)
    corners = np.full((f, nb, (sx - 1) * (sy - 1), 2), np.nan, np.float32)
    marker_ids = np.full((f, nb, sx * sy), -1, np.int32)
    status = np.zeros((f, nb), np.int32)
    dw = cref.words(dictionary)
    for k in range(f):
        if counts[k] > cref.CAPACITY:
            status[k] = OVERFLOW
            continue
        corners[k], marker_ids[k], status[k] = detect_one(cand[k, :counts[k]], g[k], squares, dw, np.shape(dictionary)[1],
                                                          list(first_ids), ratio, min_markers, max_errors)
    return dict(peaks=cand, counts=counts, corners=corners, marker_ids=marker_ids, status=status, seen=~np.isnan(corners[..., 0]))


def laplacian_sums(gray):
    """(S1, S2) as Python integers: the sums over an image (h, w) uint8, h, w >= 2, of L = g(x-1, y) + g(x+1, y) + g(x, y-1) +
    g(x, y+1) - 4 g(x, y) and of L^2, a neighbour outside the image mirrored about the border pixel (reflect-101)"""
    g = np.asarray(gray)
    if g.ndim != 2 or min(g.shape) < 2 or g.dtype != np.uint8:
        raise ValueError("gray must be (h, w) uint8 with sides from 2, got %s %s" % (g.dtype, g.shape))
    p = np.pad(g.astype(np.int64), 1, mode="reflect")
    lap = p[1:-1, :-2] + p[1:-1, 2:] + p[:-2, 1:-1] + p[2:, 1:-1] - 4 * p[1:-1, 1:-1]
    return int(lap.sum()), int((lap * lap).sum())


def laplacian(gray):
    """the Laplacian itself, float64, for np.var"""
    p = np.pad(np.asarray(gray).astype(np.float64), 1, mode="reflect")
    return p[1:-1, :-2] + p[1:-1, 2:] + p[:-2, 1:-1] + p[2:, 1:-1] - 4 * p[1:-1, 1:-1]
