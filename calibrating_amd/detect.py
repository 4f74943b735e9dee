"""The detectors that work from uint8 frames alone (host side: torch tensors in HBM): corners refined to sub-pixel,
chessboard and ChArUco corners, stand-alone markers, sharpness.  Frames come in and results go out through ``_frames``;
``imgproc`` re-exports the public names, so ``imgproc.find_markers(...)`` and its like keep their spelling."""
import ctypes

import numpy as np

from . import _native
from ._arrays import FLOAT_TYPES, check_array, dtype_name, is_np, to_caller, to_device
from ._frames import device_frames, gray_frames, integer, layout, to_result
from ._native import call

# ---- corners refined to sub-pixel (boards.py:156-172; csrc/subpix.hip) ----
SUBPIX_SINGULAR, SUBPIX_LEFT_IMAGE, SUBPIX_REVERTED, SUBPIX_BAD_START = 1, 2, 4, 8  # bits of corner_sub_pix's status
SUBPIX_MAX_ITERATIONS = 100
TERM_CRITERIA_COUNT, TERM_CRITERIA_EPS = 1, 2  # cv2.TERM_CRITERIA_MAX_ITER, cv2.TERM_CRITERIA_EPS


def sub_pix_mask(win, zero_zone=(-1, -1)):
    """cornerSubPix's window weights, (2 win_h + 1, 2 win_w + 1) float32, made on the host: row i, column j holds
    (float)(vy * exp(-x^2)) with y = (float)(i - win_h) / win_h, vy = exp(-y^2) and x alike, all float32 (each exp is
    the float64 one rounded to float32: a correctly rounded expf); zero over the zero zone when ``zero_zone >= 0`` and
    ``2 zero_zone + 1 < 2 win + 1`` on both axes."""
    ww, wh = int(win[0]), int(win[1])
    if ww <= 0 or wh <= 0:
        raise ValueError("win must be a pair of positive half-sizes, got %r" % (win,))

    def axis(n):
        v = (np.arange(2 * n + 1) - n).astype(np.float32) / np.float32(n)
        return np.exp(-(v * v).astype(np.float64)).astype(np.float32)
    mask = (axis(wh)[:, None] * axis(ww)[None, :]).astype(np.float32)
    zx, zy = int(zero_zone[0]), int(zero_zone[1])
    if zx >= 0 and zy >= 0 and 2 * zx + 1 < 2 * ww + 1 and 2 * zy + 1 < 2 * wh + 1:
        mask[wh - zy:wh + zy + 1, ww - zx:ww + zx + 1] = 0
    return mask


_MASKS = {}  # (win, zero_zone, device) -> the mask on that device: a tracking loop uploads it once, not once per frame


def _device_mask(win, zero_zone, device):
    import torch
    key = (win, zero_zone, str(device))
    if key not in _MASKS:
        if len(_MASKS) >= 64:  # (a caller that sweeps windows: start again rather than grow)
            _MASKS.clear()
        _MASKS[key] = torch.from_numpy(sub_pix_mask(win, zero_zone)).to(device)
    return _MASKS[key]


def sub_pix_criteria(criteria):
    """(max_iters, squared eps) of cornerSubPix's termination criteria: ``(count, eps)`` -- either may be None -- or cv2's
    ``(type, count, eps)``.  max_iters = clamp(count, 1, 100) when a count is carried, else 100; eps = max(eps, 0)^2 when
    an epsilon is carried, else 0."""
    c = tuple(criteria)
    if len(c) == 3:
        kind = int(c[0])
        if kind & ~(TERM_CRITERIA_COUNT | TERM_CRITERIA_EPS) or not kind:
            raise ValueError("criteria type must be TERM_CRITERIA_COUNT (1), TERM_CRITERIA_EPS (2) or both, got %r" % (c[0],))
        count = c[1] if kind & TERM_CRITERIA_COUNT else None
        eps = c[2] if kind & TERM_CRITERIA_EPS else None
    elif len(c) == 2:
        count, eps = c
    else:
        raise ValueError("criteria must be (count, eps) or cv2's (type, count, eps), got %r" % (criteria,))
    max_iters = SUBPIX_MAX_ITERATIONS if count is None else min(max(int(count), 1), SUBPIX_MAX_ITERATIONS)
    eps = 0.0 if eps is None else max(float(eps), 0.0)
    if eps != eps:
        raise ValueError("criteria: eps is NaN")
    return max_iters, eps * eps


def _corner_layout(corners, counts, frames):
    """the lengths of ragged rows, or None for a dense batch; corners that do not fit ``frames`` images are refused"""
    shape = tuple(corners.shape)
    if counts is not None:
        lengths = np.asarray(counts)
        if corners.ndim != 2 or shape[1] != 2:
            raise ValueError("with counts, corners are ragged rows (N, 2), got %s" % (shape,))
        if lengths.ndim != 1 or lengths.dtype.kind not in "iu" or (lengths < 0).any() or len(lengths) != frames:
            raise ValueError("counts must be %d non-negative integers, one per image" % frames)
        if int(lengths.sum()) != shape[0]:
            raise ValueError("counts sum to %d rows, corners have %d" % (lengths.sum(), shape[0]))
        return lengths.astype(np.int64)
    if corners.ndim == 3 and shape[2] == 2 and shape[0] == frames and (frames > 1 or shape[1] != 1):
        pass  # (f, n, 2); with one image, (n, 1, 2) is cv2's layout of n corners
    elif corners.ndim == 2 and shape[1] == 2 or corners.ndim == 3 and shape[1:] == (1, 2):
        if frames != 1:
            raise ValueError("corners %s are one frame's; %d images need (f, n, 2) or counts" % (shape, frames))
    elif corners.ndim == 3 and shape[2] == 2:
        raise ValueError("corners %s do not match %d image(s)" % (shape, frames))
    else:
        raise ValueError("corners must be (n, 2), (n, 1, 2), (f, n, 2) or ragged (N, 2) with counts, got %s" % (shape,))
    return None


def corner_sub_pix(images, corners, win=(4, 4), zero_zone=(-1, -1), criteria=(30, 0.01), counts=None, return_info=False):
    """cv2.cornerSubPix(gray, corners, win, zero_zone, criteria) for every corner of every frame in one launch
    (boards.py:163-169; UNPINNED against cv2) -> the refined corners, in the shape and type
    they came in; they are not changed in place.

    ``images``: uint8 gray (h, w) / (f, h, w), or colour (h, w, 3) / (f, h, w, 3), which goes through
    ``cvt_gray(code="bgr")`` first.  ``corners``: float32 or float64, (n, 2) or cv2's (n, 1, 2) for one image,
    (f, n, 2) for f, or ragged rows (N, 2) with ``counts`` (f lengths; a frame may have none).  NumPy in -> NumPy out; CUDA
    tensors stay on their device and the current stream.  ``criteria``: ``(count, eps)`` or cv2's ``(type, count, eps)``
    (``sub_pix_criteria``).  ``return_info``: ``(corners, iterations, status)``, int32 per corner in the corners' leading
    shape; status bits: 1 singular window, 2 the iterate left the image, 4 it drifted further than the window and the
    start is returned, 8 the start is not finite or not inside the image and is returned as it came (cv2 asserts)."""
    import torch
    check_array(images, "images")
    if dtype_name(images) != "uint8":  # (before the corners are looked at, as ever; ``layout`` below has the rest)
        raise ValueError("images must be uint8, got %s" % images.dtype)
    check_array(corners, "corners")
    if is_np(images) != is_np(corners):
        raise TypeError("images and corners must both be NumPy arrays or both be CUDA tensors")
    if dtype_name(corners) not in FLOAT_TYPES:
        raise ValueError("corners must be float32 or float64, got %s" % corners.dtype)
    lay = layout(images, "images")
    lengths = _corner_layout(corners, counts, lay.f)
    ww, wh = int(win[0]), int(win[1])
    zone = (int(zero_zone[0]), int(zero_zone[1]))
    if ww <= 0 or wh <= 0:
        raise ValueError("win must be a pair of positive half-sizes, got %r" % (win,))
    max_iters, eps = sub_pix_criteria(criteria)
    if lay.w < 2 * ww + 5 or lay.h < 2 * wh + 5:
        raise ValueError("a %d x %d image is smaller than the %d x %d a window of %r needs" % (lay.w, lay.h, 2 * ww + 5, 2 * wh + 5, (ww, wh)))
    fr = device_frames(images, lay, "bgr")
    dev = fr.data.device
    rows = to_device(corners, device=dev).reshape(-1, 2)
    n = int(rows.shape[0])
    out = torch.empty_like(rows)
    iterations = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    start = None
    if lengths is not None:
        start = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)
    mask_t = _device_mask((ww, wh), zone, dev)
    call("camd_corner_sub_pix", dev, fr.data.data_ptr(), fr.w, fr.h, fr.pitch, fr.stride, fr.f, rows.data_ptr(),
         FLOAT_TYPES[dtype_name(rows)], n, None if start is None else start.data_ptr(), ww, wh, mask_t.data_ptr(), max_iters,
         ctypes.c_double(eps), out.data_ptr(), iterations.data_ptr(), status.data_ptr(), what="corner_sub_pix")
    lead = tuple(corners.shape[:-1])
    out = out.reshape(tuple(corners.shape))
    if not return_info:
        return to_caller(out, fr.was_np)
    return to_caller((out, iterations.reshape(lead), status.reshape(lead)), fr.was_np)


# ---- chessboard corners from the image alone (csrc/chessboard.hip; a contract of our own) ----
CHESS_CAPACITY, CHESS_MAX_CORNERS, CHESS_MAX_RELATIVE, CHESS_MAX_NMS_RADIUS, CHESS_MAX_SIDE = 1024, 512, 64, 8, 16384
CHESS_FEW, CHESS_OVERFLOW, CHESS_INCOMPLETE = 1, 2, 4  # find_chessboard_corners' status; 0 = found


def chess_arguments(pattern, relative, nms_radius):
    """(across, down, relative, nms_radius) as integers within the detector's limits, or ValueError"""
    try:
        across, down = pattern
    except (TypeError, ValueError):
        raise ValueError("pattern must be the inner corners (across, down), got %r" % (pattern,))
    across, down = integer(across, "across"), integer(down, "down")
    relative, nms_radius = integer(relative, "relative"), integer(nms_radius, "nms_radius")
    if across < 2 or down < 2 or across * down > CHESS_MAX_CORNERS:
        raise ValueError("a pattern of %d x %d corners; the detector takes across, down >= 2 with at most %d corners" % (across, down, CHESS_MAX_CORNERS))
    if not 1 <= relative <= CHESS_MAX_RELATIVE:
        raise ValueError("relative must be 1 .. %d, got %d" % (CHESS_MAX_RELATIVE, relative))
    if not 1 <= nms_radius <= CHESS_MAX_NMS_RADIUS:
        raise ValueError("nms_radius must be 1 .. %d, got %d" % (CHESS_MAX_NMS_RADIUS, nms_radius))
    return across, down, relative, nms_radius


def _chess_response(fr):
    import torch
    dev = fr.data.device
    r = torch.empty((fr.f, fr.h, fr.w), dtype=torch.int16, device=dev)
    rmax = torch.empty(fr.f, dtype=torch.int32, device=dev)
    call("camd_chess_response", dev, fr.data.data_ptr(), fr.w, fr.h, fr.pitch, fr.stride, fr.f, r.data_ptr(), rmax.data_ptr(),
         what="chess_response")
    return r, rmax


def chess_response(images):
    """Stage 1 of the chessboard detector: the ChESS corner response (Bennett & Lasenby) times 5 of every pixel, in
    integers -- ``include/calibrating_amd.h`` states the formula -- -> ``(response, response_max)``: int16 in the shape of
    the gray image(s), 0 within 5 px of a border, and its maximum per frame, int32 (f,) (0-d for one image).  ``images``:
    uint8 gray (h, w) / (f, h, w) or colour (h, w, 3) / (f, h, w, 3) (through ``cvt_gray``), NumPy or CUDA; pitched views
    are read in place."""
    fr = gray_frames(images)
    return to_result(_chess_response(fr), fr.batched, fr.was_np)


def _chess_peaks(r, rmax, relative, nms_radius):
    import torch
    f, h, w = (int(v) for v in r.shape)
    peaks = torch.full((f, CHESS_CAPACITY, 2), -1, dtype=torch.int32, device=r.device)
    counts = torch.empty(f, dtype=torch.int32, device=r.device)
    ws = torch.empty(_native.lib().camd_chess_peaks_workspace_bytes(h, f), dtype=torch.uint8, device=r.device)
    call("camd_chess_peaks", r.device, r.data_ptr(), rmax.data_ptr(), w, h, f, relative, nms_radius, ws.data_ptr(),
         peaks.data_ptr(), counts.data_ptr(), what="chess_peaks")
    return peaks, counts


def chess_peaks(response, response_max, relative=8, nms_radius=3):
    """Stage 2: the candidates of response planes (f, h, w) int16 with their maxima (f,) int32 -- positive, at least
    1 / ``relative`` of the frame's maximum, and the peak of their (2 nms_radius + 1)^2 window (of equal responses the
    first in pixel order) -> ``(peaks, counts)``: int32 (f, 1024, 2) of (x, y) in pixel order, -1 beyond a frame's
    candidates, and every frame's count in full, int32 (f,)."""
    _, _, relative, nms_radius = chess_arguments((2, 2), relative, nms_radius)
    check_array(response, "response")
    check_array(response_max, "response_max")
    if is_np(response) != is_np(response_max):
        raise TypeError("response and response_max must both be NumPy arrays or both be CUDA tensors")
    if dtype_name(response) != "int16" or dtype_name(response_max) != "int32":
        raise ValueError("response must be int16 and response_max int32, got %s and %s" % (response.dtype, response_max.dtype))
    if response.ndim != 3 or 0 in tuple(response.shape) or tuple(response_max.shape) != (response.shape[0],):
        raise ValueError("response must be (f, h, w) and response_max (f,), got %s and %s" % (tuple(response.shape), tuple(response_max.shape)))
    if response.shape[0] * response.shape[1] >= 2 ** 31:
        raise ValueError("response: %d rows in all, the kernels take fewer than 2^31" % (response.shape[0] * response.shape[1]))
    r = to_device(response)
    return to_caller(_chess_peaks(r, to_device(response_max, device=r.device), relative, nms_radius), is_np(response))


def _candidates(images, relative, nms_radius, min_side=None, words=None):
    """what the chessboard and ChArUco calls start with: (gray frames, peaks, counts, the words on their device or None)"""
    import torch
    fr = gray_frames(images, max_side=CHESS_MAX_SIDE, min_side=min_side)
    peaks, counts = _chess_peaks(*_chess_response(fr), relative, nms_radius)
    words_t = None if words is None else torch.from_numpy(words.view(np.int64)).to(fr.data.device)
    return fr, peaks, counts, words_t


def find_chessboard_corners(images, pattern, relative=8, nms_radius=3, return_info=False):
    """The inner corners of a chessboard of ``pattern`` = (across, down) corners from the image alone, on the GPU, for
    every frame at once -> ``(found, corners)``: bool and float32 (n, 2) for one image, (f,) and (f, n, 2) for a batch,
    NumPy or CUDA like ``images``; corners are whole pixels in the board's order (across fastest), NaN where the board
    was not found -- seeds for ``corner_sub_pix``.  The detector is this package's own, NOT
    cv2.findChessboardCorners: ChESS response -> peaks of at least 1 / ``relative`` of the frame's strongest, alone in
    their (2 ``nms_radius`` + 1)^2 window -> a lattice grown from the peak nearest the centroid.  Squares below about
    12 px and corners within 5 px of a border are out of its range; of the two (a square pattern: four) ways to number
    a board it returns the one whose first corner comes first in pixel order.

    ``images``: uint8 gray or colour (through ``cvt_gray(code="bgr")``), (h, w[, 3]) or (f, h, w[, 3]), sides up to
    16384.  ``return_info``: ``(found, corners, status, counts)`` -- status 0 found, 1 fewer candidates than corners,
    2 more candidates than the 1024 kept, 4 lattice incomplete or of another size; counts: the candidates, int32."""
    import torch
    across, down, relative, nms_radius = chess_arguments(pattern, relative, nms_radius)
    fr, peaks, counts, _ = _candidates(images, relative, nms_radius)
    dev = fr.data.device
    corners = torch.empty((fr.f, across * down, 2), dtype=torch.float32, device=dev)
    status = torch.empty(fr.f, dtype=torch.int32, device=dev)
    call("camd_chess_lattice", dev, peaks.data_ptr(), counts.data_ptr(), fr.w, fr.h, fr.f, across, down, corners.data_ptr(),
         status.data_ptr(), what="find_chessboard_corners")
    out = (status == 0, corners, status, counts)
    return to_result(out if return_info else out[:2], fr.batched, fr.was_np)


# ---- ChArUco boards, cut or partly covered ones included (csrc/charuco.hip; a contract of our own) ----
CHARUCO_MIN_SQUARES, CHARUCO_MAX_SQUARES, CHARUCO_MAX_RATIO_DEN, CHARUCO_MAX_IDS = 3, 16, 64, 1024
CHARUCO_FEW, CHARUCO_OVERFLOW, CHARUCO_NO_LATTICE, CHARUCO_NO_CONSENSUS = 1, 2, 4, 8  # find_charuco_corners' status; 0 = found
_MIN_SIDE = 3  # the ChArUco and marker detectors take sides from 3


def charuco_arguments(squares_xy, dictionary, marker_ratio, first_id, relative, nms_radius, min_markers, max_bit_errors):
    """(sx, sy, words (n_ids,) uint64, s, num, den, first_id, relative, nms_radius, min_markers, max_bit_errors) within
    the detector's limits, or ValueError"""
    from . import boards
    try:
        sx, sy = squares_xy
        num, den = marker_ratio
    except (TypeError, ValueError):
        raise ValueError("squares_xy must be the squares (across, down) and marker_ratio two integers (numerator, denominator), "
                         "got %r and %r" % (squares_xy, marker_ratio))
    sx, sy = integer(sx, "squares across"), integer(sy, "squares down")
    num, den = integer(num, "the ratio's numerator"), integer(den, "the ratio's denominator")
    first_id, min_markers, max_bit_errors = integer(first_id, "first_id"), integer(min_markers, "min_markers"), integer(max_bit_errors, "max_bit_errors")
    _, _, relative, nms_radius = chess_arguments((2, 2), relative, nms_radius)
    if not (CHARUCO_MIN_SQUARES <= sx <= CHARUCO_MAX_SQUARES and CHARUCO_MIN_SQUARES <= sy <= CHARUCO_MAX_SQUARES):
        raise ValueError("a board of %d x %d squares; the detector takes %d .. %d each way" % (sx, sy, CHARUCO_MIN_SQUARES, CHARUCO_MAX_SQUARES))
    words = boards.marker_words(dictionary)
    s = int(np.shape(dictionary)[1])
    if not 0 < num < den <= CHARUCO_MAX_RATIO_DEN:
        raise ValueError("marker_ratio %d / %d: a marker's share of its square is 0 < numerator < denominator <= %d"
                         % (num, den, CHARUCO_MAX_RATIO_DEN))
    if first_id < 0 or first_id + (sx * sy) // 2 > len(words):
        raise ValueError("the board's %d markers from id %d on do not fit a dictionary of %d ids" % ((sx * sy) // 2, first_id, len(words)))
    if min_markers < 1 or not 0 <= max_bit_errors <= s * s:
        raise ValueError("min_markers >= 1 and max_bit_errors 0 .. %d, got %d and %d" % (s * s, min_markers, max_bit_errors))
    return sx, sy, words, s, num, den, first_id, relative, nms_radius, min_markers, max_bit_errors


def find_charuco_corners(images, squares_xy, dictionary, marker_ratio=(1, 2), first_id=0, relative=8, nms_radius=3, min_markers=2,
                         return_info=False, max_bit_errors=0):
    """The inner corners of a ChArUco board of ``squares_xy`` = (across, down) squares from the image alone, on the GPU,
    for every frame at once, boards cut by the image or partly covered included -> ``(found, corners)``: bool and
    float32 (n, 2) for one image, (f,) and (f, n, 2) for a batch, NumPy or CUDA like ``images``; n = (across - 1) *
    (down - 1), row id = y * (across - 1) + x; whole pixels -- seeds for ``corner_sub_pix`` -- and NaN where a corner was
    not seen.  The detector is this package's own, NOT cv2.aruco's: the ChESS response and
    peaks of ``find_chessboard_corners``, then a lattice grown over whatever part of the board is in view, the markers
    in its cells decoded against ``dictionary`` and the numbering most markers agree on.

    ``dictionary``: (n_ids, s, s) bits, 1 = white, s = 4 .. 7, at most 1024 ids (``boards.make_marker_dictionary``,
    ``boards.marker_bits_from_bytes_list``); the board's markers are ``first_id`` onward in row-major order of its white
    squares, the top-left square black.  ``marker_ratio``: a marker's side as a share of its square, two integers.
    ``min_markers``: decoded markers that must agree.  ``max_bit_errors``: bits a marker may differ from its entry.
    ``return_info``: ``(found, corners, marker_ids, status, counts)`` -- marker_ids int32 (across * down,) per square, -1
    where none was decoded; status 0 found, 1 fewer than 5 candidates, 2 more than the 1024 kept, 4 no lattice, 8 no
    numbering enough markers agree on; counts: the candidates."""
    import torch
    sx, sy, words, s, num, den, first_id, relative, nms_radius, min_markers, max_bit_errors = charuco_arguments(
        squares_xy, dictionary, marker_ratio, first_id, relative, nms_radius, min_markers, max_bit_errors)
    fr, peaks, counts, words_t = _candidates(images, relative, nms_radius, _MIN_SIDE, words)
    dev = fr.data.device
    corners = torch.empty((fr.f, (sx - 1) * (sy - 1), 2), dtype=torch.float32, device=dev)
    marker_ids = torch.empty((fr.f, sx * sy), dtype=torch.int32, device=dev)
    status = torch.empty(fr.f, dtype=torch.int32, device=dev)
    call("camd_charuco_detect", dev, peaks.data_ptr(), counts.data_ptr(), fr.data.data_ptr(), fr.w, fr.h, fr.pitch, fr.stride, fr.f,
         sx, sy, num, den, words_t.data_ptr(), len(words), s, first_id, min_markers, max_bit_errors, corners.data_ptr(),
         marker_ids.data_ptr(), status.data_ptr(), what="find_charuco_corners")
    out = (status == 0, corners, marker_ids, status, counts)
    return to_result(out if return_info else out[:2], fr.batched, fr.was_np)


# ---- several ChArUco boards of one set in a frame (csrc/charuco.hip, k_charuco_multi) ----
CHARUCO_MAX_BOARDS = 8


def charuco_set(first_ids, markers, n_ids):
    """the boards' first ids as a list of 1 .. 8 integers whose ranges of ``markers`` ids lie inside the dictionary and
    apart from each other, or ValueError"""
    try:
        ids = list(first_ids)
    except TypeError:
        raise ValueError("first_ids must be the boards' first marker ids, one per board, got %r" % (first_ids,))
    if not 1 <= len(ids) <= CHARUCO_MAX_BOARDS:
        raise ValueError("a set of %d boards; the detector takes 1 .. %d" % (len(ids), CHARUCO_MAX_BOARDS))
    ids = [integer(v, "every one of first_ids") for v in ids]
    for k, a in enumerate(ids):
        if a < 0 or a + markers > n_ids:
            raise ValueError("board %d's %d markers from id %d on do not fit a dictionary of %d ids" % (k, markers, a, n_ids))
        for j, b in enumerate(ids[:k]):
            if a < b + markers and b < a + markers:
                raise ValueError("boards %d and %d share marker ids: %d .. %d and %d .. %d" % (j, k, b, b + markers - 1, a, a + markers - 1))
    return ids


def find_charuco_boards(images, squares_xy, dictionary, first_ids, marker_ratio=(1, 2), relative=8, nms_radius=3, min_markers=2,
                        return_info=False, max_bit_errors=0):
    """Every board of a SET in every frame, in one pass: B = ``len(first_ids)`` boards (1 .. 8) of the same ``squares_xy``,
    ``marker_ratio`` and ``dictionary``, board b carrying the markers ``first_ids[b]`` onward; the id ranges must lie apart.
    -> ``(seen, corners)``: bool (B, n) and float32 (B, n, 2) for one image, (f, B, n) and (f, B, n, 2) for a batch,
    NumPy or CUDA like ``images``; whole pixels, NaN where a corner was not seen, ``seen`` = not NaN.  The response and
    the peaks of ``find_charuco_corners`` are computed once for all boards; then seeds are tried outward from the
    centroid of all peaks until every board is found, each lattice numbered by the board most of its markers name (the
    rules: include/calibrating_amd.h).  With one board it is ``find_charuco_corners`` bit for bit.  The 1024 candidates
    are per frame, not per board, and the markers' own corners count.

    ``return_info``: ``(seen, corners, marker_ids, status, counts)`` -- marker_ids int32 (f, B, across * down), status
    int32 (f, B) with ``find_charuco_corners``' values per board (1 and 2 are the frame's), counts (f,)."""
    import torch
    sx, sy, words, s, num, den, _, relative, nms_radius, min_markers, max_bit_errors = charuco_arguments(
        squares_xy, dictionary, marker_ratio, 0, relative, nms_radius, min_markers, max_bit_errors)
    ids = charuco_set(first_ids, (sx * sy) // 2, len(words))
    fr, peaks, counts, words_t = _candidates(images, relative, nms_radius, _MIN_SIDE, words)
    dev, nb = fr.data.device, len(ids)
    corners = torch.empty((fr.f, nb, (sx - 1) * (sy - 1), 2), dtype=torch.float32, device=dev)
    marker_ids = torch.empty((fr.f, nb, sx * sy), dtype=torch.int32, device=dev)
    status = torch.empty((fr.f, nb), dtype=torch.int32, device=dev)
    board_set = _native.CharucoBoards(nb, (ctypes.c_int * CHARUCO_MAX_BOARDS)(*ids))
    call("camd_charuco_detect_multi", dev, peaks.data_ptr(), counts.data_ptr(), fr.data.data_ptr(), fr.w, fr.h, fr.pitch, fr.stride,
         fr.f, sx, sy, num, den, words_t.data_ptr(), len(words), s, ctypes.byref(board_set), min_markers, max_bit_errors,
         corners.data_ptr(), marker_ids.data_ptr(), status.data_ptr(), what="find_charuco_boards")
    out = (~torch.isnan(corners[..., 0]), corners, marker_ids, status, counts)
    return to_result(out if return_info else out[:2], fr.batched, fr.was_np)


# ---- stand-alone ArUco markers (csrc/markers.hip; a contract of our own) ----
MARKER_CAPACITY, MARKER_MAX_RADIUS, MARKER_MAX_BOX, MARKER_MIN_SIDE = 1024, 32, 1024, 4
MARKER_OVERFLOW = 2  # find_markers' status bit: more candidates than the 1024 kept, the frame has no markers
MARKER_REFINE_CRITERIA = (30, 0.01)
# the labels of a call (4 B per pixel) and the statistics beside them (16 B) stay within this; beyond it the frames go in chunks
MARKER_PLANE_BUDGET = 1 << 30


def _mask_arguments(block_radius, offset):
    block_radius, offset = integer(block_radius, "block_radius"), integer(offset, "offset")
    if not 1 <= block_radius <= MARKER_MAX_RADIUS or not -255 <= offset <= 255:
        raise ValueError("block_radius must be 1 .. %d and offset -255 .. 255, got %d and %d" % (MARKER_MAX_RADIUS, block_radius, offset))
    return block_radius, offset


def _dark_mask(fr, block_radius, offset):
    import torch
    mask = torch.empty((fr.f, fr.h, fr.w), dtype=torch.uint8, device=fr.data.device)
    call("camd_dark_mask", mask.device, fr.data.data_ptr(), fr.w, fr.h, fr.pitch, fr.stride, fr.f, block_radius, offset,
         mask.data_ptr(), what="dark_mask")
    return mask


def dark_mask(images, block_radius=8, offset=7):
    """Stage 1 of the marker detector: uint8 in the shape of the gray image(s), 1 where a pixel is darker than its
    surroundings -- ``(gray + offset) * A < S`` with S the sum of the (2 ``block_radius`` + 1)^2 window about it, clipped to
    the image, and A the pixels of that part.  The inside of a black area wider than the window is not dark.  ``images``:
    uint8 gray (h, w) / (f, h, w) or colour (through ``cvt_gray``), NumPy or CUDA; pitched views are read in place."""
    block_radius, offset = _mask_arguments(block_radius, offset)
    fr = gray_frames(images, max_side=CHESS_MAX_SIDE)
    return to_result(_dark_mask(fr, block_radius, offset), fr.batched, fr.was_np)


def _label_components(mask):
    import torch
    f, h, w = (int(v) for v in mask.shape)
    labels = torch.empty((f, h, w), dtype=torch.int32, device=mask.device)
    call("camd_label_components", mask.device, mask.data_ptr(), w, h, f, labels.data_ptr(), what="label_components")
    return labels


def label_components(mask):
    """Stage 2: the 4-connected components of ``mask != 0``, uint8 or bool (h, w) / (f, h, w) -> int32 of the same shape: a
    pixel's label is the least ``y * w + x`` of its component, -1 where the mask is 0."""
    import torch
    check_array(mask, "mask")
    if dtype_name(mask) not in ("uint8", "bool"):
        raise ValueError("mask must be uint8 or bool, got %s" % mask.dtype)
    if mask.ndim not in (2, 3) or 0 in tuple(mask.shape):
        raise ValueError("mask must be (h, w) or (f, h, w) and not empty, got %s" % (tuple(mask.shape),))
    if max(mask.shape[-2:]) > CHESS_MAX_SIDE:  # (a mask has no colour: (f, h, 3) is 3 wide)
        raise ValueError("mask of %s; the detector takes sides up to %d" % (tuple(mask.shape), CHESS_MAX_SIDE))
    if (mask.shape[0] if mask.ndim == 3 else 1) * mask.shape[-2] >= 2 ** 31:
        raise ValueError("mask: %d rows in all, the kernels take fewer than 2^31" % (mask.shape[0] * mask.shape[-2]))
    was_np = is_np(mask)
    m = to_device(mask.view(np.uint8) if was_np and mask.dtype == np.bool_ else mask)
    m = m.to(torch.uint8) if m.dtype == torch.bool else m
    return to_result(_label_components(m if m.ndim == 3 else m[None]), mask.ndim == 3, was_np)


def _marker_arguments(dictionary, block_radius, offset, min_side, max_side, max_bit_errors, refine_win):
    from . import boards
    block_radius, offset = _mask_arguments(block_radius, offset)
    min_side, max_side, max_bit_errors = integer(min_side, "min_side"), integer(max_side, "max_side"), integer(max_bit_errors, "max_bit_errors")
    if not MARKER_MIN_SIDE <= min_side <= max_side <= MARKER_MAX_BOX:
        raise ValueError("min_side %d, max_side %d; the detector takes %d <= min_side <= max_side <= %d" % (min_side, max_side, MARKER_MIN_SIDE, MARKER_MAX_BOX))
    words = boards.marker_words(dictionary)
    s = int(np.shape(dictionary)[1])
    if not 0 <= max_bit_errors <= s * s:
        raise ValueError("max_bit_errors must be 0 .. %d, got %d" % (s * s, max_bit_errors))
    if refine_win is not None:
        try:
            ww, wh = (int(v) for v in refine_win)
        except (TypeError, ValueError):
            raise ValueError("refine_win must be None or a pair of half-sizes, got %r" % (refine_win,))
        if ww <= 0 or wh <= 0:
            raise ValueError("refine_win must be None or a pair of positive half-sizes, got %r" % (refine_win,))
        refine_win = (ww, wh)
    return words, s, block_radius, offset, min_side, max_side, max_bit_errors, refine_win


def _marker_stages(fr, words_t, n_ids, s, block_radius, offset, min_side, max_side, max_bit_errors):
    """stages 1 to 6 on frames that fit the budget -> dict of CUDA tensors"""
    import torch
    dev, (f, h, w) = fr.data.device, (fr.f, fr.h, fr.w)
    mask = _dark_mask(fr, block_radius, offset)
    labels = _label_components(mask)
    cand = torch.full((f, MARKER_CAPACITY, 6), -1, dtype=torch.int32, device=dev)
    counts = torch.empty(f, dtype=torch.int32, device=dev)
    status = torch.empty(f, dtype=torch.int32, device=dev)
    ws = torch.empty(_native.lib().camd_marker_candidates_workspace_bytes(w, h, f) + 16, dtype=torch.uint8, device=dev)
    ws_ptr = (ws.data_ptr() + 15) // 16 * 16
    call("camd_marker_candidates", dev, labels.data_ptr(), w, h, f, min_side, max_side, ws_ptr, cand.data_ptr(), counts.data_ptr(),
         status.data_ptr(), what="find_markers")
    quads = torch.empty((f, MARKER_CAPACITY, 4, 2), dtype=torch.int32, device=dev)
    id_turn = torch.empty((f, MARKER_CAPACITY), dtype=torch.int32, device=dev)
    best = torch.empty((f, n_ids), dtype=torch.int32, device=dev)
    seen = torch.empty((f, n_ids), dtype=torch.uint8, device=dev)
    corners = torch.empty((f, n_ids, 4, 2), dtype=torch.float32, device=dev)
    call("camd_marker_decode", dev, fr.data.data_ptr(), w, h, fr.pitch, fr.stride, f, labels.data_ptr(), cand.data_ptr(),
         counts.data_ptr(), min_side, words_t.data_ptr(), n_ids, s, max_bit_errors, quads.data_ptr(), id_turn.data_ptr(),
         best.data_ptr(), seen.data_ptr(), corners.data_ptr(), what="find_markers")
    del ws
    return dict(status=status, counts=counts, candidates=cand, quads=quads, id_turn=id_turn, seen=seen.bool(), corners=corners)


def find_markers(images, dictionary, block_radius=8, offset=7, min_side=12, max_side=512, max_bit_errors=0, refine_win=(3, 3),
                 return_info=False):
    """Stand-alone ArUco markers by id from the image alone, on the GPU, for every frame at once -> ``(seen, corners)``:
    bool (n_ids,) and float32 (n_ids, 4, 2) for one image, (f, n_ids) and (f, n_ids, 4, 2) for a batch, NumPy or CUDA like
    ``images``; a marker's corners are its own top-left, top-right, bottom-right, bottom-left, NaN where it was not seen.
    The detector is this package's own, NOT cv2.aruco.detectMarkers: ``dark_mask`` ->
    ``label_components`` -> the components whose box has sides ``min_side`` .. ``max_side`` and keeps off the image's
    outermost pixels -> the four extreme pixels of each outline -> the marker decoded inside them against ``dictionary``
    ((n_ids, s, s) bits, 1 = white) with up to ``max_bit_errors`` wrong bits; of several candidates with one id the one with
    the fewest errors stands.  Black markers on a light quiet zone; for an inverted print pass ``255 - images``.

    The coarse corners are whole pixels, the centres of dark pixels, so they lie about half a pixel INSIDE the printed
    outline; ``refine_win``: the half-sizes of the ``corner_sub_pix`` window (criteria (30, 0.01)) the seen corners go
    through, ``None`` returns the coarse ones.  ``return_info``: ``(seen, corners, info)``, info a dict: ``status`` (f,) --
    bit 2: more than 1024 candidates, the frame has no markers --, ``counts`` (f,), and per candidate ``candidates``
    (f, 1024, 6) int32 (root, x0, y0, x1, y1, pixels), ``quads`` (f, 1024, 4, 2) int32 clockwise, -1 where rejected,
    ``id_turn`` (f, 1024) int32 id << 2 | turn or -1, and ``coarse`` the corners before refinement."""
    import torch
    words, s, block_radius, offset, min_side, max_side, max_bit_errors, refine_win = _marker_arguments(
        dictionary, block_radius, offset, min_side, max_side, max_bit_errors, refine_win)
    fr = gray_frames(images, max_side=CHESS_MAX_SIDE, min_side=_MIN_SIDE)
    frames = fr.data if fr.data.ndim == 3 else fr.data[None]
    words_t = torch.from_numpy(words.view(np.int64)).to(frames.device)
    chunk = max(1, min(fr.f, 65535, MARKER_PLANE_BUDGET // (20 * fr.h * fr.w)))
    parts = [_marker_stages(fr._replace(data=frames[a:a + chunk], f=min(chunk, fr.f - a)), words_t, len(words), s,
                            block_radius, offset, min_side, max_side, max_bit_errors) for a in range(0, fr.f, chunk)]
    out = parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    seen, coarse = out["seen"], out["corners"]
    corners = coarse
    if refine_win is not None:
        corners = coarse.clone()
        lengths = (4 * seen.sum(1)).cpu().numpy()
        if int(lengths.sum()):
            corners[seen] = corner_sub_pix(frames, coarse[seen].reshape(-1, 2), refine_win, (-1, -1), MARKER_REFINE_CRITERIA,
                                           counts=lengths).reshape(-1, 4, 2)
    result = to_result((seen, corners), fr.batched, fr.was_np)
    info = dict(status=out["status"], counts=out["counts"], candidates=out["candidates"], quads=out["quads"], id_turn=out["id_turn"],
                coarse=coarse)
    return result + (to_result(info, fr.batched, fr.was_np),) if return_info else result


def laplacian_sums(images):
    """The exact sums behind ``sharpness``: int64 (f, 2) (a batch) or (2,) of S1 = sum L and S2 = sum L^2 over every frame,
    L the 3 x 3 Laplacian [0 1 0; 1 -4 1; 0 1 0] of the gray image with reflect-101 borders."""
    import torch
    fr = gray_frames(images, min_side=2)  # (the mirrored border takes sides from 2)
    sums = torch.empty((fr.f, 2), dtype=torch.int64, device=fr.data.device)
    call("camd_laplacian_sums", sums.device, fr.data.data_ptr(), fr.w, fr.h, fr.pitch, fr.stride, fr.f, sums.data_ptr(), what="sharpness")
    return to_result(sums, fr.batched, fr.was_np)


def sharpness(images):
    """``cv2.Laplacian(gray, cv2.CV_64F).var()`` of every image (reconstruction_with_board.py:9-12): a float for one
    image, float64 (f,) on the host for a batch.  uint8 gray (h, w) / (f, h, w) or colour (through ``cvt_gray(code="bgr")``),
    NumPy or CUDA, sides from 2.  The GPU gives the exact integer sums S1, S2 of the Laplacian and of its square
    (``laplacian_sums``); the variance (N S2 - S1^2) / N^2 is formed here from Python integers, rounded once.  UNPINNED
    against cv2."""
    from fractions import Fraction
    sums = laplacian_sums(images)
    sums = sums if is_np(sums) else sums.cpu().numpy()
    lay = layout(images, "images")
    n = lay.h * lay.w
    var = [float(Fraction(n * int(s2) - int(s1) ** 2, n * n)) for s1, s2 in sums.reshape(-1, 2)]
    return np.array(var, np.float64) if lay.batched else var[0]
