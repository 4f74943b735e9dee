"""Calibration boards: their object points and the image points of a frame (the role of the reference's calibrating/boards.py).

``Chessboard.find_image_points`` stands in for boards.py:156-172 with its middle step supplied by the caller: the
reference runs ``cv2.cvtColor -> cv2.findChessboardCorners -> cv2.cornerSubPix``; here the gray conversion and the
sub-pixel refinement run on the GPU (``imgproc.cvt_gray``, ``imgproc.corner_sub_pix``; csrc/subpix.hip) and the coarse
guess comes from ``d["corners"]`` / ``d["coarse_corners"]``: any detector's corners, or the previous frame's pose projected
with ``cam.project_points(board.object_points, T_prev)``.  ``findChessboardCorners`` itself, a heuristic quad search, is
not provided; ``Chessboard(..., detector="chess")`` finds the guess with this package's own detector
instead (``imgproc.find_chessboard_corners``; csrc/chessboard.hip), whose contract is not cv2's.
``CharucoBoard`` is the reference's ChArUco board with a detector of this package's own as well
(``imgproc.find_charuco_corners``; csrc/charuco.hip): boards cut by the image or partly covered are found, the caller brings
the marker dictionary.  ``MarkerBoard`` and ``ArucoGridBoard`` are boards of stand-alone ArUco markers, found by
``imgproc.find_markers`` (csrc/markers.hip), a third detector of this package's own.

What a board computes on the host -- its object points, its printable image, the pixels of a region of interest -- is
written from the behaviour the reference shows, which tests/golden/reference_boards.npz records bit for bit.
"""
import numpy as np

from ._frames import integer

SUBPIX_WIN, SUBPIX_ZERO_ZONE = (4, 4), (-1, -1)  # boards.py:166-167
SUBPIX_CRITERIA = (2 + 1, 30, 0.01)  # boards.py:161: cv2.TERM_CRITERIA_EPS + cv2.TERM_CRITERIA_MAX_ITER, 30, 0.01
POINT_KEYS = ("image_points", "corners", "marker_corners")  # what a region of interest moves back into the whole image
GUESS_KEYS = ("corners", "coarse_corners")
DETECTORS = (None, "chess")

NO_QUAD_SEARCH = ("Chessboard.find_image_points: no coarse corners -- the quad search of cv2.findChessboardCorners is not "
                  "provided.  Supply a start as d['corners'] or d['coarse_corners'], (n, 2) or (n, 1, 2): the corners of any "
                  "detector, or the previous frame's pose projected with cam.project_points(board.object_points, T_prev)")


def _roi_window(roi, h, w):
    """(row slice, column slice) of a region of an h x w image: None is the middle half, four numbers are (up, down,
    left, right), a slice cuts rows, a pair of slices rows and columns.  Bounds come back resolved: start >= 0."""
    if roi is None:
        rows, cols = slice(h // 4, 3 * h // 4), slice(w // 4, 3 * w // 4)
    elif isinstance(roi, slice):
        rows, cols = roi, slice(None)
    elif isinstance(roi[0], slice):
        rows, cols = roi
    else:
        up, down, left, right = roi
        rows, cols = slice(up, down), slice(left, right)
    for s in (rows, cols):
        if s.step not in (None, 1):
            raise ValueError("a region of interest is a contiguous window, got a step of %r" % (s.step,))
    return slice(*rows.indices(h)[:2]), slice(*cols.indices(w)[:2])


def _shifted(points, dx, dy):
    """points (..., 2) moved by (dx, dy) pixels -> contiguous float32; an id -> points dict entry by entry, types kept"""
    if isinstance(points, dict):
        return {key: value + (dx, dy) for key, value in points.items()}
    return np.ascontiguousarray((points + (dx, dy)).astype(np.float32))


class BaseBoard:
    """A board offers ``object_points`` (the whole board, its origin preferably at the centre) and ``find_image_points``."""

    def find_image_points(self, d):
        """``d`` is the record of one image (keys like "img", "path"): a board sets ``d["image_points"]`` (n, 2) and
        ``d["object_points"]`` (n, 3), arrays or id -> array dicts."""
        raise NotImplementedError()

    def __repr__(self):
        kwargs = getattr(self, "init_kwargs", None)
        return "Instance of %s" % type(self).__name__ if kwargs is None else str(kwargs)

    __str__ = __repr__

    @staticmethod
    def set_origin_to_center(points):
        """The points with their mean moved to the origin; for an id -> points dict the mean is over all its points."""
        if not isinstance(points, dict):
            return points - points.mean(axis=0, keepdims=True)
        every = np.concatenate([np.asarray(p).reshape(-1, np.shape(p)[-1]) for p in points.values()])
        centre = every.mean(axis=0, keepdims=True)
        return {key: p - centre for key, p in points.items()}

    @classmethod
    def get_roi_class(cls, roi_udlr=None):
        """A subclass that looks for its points inside a region only -- (up, down, left, right), a slice or a pair of
        slices, None for the middle half -- and reports them in the whole image's pixels, float32 (boards.py:100-138).
        A coarse guess in the record is in the whole image's pixels too and is left as it was given."""
        class RoiBoard(cls):
            def find_image_points(self, record):
                whole = record["img"]
                rows, cols = _roi_window(roi_udlr, whole.shape[0], whole.shape[1])
                given = {k: record[k] for k in GUESS_KEYS if record.get(k) is not None}
                for k, guess in given.items():
                    g = np.asarray(guess)
                    record[k] = g - np.array([cols.start, rows.start], g.dtype)
                record["img"] = whole[rows, cols]
                done = False
                try:
                    super().find_image_points(record)
                    done = True
                finally:
                    record["img"] = whole
                    if not done:
                        record.update(given)
                if "coarse_corners" in given:
                    record["coarse_corners"] = given["coarse_corners"]
                for k in POINT_KEYS:
                    if k in record:
                        record[k] = _shifted(record[k], cols.start, rows.start)

        return RoiBoard


class Chessboard(BaseBoard):
    def __init__(self, checkboard=(11, 8), size_mm=25, detector=None):
        """``checkboard``: inner corners (across, down); ``size_mm``: a square's side.  ``object_points``: (n, 3) float32
        metres in the board's plane, across fastest, the centre of the corners at the origin.  ``detector``: what
        ``find_image_points`` does with a record that carries no coarse corners -- None refuses it, "chess" runs
        ``imgproc.find_chessboard_corners``."""
        if detector not in DETECTORS:
            raise ValueError("detector must be one of %r, got %r" % (DETECTORS, detector))
        self.init_kwargs = dict(checkboard=checkboard, size_mm=size_mm)
        if detector is not None:
            self.init_kwargs["detector"] = detector
        self.checkboard, self.size_mm, self.detector = checkboard, size_mm, detector
        across, down = checkboard
        col, row = np.meshgrid(np.arange(across), np.arange(down))  # (down, across): across runs fastest when flattened
        grid = np.zeros((across * down, 3), np.float32)
        grid[:, 0] = col.ravel() * size_mm / 1000  # (float64 metres, rounded to float32 on the way in)
        grid[:, 1] = row.ravel() * size_mm / 1000
        self.object_points = self.set_origin_to_center(grid)

    def _coarse(self, coarse, frames=None):
        n = self.checkboard[0] * self.checkboard[1]
        c = coarse if hasattr(coarse, "is_cuda") else np.asarray(coarse)
        given = tuple(c.shape)
        if str(c.dtype).replace("torch.", "") not in ("float32", "float64"):
            c = c.astype(np.float32) if isinstance(c, np.ndarray) else c.float()
        want = (n, 2) if frames is None else (frames, n, 2)
        if frames is None and c.ndim == 3 and given[1:] == (1, 2):
            c = c[:, 0]
        if tuple(c.shape) != want:
            raise ValueError("the coarse corners of a %d x %d board must be %s%s, got %s" % (
                self.checkboard[0], self.checkboard[1], want, " or (%d, 1, 2)" % n if frames is None else "", given))
        return c

    def find_image_points(self, d):
        """boards.py:156-172 with the coarse guess taken from ``d["corners"]`` or ``d["coarse_corners"]``, (n, 2) or
        (n, 1, 2): gray conversion as the reference does it (its RGB image through COLOR_BGR2GRAY) and
        ``cornerSubPix(gray, corners, (4, 4), (-1, -1), (EPS + MAX_ITER, 30, 0.01))`` on the GPU.  Sets ``d["corners"]``
        (n, 1, 2) float32, ``d["image_points"]`` (n, 2) and ``d["object_points"]``.  Without a guess: NotImplementedError,
        or with ``detector="chess"`` the guess is detected first, and a record whose board is not found is left without
        ``image_points`` (the reference's ``if ok``, boards.py:162)."""
        from . import imgproc
        coarse = d.get("corners")
        if coarse is None:
            coarse = d.get("coarse_corners")
        if coarse is None:
            if self.detector is None:
                raise NotImplementedError(NO_QUAD_SEARCH)
            coarse = self.detect_corners(d["img"])
            if coarse is None:
                return
        coarse = self._coarse(coarse)
        if not isinstance(coarse, np.ndarray):
            coarse = coarse.detach().cpu().numpy()
        img, coarse = d["img"], np.ascontiguousarray(coarse, np.float32)
        if isinstance(img, np.ndarray):
            corners = imgproc.corner_sub_pix(img, coarse, SUBPIX_WIN, SUBPIX_ZERO_ZONE, SUBPIX_CRITERIA)
        else:  # an image on the GPU stays there; the record's points are host data, as every detector leaves them
            import torch
            corners = imgproc.corner_sub_pix(img, torch.from_numpy(coarse).to(img.device), SUBPIX_WIN, SUBPIX_ZERO_ZONE,
                                             SUBPIX_CRITERIA).cpu().numpy()
        d["corners"] = corners[:, None]
        d["image_points"] = d["corners"][:, 0]
        d["object_points"] = self.object_points

    def detect_corners(self, img):
        """The board's corners in one image, from the image alone (``imgproc.find_chessboard_corners`` with its default
        thresholds): (n, 2) float32 whole pixels on the host, in the order of ``object_points``, or None where the board
        is not found."""
        from . import imgproc
        found, corners = imgproc.find_chessboard_corners(img, self.checkboard)
        if not bool(found):
            return None
        return corners if isinstance(corners, np.ndarray) else corners.cpu().numpy()

    def find_image_points_batch(self, images, coarse=None, return_info=False):
        """A whole recording in one launch: ``images`` (f, h, w) gray or (f, h, w, 3) as the reference's loader gives
        them, ``coarse`` (f, n, 2) -> the refined corners (f, n, 2), NumPy or CUDA like the inputs, ready for
        ``perspective_n_point_batch`` with ``object_points``.  ``return_info`` adds iterations and status.

        ``coarse=None``: detect, then refine -> ``(found, corners)``: (f,) bool and (f, n, 2) float32, NaN in the
        frames whose board is not found (their rows go through the refinement as starts that are no pixel and come back
        as they are); ``return_info`` adds the refinement's iterations and status and the detector's status and
        candidate counts."""
        from . import imgproc
        if coarse is None:
            det = imgproc.find_chessboard_corners(images, self.checkboard, return_info=return_info)
            if det[1].ndim != 3:
                raise ValueError("images must be a batch (f, h, w) or (f, h, w, 3), got %s" % (tuple(images.shape),))
            refined = imgproc.corner_sub_pix(images, det[1], SUBPIX_WIN, SUBPIX_ZERO_ZONE, SUBPIX_CRITERIA, return_info=return_info)
            return (det[0], refined) if not return_info else (det[0],) + tuple(refined) + tuple(det[2:])
        coarse = self._coarse(coarse, int(images.shape[0]))
        return imgproc.corner_sub_pix(images, coarse, SUBPIX_WIN, SUBPIX_ZERO_ZONE, SUBPIX_CRITERIA, return_info=return_info)

    @classmethod
    def build_with_calibration_img(cls, hw=(1080, 1920), n=15, ppi=300):
        """A board with its printable picture (boards.py:191-218), host NumPy: ``calibration_img`` (h, w) uint8, white
        paper carrying squares of ``h // (n + 1)`` pixels that start half a square from the top left and alternate from
        black; as many whole squares as leave that margin, one column fewer where rows and columns would have the same
        parity (such a board maps onto itself under a half turn and has two legal poses).  The board's ``size_mm`` stays
        25 as in the reference; the printed size at ``ppi`` goes into ``calibration_img_name``."""
        height, width = int(hw[0]), int(hw[1])
        square = height // (n + 1)
        down, across = (height - square) // square, (width - square) // square
        if (across - down) % 2 == 0:
            across -= 1
        margin = square // 2
        row = (np.arange(height) - margin) // square  # the square a pixel row lies in; outside [0, down) is paper
        col = (np.arange(width) - margin) // square
        on_board = ((row >= 0) & (row < down))[:, None] & ((col >= 0) & (col < across))[None, :]
        black = on_board & ((row[:, None] + col[None, :]) % 2 == 0)
        board = cls(checkboard=(across - 1, down - 1), size_mm=25)
        board.calibration_img = np.where(black, 0, 255).astype(np.uint8)
        board.calibration_img_info = dict(hw=hw, ppi=ppi, **board.init_kwargs)
        printed_mm = round(square / ppi * 25.4, 2)
        board.calibration_img_name = "checkboard_hw%dx%d_size%smm.png" % (down - 1, across - 1, printed_mm)
        return board


# ---- marker dictionaries (host) ----------------------------------------------------------------------------------------
MARKER_MIN_BITS, MARKER_MAX_BITS, MARKER_MAX_IDS = 4, 7, 1024


def _check_marker_bits(bits):
    b = np.asarray(bits)
    if b.ndim != 3 or b.shape[1] != b.shape[2] or not MARKER_MIN_BITS <= b.shape[1] <= MARKER_MAX_BITS:
        raise ValueError("a marker dictionary is (n_ids, s, s) bits with s = %d .. %d, got %s"
                         % (MARKER_MIN_BITS, MARKER_MAX_BITS, b.shape))
    if not 1 <= b.shape[0] <= MARKER_MAX_IDS:
        raise ValueError("a marker dictionary holds 1 .. %d ids, got %d" % (MARKER_MAX_IDS, b.shape[0]))
    if b.dtype.kind not in "biu" or ((b != 0) & (b != 1)).any():
        raise ValueError("marker bits are 0 (black) or 1 (white)")
    return np.ascontiguousarray(b, np.uint8)


def marker_words(bits):
    """(n_ids, s, s) bits -> (n_ids,) uint64: a marker's rows from the top, each from the left, the first bit highest --
    bit (r, c) has the weight 2^(s*s - 1 - (r*s + c)).  What ``camd_charuco_detect`` takes as ``dictionary_words``."""
    b = _check_marker_bits(bits)
    s = b.shape[1]
    weights = np.uint64(1) << np.arange(s * s - 1, -1, -1, dtype=np.uint64)
    return (b.reshape(len(b), -1).astype(np.uint64) * weights).sum(1, dtype=np.uint64)


def marker_bytes_list(bits):
    """(n_ids, s, s) bits -> (n_ids, ceil(s*s / 8), 4) uint8 in the packing ``marker_bits_from_bytes_list`` reads: plane k
    holds the marker turned k quarter turns (``np.rot90(m, -k)``), bits in row-major order, eight to a byte, the first
    highest; a last byte that is not full holds its bits in its LOW end."""
    b = _check_marker_bits(bits)
    n, s = b.shape[0], b.shape[1]
    nbytes = (s * s + 7) // 8
    out = np.zeros((n, nbytes, 4), np.uint8)
    for k in range(4):
        flat = np.rot90(b, -k, axes=(1, 2)).reshape(n, -1)
        for i in range(nbytes):
            for bit in flat[:, 8 * i:8 * i + 8].T:
                out[:, i, k] = out[:, i, k] * 2 + bit
    return out


def marker_bits_from_bytes_list(bytes_list, s):
    """``cv2.aruco.Dictionary.bytesList`` (n_ids, ceil(s*s / 8), 4) -> (n_ids, s, s) uint8 bits, 1 = white: rotation 0
    (plane 0), bits in row-major order, the first bit the highest of a byte, a last byte that is not full right-aligned.
    UNPINNED: written from recollection of cv2's Dictionary::getBitsFromByteList; no cv2 is at hand
    to confirm it.  ``boards.marker_bytes_list`` is its inverse."""
    a = np.asarray(bytes_list)
    s = int(s)
    if not MARKER_MIN_BITS <= s <= MARKER_MAX_BITS:
        raise ValueError("s must be %d .. %d, got %d" % (MARKER_MIN_BITS, MARKER_MAX_BITS, s))
    nbytes = (s * s + 7) // 8
    if a.ndim != 3 or a.shape[1:] != (nbytes, 4) or a.dtype.kind not in "iu" or (a < 0).any() or (a > 255).any():
        raise ValueError("bytes_list of %d x %d markers is (n_ids, %d, 4) bytes, got %s %s" % (s, s, nbytes, a.dtype, a.shape))
    rot0 = a[:, :, 0].astype(np.uint8)
    bits = np.zeros((len(a), s * s), np.uint8)
    for i in range(s * s):
        byte, pos = divmod(i, 8)
        width = min(8, s * s - 8 * byte)  # bits the byte holds
        bits[:, i] = (rot0[:, byte] >> (width - 1 - pos)) & 1
    return _check_marker_bits(bits.reshape(len(a), s, s))


def _splitmix64(state):
    """one step of the splitmix64 generator: (next state, 64 random bits) -- plain integers, the same on every machine"""
    state = (state + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return state, z ^ (z >> 31)


def marker_distance(a, b=None):
    """the least Hamming distance of marker a (s, s) to the four turns of marker b; without b: of a to its own three turns"""
    a = np.asarray(a)
    turns, b = (range(1, 4), a) if b is None else (range(4), np.asarray(b))
    return min(int((a != np.rot90(b, k)).sum()) for k in turns)


def make_marker_dictionary(n, s, seed=0, min_distance=None):
    """A deterministic marker dictionary of this package's own (NOT one of cv2's tables): (n, s, s) uint8 bits, 1 = white.
    Markers are drawn from splitmix64(seed) and kept where they lie at least ``min_distance`` bits (default s*s // 4)
    from every turn of every marker kept before and from their own three turns, and hold at least s white and s black
    bits.  The same arguments give the same dictionary everywhere.  ValueError where 100 000 draws do not fill it."""
    n, s, state = int(n), int(s), int(seed) & 0xFFFFFFFFFFFFFFFF
    if not MARKER_MIN_BITS <= s <= MARKER_MAX_BITS or not 1 <= n <= MARKER_MAX_IDS:
        raise ValueError("n = 1 .. %d markers of s = %d .. %d bits a side, got n = %d, s = %d"
                         % (MARKER_MAX_IDS, MARKER_MIN_BITS, MARKER_MAX_BITS, n, s))
    need = s * s // 4 if min_distance is None else int(min_distance)
    kept, turns = [], []
    for _ in range(100000):
        if len(kept) == n:
            break
        state, z = _splitmix64(state)
        m = np.array([(z >> (s * s - 1 - i)) & 1 for i in range(s * s)], np.uint8).reshape(s, s)
        if not s <= int(m.sum()) <= s * s - s or marker_distance(m) < need:
            continue
        if turns and int((np.stack(turns) != m).sum((1, 2)).min()) < need:
            continue
        kept.append(m)
        turns += [np.rot90(m, k) for k in range(4)]
    if len(kept) < n:
        raise ValueError("no %d markers of %d x %d bits at distance %d from seed %d; ask for fewer or a smaller distance"
                         % (n, s, s, need, seed))
    return np.stack(kept)


# ---- the ChArUco board -------------------------------------------------------------------------------------------------
CHARUCO_MIN_POINTS = 11  # boards.py:389
NO_DICTIONARY = ("CharucoBoard: no marker dictionary -- cv2's tables are not part of this package.  Pass dictionary=(n_ids, s, "
                 "s) bits: boards.marker_bits_from_bytes_list(cv2.aruco.getPredefinedDictionary(tag).bytesList, s) from a machine "
                 "with cv2.aruco, or boards.make_marker_dictionary(n, s) for a board of this package's own")


class CharucoBoard(BaseBoard):
    def __init__(self, square_xy=(9, 5), square_size_mm=44.95, marker_size_mm=22.475, dictionary=None, first_id=0,
                 invert_color=False, using_marker_corner=False):
        """The reference's ChArUco board (boards.py:311-353) with the marker dictionary supplied by the caller.
        ``square_xy``: squares (across, down), the top-left one black; markers sit in the white squares, their ids
        ascending from ``first_id`` in row-major order.  ``object_points``: {id: (1, 3) float32 metres} of the inner
        corners, id = y * (across - 1) + x at ((x + 1) * square, (y + 1) * square, 0), their centre moved to the origin.
        The layout is cv2's current one as far as known and UNPINNED.  ``invert_color``: the board
        is printed black on white inverted; images are inverted before detection (boards.py:357-358)."""
        if dictionary is None:
            raise ValueError(NO_DICTIONARY)
        if using_marker_corner:
            raise NotImplementedError("CharucoBoard(using_marker_corner=True): the markers' own corners are not detected; "
                                      "only the board's inner corners are")
        self.dictionary = _check_marker_bits(dictionary)
        sx, sy = (int(v) for v in square_xy)
        self.square_xy, self.first_id, self.invert_color = (sx, sy), int(first_id), bool(invert_color)
        self.square_size_mm, self.marker_size_mm = square_size_mm, marker_size_mm
        self.init_kwargs = dict(square_xy=square_xy, square_size_mm=square_size_mm, marker_size_mm=marker_size_mm,
                                first_id=first_id, using_marker_corner=False, invert_color=invert_color)
        from fractions import Fraction
        ratio = Fraction(float(marker_size_mm) / float(square_size_mm)).limit_denominator(64)
        self.marker_ratio = (ratio.numerator, ratio.denominator)
        from . import detect
        detect.charuco_arguments(self.square_xy, self.dictionary, self.marker_ratio, self.first_id, 8, 3, 2, 0)
        x, y = np.meshgrid(np.arange(sx - 1), np.arange(sy - 1))
        grid = np.zeros(((sx - 1) * (sy - 1), 3), np.float32)
        grid[:, 0] = (x.ravel() + 1) * (square_size_mm / 1000.0)
        grid[:, 1] = (y.ravel() + 1) * (square_size_mm / 1000.0)
        self.object_points = self.set_origin_to_center({i: xyz[None] for i, xyz in enumerate(grid)})

    @property
    def n_corners(self):
        return (self.square_xy[0] - 1) * (self.square_xy[1] - 1)

    def marker_squares(self):
        """[(x, y)] of the squares that carry a marker, in the order of their ids from ``first_id``"""
        sx, sy = self.square_xy
        return [(x, y) for y in range(sy) for x in range(sx) if x % 2 != y % 2]

    def _detect(self, images, return_info=False):
        from . import imgproc
        if self.invert_color:
            images = 255 - images
        return imgproc.find_charuco_corners(images, self.square_xy, self.dictionary, self.marker_ratio, self.first_id,
                                            return_info=return_info)

    def find_image_points_batch(self, images, return_info=False):
        """A whole recording in one call: ``images`` (f, h, w) gray or (f, h, w, 3), NumPy or CUDA -> ``(seen, corners)``:
        (f, n) bool and (f, n, 2) float32 of the same kind -- the inner corners the detector saw in every frame, refined
        by ``corner_sub_pix`` with the reference's arguments (the seen corners only, as ragged rows), NaN where unseen.
        ``return_info`` adds ``found`` (f,), ``marker_ids`` (f, across * down), ``status`` and ``counts``."""
        import torch
        from . import imgproc
        found, coarse, marker_ids, status, counts = self._detect(images, return_info=True)
        if coarse.ndim != 3:
            raise ValueError("images must be a batch (f, h, w) or (f, h, w, 3), got %s" % (tuple(images.shape),))
        was_np = isinstance(coarse, np.ndarray)
        c = torch.from_numpy(coarse).to(imgproc.to_device(images).device) if was_np else coarse
        seen = ~torch.isnan(c[..., 0])
        lengths = seen.sum(1).cpu().numpy()
        corners = torch.full_like(c, float("nan"))
        if int(lengths.sum()):
            dev_images = images if not was_np else torch.from_numpy(np.ascontiguousarray(images)).to(c.device)
            corners[seen] = imgproc.corner_sub_pix(dev_images, c[seen], SUBPIX_WIN, SUBPIX_ZERO_ZONE, SUBPIX_CRITERIA, counts=lengths)
        if was_np:
            seen, corners = seen.cpu().numpy(), corners.cpu().numpy()
        return (seen, corners, found, marker_ids, status, counts) if return_info else (seen, corners)

    def to_frames(self, seen, corners, keys=None):
        """What ``find_image_points_batch`` returned -> {key: dict(ids, image_points, object_points)} as
        ``Cam.from_detections`` takes it: the reference's id -> points dictionaries of the frames that show at least 11
        corners (boards.py:389).  ``keys``: one per frame, default 0 .. f - 1."""
        seen = np.asarray(seen.cpu() if hasattr(seen, "is_cuda") else seen)
        corners = np.asarray(corners.cpu() if hasattr(corners, "is_cuda") else corners)
        keys = range(len(seen)) if keys is None else list(keys)
        if len(keys) != len(seen):
            raise ValueError("%d keys for %d frames" % (len(keys), len(seen)))
        frames = {}
        for key, s, c in zip(keys, seen, corners):
            ids = np.flatnonzero(s)
            if len(ids) >= CHARUCO_MIN_POINTS:
                frames[key] = dict(ids=ids, image_points={int(i): c[i][None] for i in ids},
                                   object_points={int(i): self.object_points[int(i)] for i in ids})
        return frames

    def find_image_points(self, d):
        """boards.py:355-395 with this package's detector in place of cv2.aruco's: detects the board in ``d["img"]``,
        refines the seen inner corners with ``corner_sub_pix`` and, where at least 11 are seen, sets ``d["ids"]``,
        ``d["image_points"]`` and ``d["object_points"]`` ({id: (1, 2)} and {id: (1, 3)}) and ``d["corners"]`` (k, 1, 2).
        ``d["marker_ids"]`` is set in every case: the ids decoded, in row-major order of their squares.  A record whose
        board is not found or shows fewer corners is left without ``image_points``."""
        img = d["img"]
        seen, corners, found, marker_ids, _, _ = self.find_image_points_batch(img[None], return_info=True)
        if not isinstance(seen, np.ndarray):
            seen, corners, marker_ids = seen.cpu().numpy(), corners.cpu().numpy(), marker_ids.cpu().numpy()
        d["marker_ids"] = marker_ids[0][marker_ids[0] >= 0]
        frames = self.to_frames(seen, corners)
        if 0 in frames:
            d.update(frames[0], corners=corners[0][seen[0]][:, None])

    def draw(self, square_px, margin_px=0):
        """the board as a picture, host NumPy: (down * square_px + 2 margin, across * square_px + 2 margin) uint8, white
        paper, a marker's cells ``round``-ed to whole pixels inside its square"""
        sx, sy = self.square_xy
        q, m, s = int(square_px), int(margin_px), self.dictionary.shape[1]
        img = np.full((sy * q + 2 * m, sx * q + 2 * m), 255, np.uint8)
        num, den = self.marker_ratio
        side = q * num // den
        edges = (q - side) // 2 + np.rint(np.arange(s + 3) * side / (s + 2)).astype(int)
        ids = {sq: k for k, sq in enumerate(self.marker_squares())}
        for y in range(sy):
            for x in range(sx):
                cell = img[m + y * q:m + (y + 1) * q, m + x * q:m + (x + 1) * q]
                if x % 2 == y % 2:
                    cell[:] = 0
                    continue
                k = self.first_id + ids[(x, y)]
                if k >= len(self.dictionary):
                    raise ValueError("the board's marker %d is not in a dictionary of %d ids" % (k, len(self.dictionary)))
                full = np.zeros((s + 2, s + 2), np.uint8)
                full[1:-1, 1:-1] = self.dictionary[k]
                for r in range(s + 2):
                    for c in range(s + 2):
                        cell[edges[r]:edges[r + 1], edges[c]:edges[c + 1]] = 255 * full[r, c]
        return 255 - img if self.invert_color else img

    @classmethod
    def build_with_calibration_img(cls, hw=(2480, 3508), n=10, ppi=300, dictionary=None, seed=0, invert_color=False, **init_kwargs):
        """A board with its printable picture (boards.py:406-441), host NumPy: squares of ``max(hw) // n`` pixels, as many
        whole ones as fit, markers of 0.75 of a square, the board centred on white paper.  ``dictionary=None`` makes one
        with ``make_marker_dictionary(markers, 4, seed)``.  ``calibration_img`` is (h, w) uint8."""
        height, width = int(hw[0]), int(hw[1])
        size = max(height, width) // n
        size_mm = round(size / ppi * 25.4, 2)
        sx, sy = width // size, height // size
        if dictionary is None:
            dictionary = make_marker_dictionary(init_kwargs.get("first_id", 0) + (sx * sy) // 2, 4, seed)
        init_kwargs.update(square_xy=(sx, sy), square_size_mm=size_mm, marker_size_mm=size_mm * 0.75, dictionary=dictionary,
                           invert_color=invert_color)
        board = cls(**init_kwargs)
        img = np.full((height, width), 0 if invert_color else 255, np.uint8)
        top, left = (height - sy * size) // 2, (width - sx * size) // 2
        img[top:top + sy * size, left:left + sx * size] = board.draw(size)
        board.calibration_img = img
        board.calibration_img_info = dict(hw=hw, ppi=ppi, seed=seed, **board.init_kwargs)
        board.calibration_img_name = "charuco_square_x%dy%d_size%smm.png" % (sx, sy, size_mm)
        return board


# ---- several boards in one picture -------------------------------------------------------------------------------------
NOT_A_SET = ("MultiBoards.find_image_points_batch: the boards are no set -- ChArUco boards of the same squares, sizes and "
             "dictionary with marker ids apart, 8 at the most -- so there is no one-pass detection for them; call "
             "find_image_points frame by frame, which falls back to each board's own detector")


class MultiBoards(BaseBoard):
    def __init__(self, boards, imgs=None, cam=None):
        """Several boards that stand fixed to each other, used as ONE target (the reference's multi_boards.py:15-75).
        ``boards``: a list, or a dict taken in the order of its sorted keys.  ``imgs`` and ``cam``: pictures that show
        EVERY board and a calibrated camera, see ``add_board_imgs``; without them ``object_points`` is not set and only
        detection works.  Boards that form a SET -- ``CharucoBoard``s of the same squares, sizes, colour and dictionary
        (the same object or equal bits) whose marker ids lie apart, 8 at the most -- are detected in one pass
        (``imgproc.find_charuco_boards``); any other mix goes board by board through each board's own
        ``find_image_points``, as the reference loops, with that detector's limits.  ``vis_img`` is not provided."""
        if isinstance(boards, dict):
            boards = [boards[k] for k in sorted(boards)]
        self.boards = list(boards)
        self.Ts_all = []
        self.first_ids = self._set_first_ids()
        if imgs is not None:
            self.add_board_imgs(imgs, cam)

    def _set_first_ids(self):
        """the boards' first marker ids where they form a set, else None"""
        from . import detect
        bs = self.boards
        if not 1 <= len(bs) <= detect.CHARUCO_MAX_BOARDS or not all(isinstance(b, CharucoBoard) for b in bs):
            return None
        a = bs[0]
        for b in bs[1:]:
            if (b.square_xy, b.marker_ratio, b.invert_color, b.square_size_mm, b.marker_size_mm) != (
                    a.square_xy, a.marker_ratio, a.invert_color, a.square_size_mm, a.marker_size_mm):
                return None
            if b.dictionary is not a.dictionary and not np.array_equal(b.dictionary, a.dictionary):
                return None
        try:
            return detect.charuco_set([b.first_id for b in bs], (a.square_xy[0] * a.square_xy[1]) // 2, len(a.dictionary))
        except ValueError:
            return None

    def add_board_imgs(self, imgs, cam=None):
        """multi_boards.py:24-53: every picture gives each board's pose in board 0 (what ``cam.get_calibration_board_T``
        gives per board, a set detected in one pass; a picture must show them all), the poses of all pictures so far are averaged (``geometry.mean_Ts``) and
        ``object_points`` becomes {(boardi, id): points in board 0's frame}, their centre moved to the origin."""
        from . import geometry, pointcloud
        boards = self.boards
        if hasattr(imgs, "ndim") and imgs.ndim <= 3:
            imgs = [imgs]
        if cam is None:
            cam = self.cam
        else:
            self.cam = cam
        for img in imgs:
            records = self._board_records(img, cam)
            missing = [boardi for boardi, d in enumerate(records) if "T" not in d]
            if missing:
                raise ValueError("MultiBoards.add_board_imgs: a picture must show every board, boards %r were not found" % (missing,))
            Ts_in_cam = [d["T"] for d in records]
            T_cam_in_board0 = np.linalg.inv(Ts_in_cam[0])
            self.Ts_all.append([T_cam_in_board0 @ T for T in Ts_in_cam])
        self.Ts = [geometry.mean_Ts([Ts[boardi] for Ts in self.Ts_all]) for boardi in range(len(boards))]
        new_obj_points = {}
        for boardi, board in enumerate(boards):
            object_points = board.object_points
            if not isinstance(object_points, dict):
                object_points = {None: object_points}
            for k, object_point in object_points.items():
                new_obj_points[(boardi, k)] = pointcloud.apply_T_to_point_cloud(self.Ts[boardi], np.asarray(object_point))
        self.object_points = self.set_origin_to_center(new_obj_points)

    def _board_records(self, img, cam):
        """``cam.get_calibration_board_T(img, board)`` for every board; a set is detected in one pass over the picture --
        a board's own detector looks for one board and does not reach the outer ones of several"""
        if self.first_ids is None:
            return [cam.get_calibration_board_T(img, board) for board in self.boards]
        seen, corners = self.find_image_points_batch(img[None])
        if not isinstance(seen, np.ndarray):
            seen, corners = seen.cpu().numpy(), corners.cpu().numpy()
        records = []
        for board, s, c in zip(self.boards, seen[0], corners[0]):
            d = dict(img=img)
            d.update(board.to_frames(s[None], c[None]).get(0, {}))
            if "image_points" in d:
                d.update(cam.perspective_n_point(d["image_points"], d["object_points"]))
            records.append(d)
        return records

    def find_image_points_batch(self, images, return_info=False):
        """A whole recording in one call, for boards that form a set: ``images`` (f, h, w) gray or (f, h, w, 3), NumPy or
        CUDA -> ``(seen, corners)``: (f, B, n) bool and (f, B, n, 2) float32 of the same kind -- one detection pass for all
        boards, then the seen corners refined by ``corner_sub_pix`` with the reference's arguments as ragged rows; NaN
        where unseen.  ``return_info`` adds ``marker_ids`` (f, B, across * down), ``status`` (f, B) and ``counts`` (f,)."""
        import torch
        from . import imgproc
        if self.first_ids is None:
            raise ValueError(NOT_A_SET)
        a = self.boards[0]
        if getattr(images, "ndim", 0) not in (3, 4) or (images.ndim == 3 and images.shape[-1] == 3):
            raise ValueError("images must be a batch (f, h, w) or (f, h, w, 3), got %s" % (tuple(getattr(images, "shape", ())),))
        seen_in = 255 - images if a.invert_color else images
        _, coarse, marker_ids, status, counts = imgproc.find_charuco_boards(seen_in, a.square_xy, a.dictionary, self.first_ids,
                                                                            a.marker_ratio, return_info=True)
        was_np = isinstance(coarse, np.ndarray)
        c = torch.from_numpy(coarse).to(imgproc.to_device(images).device) if was_np else coarse
        seen = ~torch.isnan(c[..., 0])
        lengths = seen.sum((1, 2)).cpu().numpy()
        corners = torch.full_like(c, float("nan"))
        if int(lengths.sum()):
            dev_images = images if not was_np else torch.from_numpy(np.ascontiguousarray(images)).to(c.device)
            corners[seen] = imgproc.corner_sub_pix(dev_images, c[seen], SUBPIX_WIN, SUBPIX_ZERO_ZONE, SUBPIX_CRITERIA, counts=lengths)
        if was_np:
            seen, corners = seen.cpu().numpy(), corners.cpu().numpy()
        return (seen, corners, marker_ids, status, counts) if return_info else (seen, corners)

    def _points_by_board(self, seen, corners):
        """{(boardi, id): (1, 2)} of one frame's rows, of the boards that show at least 11 corners (boards.py:389)"""
        points = {}
        for boardi, (s, c) in enumerate(zip(seen, corners)):
            ids = np.flatnonzero(s)
            if len(ids) >= CHARUCO_MIN_POINTS:
                points.update({(boardi, int(i)): c[i][None] for i in ids})
        return points

    def to_frames(self, seen, corners, keys=None):
        """What ``find_image_points_batch`` returned -> {key: dict(ids, image_points, object_points)} as
        ``Cam.from_detections`` takes it, ids = (boardi, id), of the frames in which at least one board shows 11 corners;
        needs ``object_points`` (``add_board_imgs``).  ``keys``: one per frame, default 0 .. f - 1."""
        seen = np.asarray(seen.cpu() if hasattr(seen, "is_cuda") else seen)
        corners = np.asarray(corners.cpu() if hasattr(corners, "is_cuda") else corners)
        keys = range(len(seen)) if keys is None else list(keys)
        if len(keys) != len(seen):
            raise ValueError("%d keys for %d frames" % (len(keys), len(seen)))
        frames = {}
        for key, s, c in zip(keys, seen, corners):
            points = self._points_by_board(s, c)
            if points:
                frames[key] = dict(ids=sorted(points), image_points=points, object_points={i: self.object_points[i] for i in points})
        return frames

    def find_image_points(self, d):
        """multi_boards.py:55-75: ``d["image_points"]`` and ``d["object_points"]`` become {(boardi, id): points} over the
        boards found in ``d["img"]``; a record in which no board is found is left alone.  A set is detected in one pass."""
        all_image_points = {}
        if self.first_ids is not None:
            seen, corners = self.find_image_points_batch(d["img"][None])
            if not isinstance(seen, np.ndarray):
                seen, corners = seen.cpu().numpy(), corners.cpu().numpy()
            all_image_points = self._points_by_board(seen[0], corners[0])
        else:
            for boardi, board in enumerate(self.boards):
                d_ = dict(img=d["img"])
                board.find_image_points(d_)
                image_points = d_.get("image_points")
                if image_points is None:
                    continue
                if not isinstance(image_points, dict):
                    image_points = {None: image_points}
                for k, image_point in image_points.items():
                    all_image_points[(boardi, k)] = image_point
        if len(all_image_points) > 0:
            d.update(image_points=all_image_points, object_points={i: self.object_points[i] for i in all_image_points})


# ---- boards of stand-alone markers ---------------------------------------------------------------------------------------
class MarkerBoard(BaseBoard):
    def __init__(self, object_points, dictionary=None, occlusion=True):
        """Any layout of stand-alone ArUco markers as ONE target.  ``object_points``: {id: (4, 3)} metres, a marker's own
        top-left, top-right, bottom-right, bottom-left corners; they are kept as they are given.  ``dictionary``:
        (n_ids, s, s) bits that hold every id (see ``CharucoBoard``).  ``occlusion=False``: a frame counts only when
        EVERY marker of the board is seen -- the rule of the reference's PredifinedArucoBoard1 (boards.py:285-287), whose
        coordinate table is not part of this package: pass it here.  Detection is ``imgproc.find_markers`` with its
        defaults (csrc/markers.hip; a contract of this package's own); for an inverted print
        hand over ``255 - img``.  ``vis`` and cv2's DetectorParameters are not provided."""
        if dictionary is None:
            raise ValueError(NO_DICTIONARY.replace("CharucoBoard", type(self).__name__))
        self.dictionary = _check_marker_bits(dictionary)
        points = {}
        for key, p in dict(object_points).items():
            p = np.asarray(p, np.float32)
            if not 0 <= integer(key, "a marker id of object_points") < len(self.dictionary) or p.shape != (4, 3):
                raise ValueError("object_points maps a marker id of the dictionary (0 .. %d) to its (4, 3) corners, got %r -> %s"
                                 % (len(self.dictionary) - 1, key, p.shape))
            points[int(key)] = p
        if not points:
            raise ValueError("a board of no markers")
        self.object_points = points
        self.ids = np.array(sorted(points))
        self.occlusion = bool(occlusion)
        self.detector = dict(block_radius=8, offset=7, min_side=12, max_side=512, max_bit_errors=0, refine_win=(3, 3))

    def find_image_points_batch(self, images, return_info=False):
        """A whole recording in one call: ``images`` (f, h, w) gray or (f, h, w, 3), NumPy or CUDA -> ``(seen, corners)``:
        (f, m) bool and (f, m, 4, 2) float32 of the same kind over the board's m markers in the order of their ids, the
        corners refined by ``corner_sub_pix``, NaN where unseen.  ``return_info`` adds ``find_markers``' info."""
        from . import imgproc
        if getattr(images, "ndim", 0) not in (3, 4) or (images.ndim == 3 and images.shape[-1] == 3):
            raise ValueError("images must be a batch (f, h, w) or (f, h, w, 3), got %s" % (tuple(getattr(images, "shape", ())),))
        seen, corners, info = imgproc.find_markers(images, self.dictionary, return_info=True, **self.detector)
        ids = self.ids if isinstance(seen, np.ndarray) else imgproc.to_device(self.ids, device=seen.device)
        seen, corners = seen[:, ids], corners[:, ids]
        return (seen, corners, info) if return_info else (seen, corners)

    def to_frames(self, seen, corners, keys=None):
        """What ``find_image_points_batch`` returned -> {key: dict(ids, image_points, object_points)} as
        ``Cam.from_detections`` takes it: {id: (4, 2)} and {id: (4, 3)}, so a frame's rows stand in id order, four per
        marker.  A frame without a marker is left out, and with ``occlusion=False`` every frame that misses one.
        ``keys``: one per frame, default 0 .. f - 1."""
        seen = np.asarray(seen.cpu() if hasattr(seen, "is_cuda") else seen)
        corners = np.asarray(corners.cpu() if hasattr(corners, "is_cuda") else corners)
        keys = range(len(seen)) if keys is None else list(keys)
        if len(keys) != len(seen):
            raise ValueError("%d keys for %d frames" % (len(keys), len(seen)))
        frames = {}
        for key, s, c in zip(keys, seen, corners):
            at = np.flatnonzero(s)
            if len(at) == 0 or (not self.occlusion and len(at) != len(self.ids)):
                continue
            ids = self.ids[at]
            frames[key] = dict(ids=ids, image_points={int(i): c[k] for i, k in zip(ids, at)},
                               object_points={int(i): self.object_points[int(i)] for i in ids})
        return frames

    def find_image_points(self, d):
        """Detects the board's markers in ``d["img"]`` and, where the frame counts, sets ``d["ids"]``,
        ``d["image_points"]`` {id: (4, 2)} and ``d["object_points"]`` {id: (4, 3)}; ``d["valid"]`` says whether it did."""
        seen, corners = self.find_image_points_batch(d["img"][None])
        frames = self.to_frames(seen, corners)
        d["valid"] = 0 in frames
        if d["valid"]:
            d.update(frames[0])


class ArucoGridBoard(MarkerBoard):
    def __init__(self, grid_size=(5, 5), marker_length_mm=60.0, marker_separation_mm=10.0, dictionary=None, first_id=0):
        """The reference's grid of markers (boards.py:516-545) with the dictionary supplied by the caller.  Marker
        ``first_id + j * gx + i`` has its top-left corner at (i, j) * (length + separation), x to the right, y down, z = 0,
        its corners top-left, top-right, bottom-right, bottom-left; then the centre of all corners moves to the origin.
        The layout is cv2.aruco.GridBoard's current one as far as known and UNPINNED."""
        gx, gy = (int(v) for v in grid_size)
        first_id = int(first_id)
        if gx < 1 or gy < 1 or first_id < 0:
            raise ValueError("a grid of %d x %d markers from id %d" % (gx, gy, first_id))
        length, pitch = marker_length_mm / 1000.0, (marker_length_mm + marker_separation_mm) / 1000.0
        square = np.array([[0, 0, 0], [length, 0, 0], [length, length, 0], [0, length, 0]], np.float64)
        points = {first_id + j * gx + i: (square + (i * pitch, j * pitch, 0)).astype(np.float32) for j in range(gy) for i in range(gx)}
        if dictionary is not None and first_id + gx * gy > len(dictionary):
            raise ValueError("the grid's %d markers from id %d on do not fit a dictionary of %d ids" % (gx * gy, first_id, len(dictionary)))
        super().__init__(points, dictionary)
        self.object_points = self.set_origin_to_center(self.object_points)
        self.grid_size, self.first_id = (gx, gy), first_id
        self.marker_length_mm, self.marker_separation_mm = marker_length_mm, marker_separation_mm
        self.init_kwargs = dict(grid_size=grid_size, marker_length_mm=marker_length_mm, marker_separation_mm=marker_separation_mm,
                                first_id=first_id)

    def draw(self, bit_px, margin_px=0):
        """the sheet as a picture, host NumPy, uint8: a marker is 6 ``bit_px`` wide whatever its bits (its s + 2 cells
        ``round``-ed to whole pixels), the separation 1 ``bit_px``, white paper, ``margin_px`` around"""
        gx, gy = self.grid_size
        s, q, m = self.dictionary.shape[1], int(bit_px), int(margin_px)
        img = np.full((gy * 7 * q - q + 2 * m, gx * 7 * q - q + 2 * m), 255, np.uint8)
        edges = np.rint(np.arange(s + 3) * (6 * q) / (s + 2)).astype(int)
        for j in range(gy):
            for i in range(gx):
                full = np.zeros((s + 2, s + 2), np.uint8)
                full[1:-1, 1:-1] = self.dictionary[self.first_id + j * gx + i]
                cell = img[m + j * 7 * q:m + j * 7 * q + 6 * q, m + i * 7 * q:m + i * 7 * q + 6 * q]
                for r in range(s + 2):
                    for c in range(s + 2):
                        cell[edges[r]:edges[r + 1], edges[c]:edges[c + 1]] = 255 * full[r, c]
        return img

    @classmethod
    def build_with_calibration_img(cls, hw=(2480, 3508), n=6, ppi=300, dictionary=None, seed=0, **init_kwargs):
        """A grid with its printable picture, host NumPy, in the reference's bit arithmetic (boards.py:579-607): a marker is
        6 units wide, the separation 1, the margin 1; a unit is ``max(hw) / (7 n + 1)`` pixels (``min(hw)`` for n = 1), and as
        many markers as fit: ``(int(side / unit + 1e-5) - 1) // 7`` each way.  Sizes in millimetres follow from ``ppi``.
        ``dictionary=None`` makes one with ``make_marker_dictionary(markers, 4, seed)``.  ``calibration_img`` is (h, w)
        uint8, the grid drawn with whole-pixel units (``int(unit)``) from a margin of ``round(unit)`` pixels."""
        height, width = int(hw[0]), int(hw[1])
        total = n * 7 + 1
        unit = (min(height, width) if n == 1 else max(height, width)) / total
        unit_mm = round(unit / ppi * 25.4, 2)
        gx, gy = (int(width / unit + 1e-5) - 1) // 7, (int(height / unit + 1e-5) - 1) // 7
        if dictionary is None:
            dictionary = make_marker_dictionary(init_kwargs.get("first_id", 0) + gx * gy, 4, seed)
        init_kwargs.update(grid_size=(gx, gy), marker_length_mm=unit_mm * 6, marker_separation_mm=unit_mm * 1, dictionary=dictionary)
        board = cls(**init_kwargs)
        margin = int(round(unit))
        sheet = board.draw(int(unit))
        img = np.full((height, width), 255, np.uint8)
        img[margin:margin + sheet.shape[0], margin:margin + sheet.shape[1]] = sheet
        board.calibration_img = img
        board.calibration_img_info = dict(hw=hw, ppi=ppi, seed=seed, bit_px=int(unit), margin_px=margin, **board.init_kwargs)
        board.calibration_img_name = "aruco_grid_x%dy%d_marker%smm_separation%smm.png" % (gx, gy, unit_mm * 6, unit_mm * 1)
        return board
