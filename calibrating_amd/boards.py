"""Calibration boards: their object points and the image points of a frame (the role of the reference's calibrating/boards.py).

``Chessboard.find_image_points`` stands in for boards.py:156-172 with its middle step supplied by the caller: the
reference runs ``cv2.cvtColor -> cv2.findChessboardCorners -> cv2.cornerSubPix``; here the gray conversion and the
sub-pixel refinement run on the GPU (``imgproc.cvt_gray``, ``imgproc.corner_sub_pix``; csrc/subpix.hip) and the coarse
guess comes from ``d["corners"]`` / ``d["coarse_corners"]``: any detector's corners, or the previous frame's pose projected
with ``cam.project_points(board.object_points, T_prev)``.  ``findChessboardCorners`` itself, a heuristic quad search, is
not provided; ``Chessboard(..., detector="chess")`` finds the guess with this package's own detector
instead (``imgproc.find_chessboard_corners``; csrc/chessboard.hip), whose contract is not cv2's.
The marker boards of the reference (ArUco, ChArUco) live in cv2.aruco and are not here.

What a board computes on the host -- its object points, its printable image, the pixels of a region of interest -- is
written from the behaviour the reference shows, which tests/golden/reference_boards.npz records bit for bit.
"""
import numpy as np

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
