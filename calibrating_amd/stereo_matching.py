"""StereoMatching plugin surface -- same names and contract as
/root/reference/calibrating/stereo_matching.py:10-70, with the SGBM plugin running on the MI355X.

``MetaStereoMatching``: ``__init__(cfg)``, ``__call__(img1, img2)`` with rectified RGB uint8
``(h, w, 3)`` images; returns ``disparity (h, w)`` in pixels of the input resolution or a dict
containing ``"disparity"`` (extra keys are merged into ``Stereo.get_depth``'s result,
stereo_camera.py:506-509).

A plugin whose class sets ``accepts_device_tensors = True`` (not in the reference) is handed the rectified pair as
torch CUDA tensors by ``Stereo.get_depth`` and may return a CUDA tensor (or a dict holding one); every other plugin
gets NumPy arrays, as in the reference.  ``FeatureMatchingAsStereoMatching`` (:113-142) is such a plugin.
"""
import numpy as np

from . import resize as _resize
from ._arrays import is_np, to_caller, to_device
from .sgbm import MODE_SGBM, StereoSGBM_create


class MetaStereoMatching:
    def __init__(self, cfg=None):
        self.cfg = cfg

    def __call__(self, img1, img2):
        # input: RGB uint8 (h, w, 3)uint8
        raise NotImplementedError()
        # output: float disparity (h, w), or dict(disparity=disparity)


class SemiGlobalBlockMatching(MetaStereoMatching):
    """cv2.StereoSGBM wrapper of the reference (stereo_matching.py:22-70) on the gfx950 kernels.

    ``cfg`` keys: ``max_size`` (reference key, default 1000: inputs are downsized so that
    max(h, w) <= max_size, :61-62) plus the StereoSGBM parameters, whose defaults are the values the
    reference hard-codes (:30-58): block 11, minDisparity 2, numDisparities 218, uniquenessRatio 5,
    speckleWindowSize 200, speckleRange 2, disp12MaxDiff 0, P1 = 8*121, P2 = 32*121, default mode.
    """

    def __init__(self, cfg=None):
        if cfg is None:
            cfg = {}
        self.cfg = cfg
        self.max_size = self.cfg.get("max_size", 1000)
        block_size = int(self.cfg.get("blockSize", 11))
        min_disp = int(self.cfg.get("minDisparity", 2))
        num_disp = int(self.cfg.get("numDisparities", 220 - 2))
        self.stereo_sgbm = StereoSGBM_create(
            minDisparity=min_disp,
            numDisparities=num_disp,
            blockSize=block_size,
            uniquenessRatio=self.cfg.get("uniquenessRatio", 5),
            speckleWindowSize=self.cfg.get("speckleWindowSize", 200),
            speckleRange=self.cfg.get("speckleRange", 2),
            disp12MaxDiff=self.cfg.get("disp12MaxDiff", 0),
            P1=self.cfg.get("P1", 8 * 1 * block_size * block_size),
            P2=self.cfg.get("P2", 32 * 1 * block_size * block_size),
            preFilterCap=self.cfg.get("preFilterCap", 0),
            mode=self.cfg.get("mode", MODE_SGBM),
        )

    def compute_disp16(self, img1, img2, batched=False):
        """Device-resident stage used by ``Stereo.get_depth``: int16 disparity*16 of the (possibly
        downsized) pair plus the width it was computed at; torch tensors in, torch tensor out.
        ``batched``: (n, h, w, c) stacks of pairs, one launch per stage."""
        lead = 1 if batched else 0
        h, w = img1.shape[lead:lead + 2]
        resize_ratio = min(self.max_size / max(h, w), 1)
        simg1, simg2 = _resize.resize(img1, resize_ratio, batched), _resize.resize(img2, resize_ratio, batched)
        return self.stereo_sgbm.compute(simg1, simg2), simg1.shape[lead + 1]

    def _disparity_from_disp16(self, sdisp16, hw, sw, batched=False):
        # stereo_matching.py:63-69: float32, clip at 0, below minDisparity -> 0, /16, back to the input size, x w/sw
        import torch
        sdisparity = sdisp16.to(torch.float32).clamp_(min=0)
        sdisparity[sdisparity < self.stereo_sgbm.getMinDisparity() * 16] = 0
        up = _resize.resize(sdisparity / 16.0, hw, batched) * hw[1]  # (/16 is exact in any form)
        # NumPy's `x * w / sw` divides; torch turns a division by a Python number into a multiplication by its
        # reciprocal (one ulp off now and then), a tensor divisor gets the IEEE division
        return up / torch.full((), float(sw), dtype=torch.float32, device=up.device)

    def call_batch(self, imgs1, imgs2):
        """``__call__`` for (n, h, w, 3) CUDA stacks of rectified pairs -> (n, h, w) float32 disparities; pair i equals
        ``self(imgs1[i], imgs2[i])``.  Not in the reference (one pair per call); used by ``Stereo.get_depth_batch``."""
        hw = tuple(imgs1.shape[1:3])
        sdisp16, sw = self.compute_disp16(imgs1, imgs2, batched=True)
        return self._disparity_from_disp16(sdisp16, hw, sw, batched=True)

    def __call__(self, img1, img2):
        was_np = is_np(img1)
        if was_np:
            img1, img2 = to_device(img1), to_device(img2)
        sdisp16, sw = self.compute_disp16(img1, img2)
        return to_caller(self._disparity_from_disp16(sdisp16, tuple(img1.shape[:2]), sw), was_np)


class FeatureMatchingAsStereoMatching(MetaStereoMatching):
    """Sparse matches made dense (stereo_matching.py:113-142): ``feature_matching(img1, img2)`` returns a dict with
    normalised ``uvs1``, ``uvs2`` (n, 2) in [0, 1); they are scaled to the grid ``cfg.get("shape", hw) // downscale``,
    (u1, v1, u1 - u2) is filled with ``sparse.interpolate_uvzs(..., inter_type="nearest")`` and, when the grid is not
    the image, blown up to ``hw`` by nearest-neighbour times ``hw[1] / grid[1]`` -- one kernel writes the full-size image.
    Returns ``dict(disparity=float32 (h, w), matched=<the matcher's dict>)``.

    ``downscale`` (not in the reference, which hard-codes 8 because its KDTree fill took 44 s at full resolution):
    ``downscale=1`` fills at full resolution.  ``uvs*`` may be NumPy arrays or CUDA tensors; tensors stay on the device
    and the disparity comes back as a tensor.

    ``inter_type`` (not in the reference either): ``"nearest"`` is the reference's fill; ``"rbf"`` fills the grid with
    the thin-plate spline ``sparse.interpolate_uvzs_rbf`` -- smooth instead of Voronoi blocks, float64, at most
    ``sparse.MAX_SPLINE_POINTS`` matches -- and blows it up the same way (``sparse.spline_upsize``)."""

    accepts_device_tensors = True

    def __init__(self, feature_matching, downscale=8, inter_type="nearest"):
        self.feature_matching = feature_matching
        self.downscale = int(downscale)
        if self.downscale < 1:
            raise ValueError("downscale must be a positive integer, got %r" % (downscale,))
        if inter_type not in ("nearest", "rbf"):
            raise ValueError('inter_type must be "nearest" or "rbf", got %r' % (inter_type,))
        self.inter_type = inter_type

    def __call__(self, img1, img2):
        from . import sparse
        matched = self.feature_matching(img1, img2)
        hw = tuple(int(v) for v in img1.shape[:2])
        resize_shape = self.feature_matching.cfg.get("shape", hw)
        resize_shape = (resize_shape[0] // self.downscale, resize_shape[1] // self.downscale)
        uvs1, uvs2 = matched["uvs1"], matched["uvs2"]
        if isinstance(uvs1, np.ndarray):
            uvs1, uvs2 = uvs1 * resize_shape[::-1], np.asarray(uvs2) * resize_shape[::-1]
            uvds = np.concatenate((uvs1, (uvs1 - uvs2)[:, :1]), 1)
        else:
            import torch
            scale = torch.tensor(resize_shape[::-1], dtype=torch.float64, device=uvs1.device)
            uvs1 = uvs1.to(torch.float64) * scale  # (float64 like NumPy's float * int tuple)
            uvs2 = torch.as_tensor(uvs2, device=uvs1.device).to(torch.float64) * scale
            uvds = torch.cat((uvs1, (uvs1 - uvs2)[:, :1]), 1)
        if self.inter_type == "rbf":
            disparity = sparse.interpolate_uvzs_rbf(uvds, resize_shape)
            if resize_shape != hw:
                disparity = sparse.spline_upsize(disparity, hw)
            return dict(disparity=disparity, matched=matched)
        disparity = sparse.interpolate_uvzs(uvds, resize_shape, constrained_type=None, inter_type="nearest",
                                            resize_hw=hw if resize_shape != hw else None)
        return dict(disparity=disparity, matched=matched)


class MatchingByBoard(MetaStereoMatching):
    """The disparity of a calibration board seen in both rectified images, from its image points
    (stereo_matching.py:73-110): ground truth for a matcher.  ``board.find_image_points`` runs on both images; the points
    are ndarrays or the reference's id -> points dicts (joined by their sorted common keys).  ``(x1, y1, x1 - x2)`` is
    scattered into an image (last writer wins) and, with ``dense_predict``, ``1 / fill(1 / sparse)`` inside the points'
    convex hull by ``sparse.interpolate_sparse2d_in_hull`` (``+inf`` outside the hull, as in the reference).  Returns
    ``dict(disparity, rectify_std)``: rectify_std is the standard deviation of ``y2 - y1``, 0 for a perfect rectification.

    Not the reference's: where either image shows no board the reference dies with ``KeyError``; here the disparity is
    all zeros and ``rectify_std`` is NaN.  CUDA images stay on the device and the disparity comes back as a tensor."""

    accepts_device_tensors = True

    def __init__(self, board, dense_predict=True):
        self.board = board
        self.dense_predict = dense_predict

    def __call__(self, img1, img2):
        from . import sparse
        d1, d2 = dict(img=img1), dict(img=img2)
        self.board.find_image_points(d1)
        self.board.find_image_points(d2)
        hw = tuple(int(v) for v in img1.shape[:2])
        was_np = is_np(img1)
        points1, points2 = d1.get("image_points"), d2.get("image_points")
        if isinstance(points1, dict) and isinstance(points2, dict):
            keys = sorted(set(points1).intersection(points2))
            points1 = np.concatenate([points1[k] for k in keys], 0) if keys else None
            points2 = np.concatenate([points2[k] for k in keys], 0) if keys else None
        if points1 is None or points2 is None or not len(points1):
            if was_np:
                return dict(disparity=np.zeros(hw, np.float32), rectify_std=float("nan"))
            import torch
            return dict(disparity=torch.zeros(hw, dtype=torch.float32, device=img1.device), rectify_std=float("nan"))
        points1, points2 = np.asarray(points1), np.asarray(points2)
        rectify_std = np.std((points2 - points1)[:, 1])
        point_disps = (points1 - points2)[:, 0]
        xyds = np.append(points1, point_disps[:, None], axis=-1)
        if not was_np:
            import torch
            xyds = torch.from_numpy(np.ascontiguousarray(xyds)).to(img1.device)
        sparse_disp = sparse.uvzs_to_arr2d(xyds, hw)
        if self.dense_predict:
            with np.errstate(divide="ignore"):  # (1 / 0 = inf marks the pixels without a sample, as in the reference)
                disparity = sparse.interpolate_sparse2d_in_hull(1 / sparse_disp, reciprocal=True)
        else:
            disparity = sparse_disp
        return dict(disparity=disparity, rectify_std=rectify_std)
