"""cv2-shaped front ends of the remap / filter / depth kernels (host side: torch tensors in HBM).

Each function names the cv2 / NumPy call of the reference it stands in for; all of them work on
torch CUDA tensors (zero-copy) or NumPy arrays (copied to the GPU and back).
"""
import ctypes
import sys

import numpy as np

from . import _arrays, _frames, _native, detect
from ._arrays import DIST_COUNTS, FLOAT_TYPES, K9, check_array, dist, dtype_name, is_np, mat, to_caller, to_device
from ._native import INTER_LANCZOS4, INTER_LINEAR, INTER_NEAREST, call

from ._frames import GRAY_WEIGHTS, cvt_gray  # noqa: F401  (the public names of ``_frames`` and ``detect`` stay reachable here)
from .detect import (  # noqa: F401
    CHARUCO_FEW, CHARUCO_MAX_BOARDS, CHARUCO_MAX_IDS, CHARUCO_MAX_RATIO_DEN, CHARUCO_MAX_SQUARES, CHARUCO_MIN_SQUARES,
    CHARUCO_NO_CONSENSUS, CHARUCO_NO_LATTICE, CHARUCO_OVERFLOW, CHESS_CAPACITY, CHESS_FEW, CHESS_INCOMPLETE, CHESS_MAX_CORNERS,
    CHESS_MAX_NMS_RADIUS, CHESS_MAX_RELATIVE, CHESS_MAX_SIDE, CHESS_OVERFLOW, MARKER_CAPACITY, MARKER_MAX_BOX, MARKER_MAX_RADIUS,
    MARKER_MIN_SIDE, MARKER_OVERFLOW, MARKER_REFINE_CRITERIA, SUBPIX_BAD_START, SUBPIX_LEFT_IMAGE,
    SUBPIX_MAX_ITERATIONS, SUBPIX_REVERTED, SUBPIX_SINGULAR, TERM_CRITERIA_COUNT, TERM_CRITERIA_EPS, chess_peaks, chess_response,
    corner_sub_pix, dark_mask, find_charuco_boards, find_charuco_corners, find_chessboard_corners, find_markers, label_components,
    laplacian_sums, sharpness, sub_pix_criteria, sub_pix_mask)


# The two documented switches, ``imgproc.GRAY_BITS`` and ``imgproc.MARKER_PLANE_BUDGET``: each has ONE value, in the module whose code reads
# it at call time (a re-export would be a copy that assigning changes nothing by), so they are properties of this module's class.
class _Switches(type(sys)):
    GRAY_BITS = property(lambda m: _frames.GRAY_BITS, lambda m, v: setattr(_frames, "GRAY_BITS", v))
    MARKER_PLANE_BUDGET = property(lambda m: detect.MARKER_PLANE_BUDGET, lambda m, v: setattr(detect, "MARKER_PLANE_BUDGET", v))


sys.modules[__name__].__class__ = _Switches


def _img_dims(t):
    """(batch, h, w, cn, batched) of a (h,w) | (h,w,c) | (n,h,w,c) uint8 image tensor."""
    if t.dim() == 2:
        return 1, t.shape[0], t.shape[1], 1, False
    if t.dim() == 3:
        return 1, t.shape[0], t.shape[1], t.shape[2], False
    if t.dim() == 4:
        return t.shape[0], t.shape[1], t.shape[2], t.shape[3], True
    raise ValueError("unsupported image shape %s" % (tuple(t.shape),))


def remap(src, mapx, mapy, interpolation=INTER_LANCZOS4, x_shift=0):
    """cv2.remap(src, mapx, mapy, interpolation) for uint8 images, CV_32FC1 maps, BORDER_CONSTANT 0
    (stereo_camera.py:217-228).  ``x_shift`` fuses stereo_camera.py:230-240."""
    import torch
    s, was_np = to_device(src, dtype="uint8"), is_np(src)
    mx = to_device(mapx, dtype="float32")
    my = to_device(mapy, dtype="float32")
    if mx.shape != my.shape or mx.dim() != 2:
        raise ValueError("mapx / mapy must be 2-D float32 arrays of equal shape")
    n, sh, sw, cn, batched = _img_dims(s)
    dh, dw = mx.shape
    shape = (n, dh, dw) + ((cn,) if s.dim() > 2 else ())
    dst = torch.empty(shape, dtype=torch.uint8, device=s.device)
    call("camd_remap_u8", s.device, s.data_ptr(), sw, sh, cn, sw * cn, sh * sw * cn, mx.data_ptr(), my.data_ptr(),
         dst.data_ptr(), dw, dh, dw * cn, dh * dw * cn, int(interpolation), int(x_shift), n, what="remap")
    return to_caller(dst if batched else dst[0], was_np)


def init_undistort_rectify_map(A, dist, R, Anew, size, valid_for=None, device=None):
    """cv2.initUndistortRectifyMap(A, dist, R, Anew, size, CV_32FC1) built on the GPU
    (stereo_camera.py:159-165, utils.py:184-191): returns (mapx, mapy) float32 CUDA tensors (h, w), plus
    the uint8 valid mask of stereo_camera.py:167-176 when ``valid_for=(src_w, src_h)`` is given."""
    import torch
    _native.require_device()
    w, h = int(size[0]), int(size[1])
    A, Anew = mat(A, 9), K9(Anew)
    Rm = None if R is None else mat(R, 9)
    D, dptr, nd = _arrays.dist(dist)  # (the parameter shadows the helper's name)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    mapx = torch.empty((h, w), dtype=torch.float32, device=dev)
    mapy = torch.empty((h, w), dtype=torch.float32, device=dev)
    mask = torch.empty((h, w), dtype=torch.uint8, device=dev) if valid_for is not None else None
    sw, sh = (int(valid_for[0]), int(valid_for[1])) if valid_for is not None else (0, 0)
    call("camd_init_undistort_rectify_map", dev, A.ctypes.data, dptr, nd, None if Rm is None else Rm.ctypes.data,
         Anew.ctypes.data, w, h, mapx.data_ptr(), mapy.data_ptr(), None if mask is None else mask.data_ptr(), sw, sh,
         what="init_undistort_rectify_map")
    return (mapx, mapy) if mask is None else (mapx, mapy, mask)


def undistort_maps_device(K, D, size, device=None):
    """The CV_16SC2 + CV_16UC1 maps of cv2.undistort, built on the GPU: (mapxy int16 (h,w,2), mapa int16 view)."""
    import torch
    _native.require_device()
    w, h = int(size[0]), int(size[1])
    K = mat(K, 9)
    D, dptr, nd = dist(D)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    mxy = torch.empty((h, w, 2), dtype=torch.int16, device=dev)
    ma = torch.empty((h, w), dtype=torch.int16, device=dev)  # uint16 bit patterns (torch has no uint16 arithmetic)
    call("camd_undistort_maps", dev, K.ctypes.data, dptr, nd, w, h, mxy.data_ptr(), ma.data_ptr(), what="undistort_maps")
    return mxy, ma


def undistort_maps(K, D, size):
    """The CV_16SC2 + CV_16UC1 maps cv2.undistort(img, K, D) builds internally (host, init time)."""
    w, h = int(size[0]), int(size[1])
    K = mat(K, 9)
    D, dptr, nd = dist(D)
    mxy = np.empty((h, w, 2), np.int16)
    ma = np.empty((h, w), np.uint16)
    rc = _native.lib().camd_undistort_maps_host(K.ctypes.data, dptr, nd, w, h, mxy.ctypes.data, ma.ctypes.data)
    _native.check(rc, "undistort_maps")
    return mxy, ma


def remap_fixed_bilinear(src, mapxy, mapa):
    """cv2.remap(src, map16SC2, map16UC1, INTER_LINEAR): the second half of cv2.undistort
    (stereo_camera.py:430-431)."""
    import torch
    s, was_np = to_device(src, dtype="uint8"), is_np(src)
    mxy = to_device(mapxy, dtype="int16")
    ma = to_device(mapa.view(np.int16) if is_np(mapa) else mapa, dtype="int16")
    n, sh, sw, cn, batched = _img_dims(s)
    dh, dw = ma.shape
    shape = (n, dh, dw) + ((cn,) if s.dim() > 2 else ())
    dst = torch.empty(shape, dtype=torch.uint8, device=s.device)
    call("camd_remap_fixed_bilinear_u8", s.device, s.data_ptr(), sw, sh, cn, sw * cn, sh * sw * cn, mxy.data_ptr(),
         ma.data_ptr(), dst.data_ptr(), dw, dh, dw * cn, dh * dw * cn, n, what="remap_fixed_bilinear")
    return to_caller(dst if batched else dst[0], was_np)


def medianBlur3_s16(disp):
    """cv2.medianBlur(disp, 3) on int16 (the unconditional tail of StereoSGBM.compute)."""
    import torch
    s, was_np = to_device(disp, dtype="int16"), is_np(disp)
    h, w = s.shape[-2:]
    n = s.numel() // (h * w)
    dst = torch.empty_like(s)
    call("camd_median3_s16", s.device, s.data_ptr(), dst.data_ptr(), w, h, n, what="medianBlur3_s16")
    return to_caller(dst, was_np)


def filterSpeckles(disp, newVal, maxSpeckleSize, maxDiff):
    """cv2.filterSpeckles(disp, newVal, maxSpeckleSize, maxDiff) on int16; returns a new array."""
    import torch
    s, was_np = to_device(disp, dtype="int16"), is_np(disp)
    s = s.clone()
    h, w = s.shape[-2:]
    n = s.numel() // (h * w)
    ws = torch.empty(_native.lib().camd_speckle_workspace_bytes(w, h, n), dtype=torch.uint8, device=s.device)
    call("camd_filter_speckles_s16", s.device, s.data_ptr(), w, h, int(newVal), int(maxSpeckleSize), int(maxDiff),
         ws.data_ptr(), n, what="filterSpeckles")
    return to_caller(s, was_np)


def disp_to_depth(disp16, valid_mask, sgbm_min_disparity, add_min_disparity, translate, baseline_fx,
                  max_depth):
    """stereo_matching.py:63-69 + stereo_camera.py:510-513 in one pass.
    Returns (disparity float32, rectify_depth float64)."""
    import torch
    d, was_np = to_device(disp16, dtype="int16"), is_np(disp16)
    m = to_device(valid_mask.view(np.uint8) if is_np(valid_mask) and valid_mask.dtype == bool else valid_mask)
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    h, w = d.shape[-2:]
    n = d.numel() // (h * w)
    disparity = torch.empty(d.shape, dtype=torch.float32, device=d.device)
    depth = torch.empty(d.shape, dtype=torch.float64, device=d.device)
    call("camd_disp_to_depth", d.device, d.data_ptr(), m.data_ptr(), w, h, int(sgbm_min_disparity), int(add_min_disparity),
         int(bool(translate)), ctypes.c_double(baseline_fx), ctypes.c_double(max_depth), disparity.data_ptr(),
         depth.data_ptr(), n, what="disp_to_depth")
    return to_caller((disparity, depth), was_np)


def disp16_resized_to_depth(sdisp16, hw, valid_mask, sgbm_min_disparity, add_min_disparity, translate, baseline_fx,
                            max_depth):
    """The matcher's downsizing branch (stereo_matching.py:63-69 with max_size < image) + stereo_camera.py:510-513 +
    :408-413 in one pass: ``sdisp16`` is the int16 disparity of the downsized pair(s), ``hw`` the rectified size.
    Returns (disparity float32, rectify_depth float64) at ``hw``.  CUDA tensors only."""
    import torch
    d = to_device(sdisp16, dtype="int16")
    m = to_device(valid_mask)
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    sh, sw = d.shape[-2:]
    n = d.numel() // (sh * sw)
    h, w = int(hw[0]), int(hw[1])
    disparity = torch.empty(d.shape[:-2] + (h, w), dtype=torch.float32, device=d.device)
    depth = torch.empty(d.shape[:-2] + (h, w), dtype=torch.float64, device=d.device)
    call("camd_disp16_resized_to_depth", d.device, d.data_ptr(), sw, sh, m.data_ptr(), w, h, int(sgbm_min_disparity),
         int(add_min_disparity), int(bool(translate)), ctypes.c_double(baseline_fx), ctypes.c_double(max_depth),
         disparity.data_ptr(), depth.data_ptr(), n, what="disp16_resized_to_depth")
    return disparity, depth


def unrectify_depth(depth, M_row2, mapx, mapy):
    """utils.rotate_depth_by_remap (utils.py:192-199): z-rescale + INTER_NEAREST remap, float64."""
    import torch
    z, was_np = to_device(depth, dtype="float64"), is_np(depth)
    mx = to_device(mapx, dtype="float32")
    my = to_device(mapy, dtype="float32")
    h, w = z.shape[-2:]
    n = z.numel() // (h * w)
    oh, ow = mx.shape
    M = (ctypes.c_double * 3)(*[float(v) for v in np.asarray(M_row2).reshape(3)])
    out = torch.empty(z.shape[:-2] + (oh, ow), dtype=torch.float64, device=z.device)
    call("camd_unrectify_depth", z.device, z.data_ptr(), w, h, M, mx.data_ptr(), my.data_ptr(), out.data_ptr(), ow, oh, n,
         what="unrectify_depth")
    return to_caller(out, was_np)


def check_distortion(D):
    """The distortion vector as the kernels take it (float64, flat, up to 14 entries); tilted-sensor coefficients
    (tauX, tauY = D[12:14]) are refused here, before any device call, as everywhere else in the library."""
    D = dist(D)[0]
    if D.size > 14:
        raise ValueError("%d distortion coefficients; cv2's model has at most 14" % D.size)
    if D.size > 12 and (D[12:] != 0).any():
        raise ValueError("tilted-sensor distortion (tauX, tauY) not implemented")
    return D


def _cv2_distortion(D):
    """``dist`` of a vector that passed ``check_distortion`` and has one of the lengths cv2 takes."""
    D = check_distortion(D)
    if D.size not in DIST_COUNTS:
        raise ValueError("%d distortion coefficients; cv2 takes 4, 5, 8, 12 or 14" % D.size)
    return dist(D)


def _point_rows(a, width, what):
    """The (n, width) rows of ``a`` = (n, width) or (n, 1, width), float32 / float64, ndarray or CUDA tensor -- checked
    before the device is touched -- as (CUDA tensor whose rows are read in place, row stride in elements, was_numpy).
    A tensor whose rows are the leading columns of wider rows (``uvzs[:, :2]``, ``xyzuv[:, :3]``) is not copied."""
    check_array(a, what)
    was_np = is_np(a)
    if dtype_name(a) not in FLOAT_TYPES:
        raise ValueError("%s must be float32 or float64 (cv2 takes nothing else), got %s" % (what, a.dtype))
    if a.ndim == 3 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError("%s must be (n, %d) or (n, 1, %d), got %s" % (what, width, width, tuple(a.shape)))
    if a.shape[0] >= 2 ** 31:
        raise ValueError("%s: %d rows, the kernels take fewer than 2^31" % (what, a.shape[0]))
    if was_np:
        return to_device(a), width, True
    n = a.shape[0]
    if a.stride(1) != 1 or (n > 1 and not width <= a.stride(0) < 2 ** 31):
        a = a.contiguous()
    return a, (int(a.stride(0)) if n > 1 else width), False


def undistort_points(uvs, K, D=None, iters=5, pixels=False):
    """cv2.undistortPoints(uvs, K, D)[:, 0] (camera.py:286; no R, no P) on the GPU: pixels of the raw image, (n, 2) or
    (n, 1, 2), float32 or float64 -> the normalised pinhole coordinates (n, 2) in the same type.  ``iters`` (1 .. 100)
    rounds of cv2's fixed-point iteration, 5 as in cv2, which tests no epsilon here.  NumPy in -> NumPy out; a CUDA
    tensor -> a tensor on its device and the current stream, its rows read in place (no copy for ``uvzs[:, :2]``).
    ``pixels=True``: the points go back to pixels of the undistorted camera in the same kernel, normalised * [fx, fy] +
    [cx, cy] in float64 -> (n, 2) float64 whatever the input's type: the whole of ``Cam.undistort_points``."""
    import torch
    D, dptr, nd = _cv2_distortion(D)
    if int(iters) != iters or not 1 <= iters <= 100:
        raise ValueError("iters must be an integer in 1 .. 100, got %r" % (iters,))
    K = K9(K)
    t, stride, was_np = _point_rows(uvs, 2, "uvs")
    out = torch.empty((t.shape[0], 2), dtype=torch.float64 if pixels else t.dtype, device=t.device)
    if t.shape[0]:
        uv_type = FLOAT_TYPES[dtype_name(t)]
        out_type = _native.VALUE_F64 | _native.POINTS_PIXELS if pixels else uv_type
        call("camd_undistort_points", t.device, t.data_ptr(), uv_type, t.shape[0], stride, K.ctypes.data, dptr, nd, int(iters),
             out.data_ptr(), out_type, what="undistort_points")
    return to_caller(out, was_np)


def project_points(xyzs, rvec_or_R, tvec, K, D=None):
    """cv2.projectPoints(xyzs, rvec, tvec, K, D)[0][:, 0] (camera.py:280) on the GPU: points (n, 3) or (n, 1, 3), float32
    or float64 -> their pixels (n, 2) in the same type.  ``rvec_or_R``: a Rodrigues vector (turned into its matrix on the
    host, ``geometry.rodrigues``) or a 3x3 matrix; ``tvec``: 3 numbers.  NumPy in -> NumPy out; a CUDA tensor -> a tensor
    on its device and the current stream, its rows read in place (no copy for ``xyzuv[:, :3]``)."""
    import torch
    from . import geometry
    D, dptr, nd = _cv2_distortion(D)
    R = np.asarray(rvec_or_R, np.float64)
    if R.size not in (3, 9):
        raise ValueError("rvec_or_R must be a Rodrigues vector or a 3x3 matrix, got shape %s" % (R.shape,))
    R = mat(geometry.rodrigues(R) if R.size == 3 else R, 9)
    tv = np.ascontiguousarray(tvec, np.float64).reshape(-1)
    if tv.size != 3:
        raise ValueError("tvec must hold 3 numbers, got %d" % tv.size)
    K = K9(K)
    t, stride, was_np = _point_rows(xyzs, 3, "xyzs")
    out = torch.empty((t.shape[0], 2), dtype=t.dtype, device=t.device)
    if t.shape[0]:
        call("camd_project_points", t.device, t.data_ptr(), FLOAT_TYPES[dtype_name(t)], t.shape[0], stride, R.ctypes.data,
             tv.ctypes.data, K.ctypes.data, dptr, nd, out.data_ptr(), what="project_points")
    return to_caller(out, was_np)


def distort_index_map(K, D, size, device=None):
    """The per-rig part of ``Stereo.distort_depth`` (stereo_camera.py:440-462) built on the GPU: an int32 CUDA tensor
    (h, w) whose entry [y, x] is the row-major index of the FIRST pixel of the undistorted image that
    cv2.undistortPoints -> cv2.projectPoints -> .astype(np.int32) sends to (x, y) -- what np.unique(axis=0,
    return_index=True) picks -- or -1 where none lands.

    A rig with a target outside the image raises ``IndexError`` (the one synchronisation of this table: its counters
    are read here, once).  The reference raises it too for targets >= w / >= h and silently wraps negative ones to the
    far edge (NumPy's negative indexing); here both sides are refused."""
    import torch
    D, dptr, nd = dist(check_distortion(D))
    w, h = int(size[0]), int(size[1])
    if w <= 0 or h <= 0:
        raise ValueError("image size must be positive, got %s" % ((w, h),))
    K = K9(K)
    _native.require_device()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = torch.empty((h, w), dtype=torch.int32, device=dev)
    stats = torch.empty(6, dtype=torch.int32, device=dev)
    call("camd_distort_index_map", dev, K.ctypes.data, dptr, nd, w, h, idx.data_ptr(), stats.data_ptr(),
         what="distort_index_map")
    n_out, min_u, max_u, min_v, max_v, n_nonfinite = (int(v) for v in stats.cpu())
    if n_out:
        where = "U in [%d, %d], V in [%d, %d]" % (min_u, max_u, min_v, max_v) if min_u <= max_u else "no finite target"
        raise IndexError("distort_depth: %d of %d pixels of the undistorted image land outside the %dx%d distorted image "
                         "(%s; %d of them not finite) -- the reference raises IndexError for targets beyond the far edges "
                         "and wraps negative ones around; this rig is refused" % (n_out, w * h, w, h, where, n_nonfinite))
    return idx


def distort_depth(depth, src_index):
    """stereo_camera.py:438,463 (``res = zeros; res[y, x] = depths[index]``) as one gather through ``src_index``
    (``distort_index_map``): depth (h, w) or (n, h, w), float64 or float32 -> the same shape and dtype; holes are 0."""
    import torch
    idx = to_device(src_index, dtype="int32")
    z, was_np = to_device(depth), is_np(depth)
    if z.dtype not in (torch.float64, torch.float32):
        raise ValueError("depth must be float64 or float32, got %s" % z.dtype)
    if idx.dim() != 2 or z.dim() not in (2, 3) or tuple(z.shape[-2:]) != tuple(idx.shape):
        raise ValueError("depth %s does not match the %s index table: expected (h, w) or (n, h, w)"
                         % (tuple(z.shape), tuple(idx.shape)))
    if idx.device != z.device:
        raise ValueError("the index table lives on %s, the depth on %s" % (idx.device, z.device))
    h, w = idx.shape
    out = torch.empty_like(z)
    if z.numel():
        call("camd_distort_depth", z.device, z.data_ptr(), z.element_size(), w, h, idx.data_ptr(), out.data_ptr(),
             z.numel() // (h * w), what="distort_depth")
    return to_caller(out, was_np)
