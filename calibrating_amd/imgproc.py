"""cv2-shaped front ends of the remap / filter / depth kernels (host side: torch tensors in HBM).

Each function names the cv2 / NumPy call of the reference it stands in for; all of them work on
torch CUDA tensors (zero-copy) or NumPy arrays (copied to the GPU and back).
"""
import ctypes

import numpy as np

from . import _arrays, _native
from ._arrays import DIST_COUNTS, FLOAT_TYPES, K9, check_array, dist, dtype_name, is_np, mat, to_caller, to_device
from ._native import INTER_LANCZOS4, INTER_LINEAR, INTER_NEAREST, call


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


# ---- gray images and corners refined to sub-pixel (boards.py:156-172; csrc/subpix.hip) ----
# cv2's fixed-point weights of B, G, R and their shift, by the bits of the fixed point (recalled,
# unpinned).  OpenCV 4.x: 15 bits, older releases: 14.  GRAY_BITS is the switch.
GRAY_WEIGHTS = {15: (3735, 19235, 9798), 14: (1868, 9617, 4899)}
GRAY_BITS = 15
SUBPIX_SINGULAR, SUBPIX_LEFT_IMAGE, SUBPIX_REVERTED, SUBPIX_BAD_START = 1, 2, 4, 8  # bits of corner_sub_pix's status
SUBPIX_MAX_ITERATIONS = 100
TERM_CRITERIA_COUNT, TERM_CRITERIA_EPS = 1, 2  # cv2.TERM_CRITERIA_MAX_ITER, cv2.TERM_CRITERIA_EPS


def _image_rows(t, channels):
    """(batch, h, w, pitch, stride) in bytes of a uint8 CUDA tensor (h, w[, 3]) or (f, h, w[, 3]) whose pixels are
    contiguous; rows and images may be apart by more than their bytes (a crop, a slice of a wider batch)."""
    lead = t.dim() - (3 if channels == 3 else 2)
    h, w = int(t.shape[lead]), int(t.shape[lead + 1])
    f = int(t.shape[0]) if lead else 1
    st = t.stride()
    tight = (st[-1] == 1 and st[-2] == 3) if channels == 3 else st[-1] == 1
    pitch = int(st[lead]) if h > 1 else w * channels
    stride = int(st[0]) if lead and f > 1 else h * pitch
    if not tight or pitch < w * channels or stride < (h - 1) * pitch + w * channels:
        t = t.contiguous()
        pitch, stride = w * channels, h * w * channels
    return t, f, h, w, pitch, stride


def _check_image(img, what):
    check_array(img, what)
    if dtype_name(img) != "uint8":
        raise ValueError("%s must be uint8, got %s" % (what, img.dtype))


def _to_image(img):
    """The CUDA tensor of an image: an ndarray is uploaded, a tensor is taken as it is (pitched views are read in place)."""
    import torch
    if is_np(img):
        _native.require_device()
        return torch.from_numpy(np.ascontiguousarray(img)).cuda()
    return img


def cvt_gray(img, code="bgr"):
    """cv2.cvtColor(img, cv2.COLOR_BGR2GRAY) (``code="bgr"``) or COLOR_RGB2GRAY (``"rgb"``) on uint8, on the GPU:
    (h, w, 3) or (f, h, w, 3) -> (h, w) or (f, h, w).  The first channel gets blue's weight with "bgr" and red's with
    "rgb"; the reference hands an RGB image to COLOR_BGR2GRAY (boards.py:159), which ``Chessboard`` repeats.  Weights:
    ``GRAY_WEIGHTS[GRAY_BITS]`` (U32).  A tensor whose rows or images are apart (a crop) is read in place."""
    import torch
    _check_image(img, "img")
    if code not in ("bgr", "rgb"):
        raise ValueError("code must be 'bgr' or 'rgb', got %r" % (code,))
    if img.ndim not in (3, 4) or img.shape[-1] != 3:
        raise ValueError("img must be (h, w, 3) or (f, h, w, 3), got %s" % (tuple(img.shape),))
    if 0 in tuple(img.shape):
        raise ValueError("img is empty: %s" % (tuple(img.shape),))
    was_np = is_np(img)
    t, f, h, w, pitch, stride = _image_rows(_to_image(img), 3)
    by, gy, ry = GRAY_WEIGHTS[GRAY_BITS]
    k = (by, gy, ry) if code == "bgr" else (ry, gy, by)
    dst = torch.empty((f, h, w), dtype=torch.uint8, device=t.device)
    call("camd_bgr_to_gray_u8", t.device, t.data_ptr(), w, h, pitch, stride, dst.data_ptr(), w, h * w, f, k[0], k[1], k[2],
         GRAY_BITS, what="cvt_gray")
    return to_caller(dst if img.ndim == 4 else dst[0], was_np)


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
    """(rows (N, 2) view, lengths or None for a dense batch, the shape the result takes)."""
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
    _check_image(images, "images")
    check_array(corners, "corners")
    if is_np(images) != is_np(corners):
        raise TypeError("images and corners must both be NumPy arrays or both be CUDA tensors")
    if dtype_name(corners) not in FLOAT_TYPES:
        raise ValueError("corners must be float32 or float64, got %s" % corners.dtype)
    colour = images.ndim in (3, 4) and images.shape[-1] == 3  # (no gray image is 3 wide: the smallest window needs 7)
    if images.ndim not in (2, 3, 4) or (images.ndim == 4 and not colour):
        raise ValueError("images must be (h, w), (f, h, w), (h, w, 3) or (f, h, w, 3), got %s" % (tuple(images.shape),))
    frames = int(images.shape[0]) if images.ndim - (1 if colour else 0) == 3 else 1
    lengths = _corner_layout(corners, counts, frames)
    ww, wh = int(win[0]), int(win[1])
    zone = (int(zero_zone[0]), int(zero_zone[1]))
    if ww <= 0 or wh <= 0:
        raise ValueError("win must be a pair of positive half-sizes, got %r" % (win,))
    max_iters, eps = sub_pix_criteria(criteria)
    was_np = is_np(images)
    gray = cvt_gray(_to_image(images), "bgr") if colour else _to_image(images)
    gray, f, h, w, pitch, stride = _image_rows(gray, 1)
    if w < 2 * ww + 5 or h < 2 * wh + 5:
        raise ValueError("a %d x %d image is smaller than the %d x %d a window of %r needs" % (w, h, 2 * ww + 5, 2 * wh + 5, (ww, wh)))
    rows = to_device(corners, device=gray.device).reshape(-1, 2)
    n = int(rows.shape[0])
    out = torch.empty_like(rows)
    iterations = torch.empty(n, dtype=torch.int32, device=gray.device)
    status = torch.empty(n, dtype=torch.int32, device=gray.device)
    start = None
    if lengths is not None:
        start = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(gray.device)
    mask_t = _device_mask((ww, wh), zone, gray.device)
    call("camd_corner_sub_pix", gray.device, gray.data_ptr(), w, h, pitch, stride, f, rows.data_ptr(), FLOAT_TYPES[dtype_name(rows)],
         n, None if start is None else start.data_ptr(), ww, wh, mask_t.data_ptr(), max_iters, ctypes.c_double(eps),
         out.data_ptr(), iterations.data_ptr(), status.data_ptr(), what="corner_sub_pix")
    lead = tuple(corners.shape[:-1])
    out = out.reshape(tuple(corners.shape))
    if not return_info:
        return to_caller(out, was_np)
    return to_caller((out, iterations.reshape(lead), status.reshape(lead)), was_np)


# ---- chessboard corners from the image alone (csrc/chessboard.hip; a contract of our own) ----
CHESS_CAPACITY, CHESS_MAX_CORNERS, CHESS_MAX_RELATIVE, CHESS_MAX_NMS_RADIUS, CHESS_MAX_SIDE = 1024, 512, 64, 8, 16384
CHESS_FEW, CHESS_OVERFLOW, CHESS_INCOMPLETE = 1, 2, 4  # find_chessboard_corners' status; 0 = found


def _chess_arguments(pattern, relative, nms_radius):
    """(across, down, relative, nms_radius) as integers within the detector's limits, or ValueError"""
    try:
        across, down = pattern
    except (TypeError, ValueError):
        raise ValueError("pattern must be the inner corners (across, down), got %r" % (pattern,))
    for name, v in (("across", across), ("down", down), ("relative", relative), ("nms_radius", nms_radius)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be an integer, got %r" % (name, v))
    across, down, relative, nms_radius = int(across), int(down), int(relative), int(nms_radius)
    if across < 2 or down < 2 or across * down > CHESS_MAX_CORNERS:
        raise ValueError("a pattern of %d x %d corners; the detector takes across, down >= 2 with at most %d corners"
                         % (across, down, CHESS_MAX_CORNERS))
    if not 1 <= relative <= CHESS_MAX_RELATIVE:
        raise ValueError("relative must be 1 .. %d, got %d" % (CHESS_MAX_RELATIVE, relative))
    if not 1 <= nms_radius <= CHESS_MAX_NMS_RADIUS:
        raise ValueError("nms_radius must be 1 .. %d, got %d" % (CHESS_MAX_NMS_RADIUS, nms_radius))
    return across, down, relative, nms_radius


def _chess_gray(images, what):
    """(gray CUDA tensor, frames, h, w, pitch, stride, batched, was_numpy) of uint8 images (h, w[, 3]) or (f, h, w[, 3]);
    colour goes through ``cvt_gray(code="bgr")``.  Every refusal comes before the device is touched."""
    _check_image(images, what)
    colour = images.ndim in (3, 4) and images.shape[-1] == 3  # (a gray image 3 wide has no pixel 5 from its borders)
    if images.ndim not in (2, 3, 4) or (images.ndim == 4 and not colour):
        raise ValueError("%s must be (h, w), (f, h, w), (h, w, 3) or (f, h, w, 3), got %s" % (what, tuple(images.shape)))
    if 0 in tuple(images.shape):
        raise ValueError("%s is empty: %s" % (what, tuple(images.shape)))
    batched = images.ndim - (1 if colour else 0) == 3
    gray = cvt_gray(_to_image(images), "bgr") if colour else _to_image(images)
    gray, f, h, w, pitch, stride = _image_rows(gray, 1)
    if f * h >= 2 ** 31:
        raise ValueError("%s: %d rows in all, the kernels take fewer than 2^31" % (what, f * h))
    return gray, f, h, w, pitch, stride, batched, is_np(images)


def _chess_response(gray, f, h, w, pitch, stride):
    import torch
    r = torch.empty((f, h, w), dtype=torch.int16, device=gray.device)
    rmax = torch.empty(f, dtype=torch.int32, device=gray.device)
    call("camd_chess_response", gray.device, gray.data_ptr(), w, h, pitch, stride, f, r.data_ptr(), rmax.data_ptr(),
         what="chess_response")
    return r, rmax


def chess_response(images):
    """Stage 1 of the chessboard detector: the ChESS corner response (Bennett & Lasenby) times 5 of every pixel, in
    integers -- ``include/calibrating_amd.h`` states the formula -- -> ``(response, response_max)``: int16 in the shape of
    the gray image(s), 0 within 5 px of a border, and its maximum per frame, int32 (f,) (0-d for one image).  ``images``:
    uint8 gray (h, w) / (f, h, w) or colour (h, w, 3) / (f, h, w, 3) (through ``cvt_gray``), NumPy or CUDA; pitched views
    are read in place."""
    gray, f, h, w, pitch, stride, batched, was_np = _chess_gray(images, "images")
    r, rmax = _chess_response(gray, f, h, w, pitch, stride)
    return to_caller((r, rmax) if batched else (r[0], rmax[0]), was_np)


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
    _, _, relative, nms_radius = _chess_arguments((2, 2), relative, nms_radius)
    check_array(response, "response")
    check_array(response_max, "response_max")
    if is_np(response) != is_np(response_max):
        raise TypeError("response and response_max must both be NumPy arrays or both be CUDA tensors")
    if dtype_name(response) != "int16" or dtype_name(response_max) != "int32":
        raise ValueError("response must be int16 and response_max int32, got %s and %s" % (response.dtype, response_max.dtype))
    if response.ndim != 3 or 0 in tuple(response.shape) or tuple(response_max.shape) != (response.shape[0],):
        raise ValueError("response must be (f, h, w) and response_max (f,), got %s and %s"
                         % (tuple(response.shape), tuple(response_max.shape)))
    if response.shape[0] * response.shape[1] >= 2 ** 31:
        raise ValueError("response: %d rows in all, the kernels take fewer than 2^31" % (response.shape[0] * response.shape[1]))
    r = to_device(response)
    return to_caller(_chess_peaks(r, to_device(response_max, device=r.device), relative, nms_radius), is_np(response))


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
    across, down, relative, nms_radius = _chess_arguments(pattern, relative, nms_radius)
    check_array(images, "images")
    if images.ndim in (2, 3, 4) and max(images.shape[-3:-1] if images.shape[-1] == 3 else images.shape[-2:]) > CHESS_MAX_SIDE:
        raise ValueError("images of %s; the detector takes sides up to %d" % (tuple(images.shape), CHESS_MAX_SIDE))
    gray, f, h, w, pitch, stride, batched, was_np = _chess_gray(images, "images")
    r, rmax = _chess_response(gray, f, h, w, pitch, stride)
    peaks, counts = _chess_peaks(r, rmax, relative, nms_radius)
    corners = torch.empty((f, across * down, 2), dtype=torch.float32, device=gray.device)
    status = torch.empty(f, dtype=torch.int32, device=gray.device)
    call("camd_chess_lattice", gray.device, peaks.data_ptr(), counts.data_ptr(), w, h, f, across, down, corners.data_ptr(),
         status.data_ptr(), what="find_chessboard_corners")
    out = (status == 0, corners, status, counts)
    if not batched:
        out = tuple(v[0] for v in out)
    out = to_caller(out if return_info else out[:2], was_np)
    if was_np and not batched:
        out = (bool(out[0]),) + tuple(out[1:])
    return out


# ---- ChArUco boards, cut or partly covered ones included (csrc/charuco.hip; a contract of our own) ----
CHARUCO_MIN_SQUARES, CHARUCO_MAX_SQUARES, CHARUCO_MAX_RATIO_DEN, CHARUCO_MAX_IDS = 3, 16, 64, 1024
CHARUCO_FEW, CHARUCO_OVERFLOW, CHARUCO_NO_LATTICE, CHARUCO_NO_CONSENSUS = 1, 2, 4, 8  # find_charuco_corners' status; 0 = found


def _charuco_arguments(squares_xy, dictionary, marker_ratio, first_id, relative, nms_radius, min_markers, max_bit_errors):
    """(sx, sy, words (n_ids,) uint64, s, num, den, first_id, relative, nms_radius, min_markers, max_bit_errors) within
    the detector's limits, or ValueError"""
    from . import boards
    try:
        sx, sy = squares_xy
        num, den = marker_ratio
    except (TypeError, ValueError):
        raise ValueError("squares_xy must be the squares (across, down) and marker_ratio two integers (numerator, denominator), "
                         "got %r and %r" % (squares_xy, marker_ratio))
    for name, v in (("squares across", sx), ("squares down", sy), ("the ratio's numerator", num), ("the ratio's denominator", den),
                    ("first_id", first_id), ("min_markers", min_markers), ("max_bit_errors", max_bit_errors)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be an integer, got %r" % (name, v))
    _, _, relative, nms_radius = _chess_arguments((2, 2), relative, nms_radius)
    sx, sy, num, den, first_id, min_markers, max_bit_errors = (int(v) for v in (sx, sy, num, den, first_id, min_markers, max_bit_errors))
    if not (CHARUCO_MIN_SQUARES <= sx <= CHARUCO_MAX_SQUARES and CHARUCO_MIN_SQUARES <= sy <= CHARUCO_MAX_SQUARES):
        raise ValueError("a board of %d x %d squares; the detector takes %d .. %d each way"
                         % (sx, sy, CHARUCO_MIN_SQUARES, CHARUCO_MAX_SQUARES))
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
    sx, sy, words, s, num, den, first_id, relative, nms_radius, min_markers, max_bit_errors = _charuco_arguments(
        squares_xy, dictionary, marker_ratio, first_id, relative, nms_radius, min_markers, max_bit_errors)
    check_array(images, "images")
    if images.ndim in (2, 3, 4) and max(images.shape[-3:-1] if images.shape[-1] == 3 else images.shape[-2:]) > CHESS_MAX_SIDE:
        raise ValueError("images of %s; the detector takes sides up to %d" % (tuple(images.shape), CHESS_MAX_SIDE))
    gray, f, h, w, pitch, stride, batched, was_np = _chess_gray(images, "images")
    if w < 3 or h < 3:
        raise ValueError("images of %d x %d; the detector takes sides from 3" % (w, h))
    r, rmax = _chess_response(gray, f, h, w, pitch, stride)
    peaks, counts = _chess_peaks(r, rmax, relative, nms_radius)
    corners = torch.empty((f, (sx - 1) * (sy - 1), 2), dtype=torch.float32, device=gray.device)
    marker_ids = torch.empty((f, sx * sy), dtype=torch.int32, device=gray.device)
    status = torch.empty(f, dtype=torch.int32, device=gray.device)
    words_t = torch.from_numpy(words.view(np.int64)).to(gray.device)
    call("camd_charuco_detect", gray.device, peaks.data_ptr(), counts.data_ptr(), gray.data_ptr(), w, h, pitch, stride, f, sx, sy,
         num, den, words_t.data_ptr(), len(words), s, first_id, min_markers, max_bit_errors, corners.data_ptr(),
         marker_ids.data_ptr(), status.data_ptr(), what="find_charuco_corners")
    out = (status == 0, corners, marker_ids, status, counts)
    if not batched:
        out = tuple(v[0] for v in out)
    out = to_caller(out if return_info else out[:2], was_np)
    if was_np and not batched:
        out = (bool(out[0]),) + tuple(out[1:])
    return out


# ---- several ChArUco boards of one set in a frame (csrc/charuco.hip, k_charuco_multi) ----
CHARUCO_MAX_BOARDS = 8


def _charuco_set(first_ids, markers, n_ids):
    """the boards' first ids as a list of 1 .. 8 integers whose ranges of ``markers`` ids lie inside the dictionary and
    apart from each other, or ValueError"""
    try:
        ids = list(first_ids)
    except TypeError:
        raise ValueError("first_ids must be the boards' first marker ids, one per board, got %r" % (first_ids,))
    if not 1 <= len(ids) <= CHARUCO_MAX_BOARDS:
        raise ValueError("a set of %d boards; the detector takes 1 .. %d" % (len(ids), CHARUCO_MAX_BOARDS))
    for v in ids:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("first_ids must be integers, got %r" % (v,))
    ids = [int(v) for v in ids]
    for k, a in enumerate(ids):
        if a < 0 or a + markers > n_ids:
            raise ValueError("board %d's %d markers from id %d on do not fit a dictionary of %d ids" % (k, markers, a, n_ids))
        for j, b in enumerate(ids[:k]):
            if a < b + markers and b < a + markers:
                raise ValueError("boards %d and %d share marker ids: %d .. %d and %d .. %d"
                                 % (j, k, b, b + markers - 1, a, a + markers - 1))
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
    sx, sy, words, s, num, den, _, relative, nms_radius, min_markers, max_bit_errors = _charuco_arguments(
        squares_xy, dictionary, marker_ratio, 0, relative, nms_radius, min_markers, max_bit_errors)
    ids = _charuco_set(first_ids, (sx * sy) // 2, len(words))
    check_array(images, "images")
    if images.ndim in (2, 3, 4) and max(images.shape[-3:-1] if images.shape[-1] == 3 else images.shape[-2:]) > CHESS_MAX_SIDE:
        raise ValueError("images of %s; the detector takes sides up to %d" % (tuple(images.shape), CHESS_MAX_SIDE))
    gray, f, h, w, pitch, stride, batched, was_np = _chess_gray(images, "images")
    if w < 3 or h < 3:
        raise ValueError("images of %d x %d; the detector takes sides from 3" % (w, h))
    r, rmax = _chess_response(gray, f, h, w, pitch, stride)
    peaks, counts = _chess_peaks(r, rmax, relative, nms_radius)
    nb = len(ids)
    corners = torch.empty((f, nb, (sx - 1) * (sy - 1), 2), dtype=torch.float32, device=gray.device)
    marker_ids = torch.empty((f, nb, sx * sy), dtype=torch.int32, device=gray.device)
    status = torch.empty((f, nb), dtype=torch.int32, device=gray.device)
    words_t = torch.from_numpy(words.view(np.int64)).to(gray.device)
    board_set = _native.CharucoBoards(nb, (ctypes.c_int * CHARUCO_MAX_BOARDS)(*ids))
    call("camd_charuco_detect_multi", gray.device, peaks.data_ptr(), counts.data_ptr(), gray.data_ptr(), w, h, pitch, stride, f, sx,
         sy, num, den, words_t.data_ptr(), len(words), s, ctypes.byref(board_set), min_markers, max_bit_errors, corners.data_ptr(),
         marker_ids.data_ptr(), status.data_ptr(), what="find_charuco_boards")
    out = (~torch.isnan(corners[..., 0]), corners, marker_ids, status, counts)
    if not batched:
        out = tuple(v[0] for v in out)
    return to_caller(out if return_info else out[:2], was_np)


# ---- stand-alone ArUco markers (csrc/markers.hip; a contract of our own) ----
MARKER_CAPACITY, MARKER_MAX_RADIUS, MARKER_MAX_BOX, MARKER_MIN_SIDE = 1024, 32, 1024, 4
MARKER_OVERFLOW = 2  # find_markers' status bit: more candidates than the 1024 kept, the frame has no markers
MARKER_REFINE_CRITERIA = (30, 0.01)
# the labels of a call (4 B per pixel) and the statistics beside them (16 B) stay within this; beyond it the frames go in chunks
MARKER_PLANE_BUDGET = 1 << 30


def _marker_integers(**named):
    for name, v in named.items():
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be an integer, got %r" % (name, v))
    return tuple(int(v) for v in named.values())


def _mask_arguments(block_radius, offset):
    block_radius, offset = _marker_integers(block_radius=block_radius, offset=offset)
    if not 1 <= block_radius <= MARKER_MAX_RADIUS or not -255 <= offset <= 255:
        raise ValueError("block_radius must be 1 .. %d and offset -255 .. 255, got %d and %d" % (MARKER_MAX_RADIUS, block_radius, offset))
    return block_radius, offset


def _marker_side_limit(shape, colour_ok=True):
    if len(shape) in (2, 3, 4):
        sides = shape[-3:-1] if colour_ok and len(shape) > 2 and shape[-1] == 3 else shape[-2:]
        if max(sides) > CHESS_MAX_SIDE:
            raise ValueError("images of %s; the detector takes sides up to %d" % (tuple(shape), CHESS_MAX_SIDE))


def _dark_mask(gray, f, h, w, pitch, stride, block_radius, offset):
    import torch
    mask = torch.empty((f, h, w), dtype=torch.uint8, device=gray.device)
    call("camd_dark_mask", gray.device, gray.data_ptr(), w, h, pitch, stride, f, block_radius, offset, mask.data_ptr(), what="dark_mask")
    return mask


def dark_mask(images, block_radius=8, offset=7):
    """Stage 1 of the marker detector: uint8 in the shape of the gray image(s), 1 where a pixel is darker than its
    surroundings -- ``(gray + offset) * A < S`` with S the sum of the (2 ``block_radius`` + 1)^2 window about it, clipped to
    the image, and A the pixels of that part.  The inside of a black area wider than the window is not dark.  ``images``:
    uint8 gray (h, w) / (f, h, w) or colour (through ``cvt_gray``), NumPy or CUDA; pitched views are read in place."""
    block_radius, offset = _mask_arguments(block_radius, offset)
    check_array(images, "images")
    _marker_side_limit(tuple(images.shape))
    gray, f, h, w, pitch, stride, batched, was_np = _chess_gray(images, "images")
    mask = _dark_mask(gray, f, h, w, pitch, stride, block_radius, offset)
    return to_caller(mask if batched else mask[0], was_np)


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
    _marker_side_limit(tuple(mask.shape), colour_ok=False)
    if (mask.shape[0] if mask.ndim == 3 else 1) * mask.shape[-2] >= 2 ** 31:
        raise ValueError("mask: %d rows in all, the kernels take fewer than 2^31" % (mask.shape[0] * mask.shape[-2]))
    was_np = is_np(mask)
    m = _to_image(mask.view(np.uint8) if was_np and mask.dtype == np.bool_ else mask)
    m = m.to(torch.uint8) if m.dtype == torch.bool else m
    m = (m if m.ndim == 3 else m[None]).contiguous()
    labels = _label_components(m)
    return to_caller(labels if mask.ndim == 3 else labels[0], was_np)


def _marker_arguments(dictionary, block_radius, offset, min_side, max_side, max_bit_errors, refine_win):
    from . import boards
    block_radius, offset = _mask_arguments(block_radius, offset)
    min_side, max_side, max_bit_errors = _marker_integers(min_side=min_side, max_side=max_side, max_bit_errors=max_bit_errors)
    if not MARKER_MIN_SIDE <= min_side <= max_side <= MARKER_MAX_BOX:
        raise ValueError("min_side %d, max_side %d; the detector takes %d <= min_side <= max_side <= %d"
                         % (min_side, max_side, MARKER_MIN_SIDE, MARKER_MAX_BOX))
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


def _marker_stages(gray, f, h, w, pitch, stride, words_t, n_ids, s, block_radius, offset, min_side, max_side, max_bit_errors):
    """stages 1 to 6 on frames that fit the budget -> dict of CUDA tensors"""
    import torch
    dev = gray.device
    mask = _dark_mask(gray, f, h, w, pitch, stride, block_radius, offset)
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
    call("camd_marker_decode", dev, gray.data_ptr(), w, h, pitch, stride, f, labels.data_ptr(), cand.data_ptr(), counts.data_ptr(),
         min_side, words_t.data_ptr(), n_ids, s, max_bit_errors, quads.data_ptr(), id_turn.data_ptr(), best.data_ptr(),
         seen.data_ptr(), corners.data_ptr(), what="find_markers")
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
    check_array(images, "images")
    _marker_side_limit(tuple(images.shape))
    gray, f, h, w, pitch, stride, batched, was_np = _chess_gray(images, "images")
    if w < 3 or h < 3:
        raise ValueError("images of %d x %d; the detector takes sides from 3" % (w, h))
    words_t = torch.from_numpy(words.view(np.int64)).to(gray.device)
    chunk = max(1, min(f, 65535, MARKER_PLANE_BUDGET // (20 * h * w)))
    parts = []
    for a in range(0, f, chunk):
        n = min(chunk, f - a)
        parts.append(_marker_stages(gray[a:a + n] if gray.ndim == 3 else gray, n, h, w, pitch, stride, words_t, len(words), s,
                                    block_radius, offset, min_side, max_side, max_bit_errors))
    out = parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    seen, coarse = out["seen"], out["corners"]
    corners = coarse
    if refine_win is not None:
        corners = coarse.clone()
        lengths = (4 * seen.sum(1)).cpu().numpy()
        if int(lengths.sum()):
            g = gray if gray.ndim == 3 else gray[None]
            corners[seen] = corner_sub_pix(g, coarse[seen].reshape(-1, 2), refine_win, (-1, -1), MARKER_REFINE_CRITERIA,
                                           counts=lengths).reshape(-1, 4, 2)
    info = dict(status=out["status"], counts=out["counts"], candidates=out["candidates"], quads=out["quads"], id_turn=out["id_turn"],
                coarse=coarse)
    if not batched:
        seen, corners, info = seen[0], corners[0], {k: v[0] for k, v in info.items()}
    if not return_info:
        return to_caller((seen, corners), was_np)
    seen, corners = to_caller((seen, corners), was_np)
    return seen, corners, {k: to_caller(v, was_np) for k, v in info.items()}


def laplacian_sums(images):
    """The exact sums behind ``sharpness``: int64 (f, 2) (a batch) or (2,) of S1 = sum L and S2 = sum L^2 over every frame,
    L the 3 x 3 Laplacian [0 1 0; 1 -4 1; 0 1 0] of the gray image with reflect-101 borders."""
    import torch
    _check_image(images, "images")
    if images.ndim in (2, 3, 4) and min(images.shape[-3:-1] if images.shape[-1] == 3 and images.ndim > 2 else images.shape[-2:]) < 2:
        raise ValueError("images of %s; the Laplacian's mirrored border takes sides from 2" % (tuple(images.shape),))
    gray, f, h, w, pitch, stride, batched, was_np = _chess_gray(images, "images")
    sums = torch.empty((f, 2), dtype=torch.int64, device=gray.device)
    call("camd_laplacian_sums", gray.device, gray.data_ptr(), w, h, pitch, stride, f, sums.data_ptr(), what="sharpness")
    return to_caller(sums if batched else sums[0], was_np)


def sharpness(images):
    """``cv2.Laplacian(gray, cv2.CV_64F).var()`` of every image (reconstruction_with_board.py:9-12): a float for one
    image, float64 (f,) on the host for a batch.  uint8 gray (h, w) / (f, h, w) or colour (through ``cvt_gray(code="bgr")``),
    NumPy or CUDA, sides from 2.  The GPU gives the exact integer sums S1, S2 of the Laplacian and of its square
    (``laplacian_sums``); the variance (N S2 - S1^2) / N^2 is formed here from Python integers, rounded once.  UNPINNED
    against cv2."""
    from fractions import Fraction
    sums = laplacian_sums(images)
    sums = sums if is_np(sums) else sums.cpu().numpy()
    colour = images.ndim in (3, 4) and images.shape[-1] == 3
    h, w = (images.shape[-3:-1] if colour else images.shape[-2:])
    n = int(h) * int(w)
    var = [float(Fraction(n * int(s2) - int(s1) ** 2, n * n)) for s1, s2 in sums.reshape(-1, 2)]
    return var[0] if sums.ndim == 1 else np.array(var, np.float64)
