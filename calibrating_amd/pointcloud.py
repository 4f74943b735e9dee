"""Depth post-ops around ``get_depth`` on the GPU -- same names and argument meaning as the reference's
``utils.depth_to_point_cloud`` / ``apply_T_to_point_cloud`` / ``point_cloud_to_depth``
(/root/reference/calibrating/utils.py:152-161, 213-318) and the interpolation-rate rule of
``utils._get_appropriate_interpolation_rate`` (:201-210).  float64 like the reference's NumPy.
NumPy in -> NumPy out, torch CUDA tensors in -> tensors out.

The payload half -- ``point_cloud_to_arr2d`` with values (:254-317), ``get_reproject_remap`` (:332-344) and the
``cv2.remap(img2, mapx, mapy, INTER_LINEAR)`` after it (camera.py:322-342, here ``reproject_img``) -- runs through a
z-buffer that remembers its winner.  Points that share a pixel and have bit-equal z: the larger index wins
(INTEGRATION.md section D).
"""
import ctypes

import numpy as np

from . import _native
from ._arrays import VALUE_TYPES, K9, Kinv9, check_array, dtype_name, is_np, mat, positive_wh, to_caller, to_device
from ._native import call


def _f64(a):
    """(float64 CUDA tensor -- this module casts, as the reference's NumPy does -- , was_numpy)"""
    return to_device(a, dtype="float64", cast=True), is_np(a)


def get_appropriate_interpolation_rate(cam1, cam2, interpolation=1.5):
    """utils._get_appropriate_interpolation_rate (utils.py:201-210)."""
    if interpolation:
        rate = cam1.K[0, 0] / cam2.K[0, 0] * interpolation
        if interpolation >= 1:
            rate = max(rate, 1)
    else:
        rate = 1
    return rate


def depth_to_point_cloud(depth, K, interpolation_rate=1, return_xyzuv=False):
    """(N, 3) points of the non-zero depths in row-major order, or (N, 5) ``xyzuv`` (utils.py:213-246).
    uint16 depth is millimetres, as in the reference."""
    import torch
    if is_np(depth) and depth.dtype == np.uint16:
        depth = np.float32(depth / 1000.0)
    d, was_np = _f64(depth)
    if d.dim() != 2:
        raise AssertionError("depth.ndim == 2")
    h, w = d.shape
    lib = _native.lib()
    rate = float(interpolation_rate)
    gw, gh = ctypes.c_int(), ctypes.c_int()
    _native.check(lib.camd_point_cloud_grid(w, h, rate, ctypes.byref(gw), ctypes.byref(gh)), "depth_to_point_cloud")
    cap = gw.value * gh.value
    Kinv = Kinv9(K)
    pts = torch.empty((cap, 3), dtype=torch.float64, device=d.device)
    uv = torch.empty((cap, 2), dtype=torch.float64, device=d.device) if return_xyzuv else None
    count = torch.zeros(1, dtype=torch.int64, device=d.device)
    ws = torch.empty(lib.camd_point_cloud_workspace_bytes(w, h, rate), dtype=torch.uint8, device=d.device)
    call("camd_depth_to_point_cloud", d.device, d.data_ptr(), w, h, Kinv.ctypes.data, rate, pts.data_ptr(),
         None if uv is None else uv.data_ptr(), cap, count.data_ptr(), ws.data_ptr(), what="depth_to_point_cloud")
    n = int(count.item())  # synchronises: the output length is data dependent
    return to_caller(torch.cat([pts[:n], uv[:n]], dim=1) if return_xyzuv else pts[:n], was_np)


def apply_T_to_point_cloud(T, point_cloud):
    """(T @ [p, 1])[:3] for every row; extra columns are carried over (utils.py:152-161)."""
    import torch
    p, was_np = _f64(point_cloud)
    xyz = p[:, :3].contiguous()
    out = torch.empty_like(xyz)
    Tm = mat(T, 16)
    call("camd_apply_T_to_point_cloud", p.device, xyz.data_ptr(), xyz.shape[0], Tm.ctypes.data, out.data_ptr(),
         what="apply_T_to_point_cloud")
    if p.shape[1] > 3:
        out = torch.cat([out, p[:, 3:]], dim=1)
    return to_caller(out, was_np)


def point_cloud_to_depth(points, K, xy, bg_value=0):
    """Depth image (xy[1], xy[0]) float64 of a point cloud: nearest z per pixel (utils.py:249-318)."""
    import torch
    p, was_np = _f64(points)
    if p.dim() != 2 or p.shape[1] < 3:
        raise ValueError("points must be (N, >=3)")
    w, h = int(xy[0]), int(xy[1])
    Km = K9(K)
    depth = torch.empty((h, w), dtype=torch.float64, device=p.device)
    keys = torch.empty((h, w), dtype=torch.int64, device=p.device)
    call("camd_point_cloud_to_depth", p.device, p.data_ptr(), p.shape[0], p.shape[1], Km.ctypes.data, w, h, float(bg_value),
         depth.data_ptr(), keys.data_ptr(), what="point_cloud_to_depth")
    return to_caller(depth, was_np)


def project_depth(depth2, K2, T_2in1, K1, xy1, interpolation_rate=1):
    """depth image of camera 2 seen from camera 1: depth_to_point_cloud -> apply_T -> point_cloud_to_depth
    (camera.py:298-309) as one scatter pass over the sampling grid.  uint16 depth is millimetres, as in the
    ``depth_to_point_cloud`` the reference composes it from."""
    import torch
    check_array(depth2, "depth2")
    d, was_np = _depth_metres(depth2, dtype_name(depth2)), is_np(depth2)
    h2, w2 = d.shape
    w1, h1 = int(xy1[0]), int(xy1[1])
    K2inv, Tm, K1m = Kinv9(K2), mat(T_2in1, 16), K9(K1)
    depth1 = torch.empty((h1, w1), dtype=torch.float64, device=d.device)
    keys = torch.empty((h1, w1), dtype=torch.int64, device=d.device)
    call("camd_project_depth", d.device, d.data_ptr(), w2, h2, K2inv.ctypes.data, Tm.ctypes.data, K1m.ctypes.data,
         float(interpolation_rate), w1, h1, depth1.data_ptr(), keys.data_ptr(), what="project_depth")
    return to_caller(depth1, was_np)


# ---- the z-buffer with a payload -----------------------------------------------------------------------------------
def _same_device(a, b, what):
    if not is_np(a) and not is_np(b) and a.device != b.device:
        raise ValueError("%s live on different devices: %s and %s" % (what, a.device, b.device))


def point_cloud_to_arr2d(points, K, xy, values=None, bg_value=0):
    """Image (xy[1], xy[0][, C]) of what the nearest point per pixel carries (utils.py:254-317): ``values`` (N,) or
    (N, 1) -> (h, w); (N, C >= 2) -> (h, w, C); float64, float32 or uint8, the result has the values' dtype and
    ``bg_value`` where no point lands.  ``values=None`` is ``point_cloud_to_depth``.  The coloured-cloud path is
    ``values = img[mask]``.  Points with bit-equal z on one pixel: the later row wins."""
    if values is None:
        return point_cloud_to_depth(points, K, xy, bg_value=bg_value)
    check_array(points, "points")
    check_array(values, "values")
    if len(points.shape) != 2 or points.shape[1] < 3:
        raise ValueError("points must be (N, >=3), got %s" % (tuple(points.shape),))
    n = int(points.shape[0])
    vshape = tuple(values.shape)
    if len(vshape) not in (1, 2) or vshape[0] != n or (len(vshape) == 2 and vshape[1] < 1):
        raise ValueError("values must be (N,) or (N, C) with N = %d points, got %s" % (n, vshape))
    name = dtype_name(values)
    if name not in VALUE_TYPES:
        raise ValueError("values must be float64, float32 or uint8, got %s" % name)
    bg = float(bg_value)
    if name == "uint8" and not (0 <= bg <= 255 and bg == int(bg)):
        raise ValueError("bg_value %r is not a uint8" % (bg_value,))
    _same_device(points, values, "points and values")
    w, h = positive_wh(xy)
    Km = K9(K)
    channels = vshape[1] if len(vshape) == 2 else 1
    import torch
    p, _ = _f64(points)
    v = to_device(values, device=p.device)
    out = torch.empty((h, w, channels) if channels >= 2 else (h, w), dtype=v.dtype, device=p.device)
    keys = torch.empty((h, w), dtype=torch.int64, device=p.device)
    owner = torch.empty((h, w), dtype=torch.int32, device=p.device)
    call("camd_point_cloud_to_arr2d", p.device, p.data_ptr(), n, p.shape[1], Km.ctypes.data, w, h, v.data_ptr(), channels,
         VALUE_TYPES[name], bg, out.data_ptr(), keys.data_ptr(), owner.data_ptr(), what="point_cloud_to_arr2d")
    return to_caller(out, is_np(values))


def _check_depth2(depth2):
    check_array(depth2, "depth2")
    if len(depth2.shape) not in (2, 3) or 0 in tuple(depth2.shape):
        raise ValueError("depth2 must be (h2, w2) or (n, h2, w2), got %s" % (tuple(depth2.shape),))
    name = dtype_name(depth2)
    if name not in ("float64", "float32", "uint16"):
        raise ValueError("depth2 must be float64, float32 or uint16 (millimetres), got %s" % name)
    return name


def _depth_metres(depth2, name):
    """float64 CUDA tensor of the depth in metres; uint16 is millimetres through float32 (utils.py:218-219)."""
    if name == "uint16":
        if is_np(depth2):
            depth2 = np.float32(depth2 / 1000.0)
        else:
            import torch
            depth2 = (depth2.to(torch.float64) / 1000.0).to(torch.float32)
    return to_device(depth2, dtype="float64", cast=True)


def _reproject_args(K1, K2, T_2in1, xy1, interpolation_rate):
    w1, h1 = positive_wh(xy1, "xy1")
    rate = float(interpolation_rate)
    if not (rate > 0 and np.isfinite(rate)):
        raise ValueError("interpolation_rate must be positive and finite, got %r" % (interpolation_rate,))
    K2m = np.asarray(K2, np.float64)
    if K2m.ndim != 2 or K2m.shape[0] < 3 or K2m.shape[1] < 3:
        raise ValueError("K2 must be a 3x3 matrix, got shape %s" % (K2m.shape,))
    K2inv = Kinv9(K2m)
    K1m = np.asarray(K1, np.float64)
    if K1m.ndim != 2 or K1m.shape[0] < 3 or K1m.shape[1] < 3:
        raise ValueError("K1 must be a 3x3 matrix, got shape %s" % (K1m.shape,))
    return w1, h1, rate, K2inv, mat(T_2in1, 16), K9(K1m)


def _reproject_maps(d, w1, h1, rate, K2inv, Tm, K1m):
    """(n, 2, h1, w1) float32 CUDA tensor of a float64 (n, h2, w2) CUDA depth."""
    import torch
    n, h2, w2 = d.shape
    maps = torch.empty((n, 2, h1, w1), dtype=torch.float32, device=d.device)
    keys = torch.empty((n, h1, w1), dtype=torch.int64, device=d.device)
    owner = torch.empty((n, h1, w1), dtype=torch.int32, device=d.device)
    call("camd_reproject_remap", d.device, d.data_ptr(), w2, h2, h2 * w2, K2inv.ctypes.data, Tm.ctypes.data, K1m.ctypes.data,
         rate, w1, h1, maps.data_ptr(), maps.data_ptr() + 4 * h1 * w1, 2 * h1 * w1, keys.data_ptr(), owner.data_ptr(), n,
         what="get_reproject_remap")
    return maps


def get_reproject_remap(K1, K2, T_2in1, depth2, xy1, interpolation_rate=1):
    """(mapx, mapy) = (2, h1, w1) float32: where each pixel of camera 1 finds itself in camera 2's image, through
    camera 2's depth; -1 where nothing landed (utils.py:332-344).  ``depth2`` (n, h2, w2) -> (n, 2, h1, w1).
    uint16 depth is millimetres."""
    name = _check_depth2(depth2)
    args = _reproject_args(K1, K2, T_2in1, xy1, interpolation_rate)
    d = _depth_metres(depth2, name)
    batched = d.dim() == 3
    maps = _reproject_maps(d if batched else d[None], *args)
    return to_caller(maps if batched else maps[0], is_np(depth2))


def reproject_img(img2, depth2, K2, T_2in1, K1, xy1, interpolation_rate=1):
    """Camera 2's image in camera 1's frame: ``get_reproject_remap`` then ``cv2.remap(img2, mapx, mapy,
    cv2.INTER_LINEAR)`` (camera.py:333-341).  ``img2`` uint8 (h2, w2) or (h2, w2, 3) with ``depth2`` (h2, w2); a batch
    is ``depth2`` (n, h2, w2) with ``img2`` (n, h2, w2) or (n, h2, w2, 3).  Pixels nothing reaches are 0."""
    from . import imgproc
    name = _check_depth2(depth2)
    check_array(img2, "img2")
    if dtype_name(img2) != "uint8":
        raise ValueError("img2 must be uint8, got %s" % dtype_name(img2))
    batched = len(depth2.shape) == 3
    ishape, dshape = tuple(img2.shape), tuple(depth2.shape)
    if not (ishape == dshape or ishape == dshape + (3,)):
        raise ValueError("img2 %s does not match depth2 %s: expected the depth's shape, or that with 3 channels"
                         % (ishape, dshape))
    _same_device(img2, depth2, "img2 and depth2")
    args = _reproject_args(K1, K2, T_2in1, xy1, interpolation_rate)
    import torch
    d = _depth_metres(depth2, name)
    img = to_device(img2, device=d.device)
    maps = _reproject_maps(d if batched else d[None], *args)
    imgs = img if batched else img[None]
    out = torch.stack([imgproc.remap(imgs[i], maps[i, 0], maps[i, 1], imgproc.INTER_LINEAR) for i in range(len(imgs))])
    return to_caller(out if batched else out[0], is_np(img2))
