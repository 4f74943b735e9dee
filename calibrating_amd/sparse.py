"""Sparse (u, v, z) samples <-> dense images on the GPU -- same names, argument order, defaults and returned dtypes as
the reference's ``utils.uvzs_to_arr2d`` / ``arr2d_to_uvzs`` / ``interpolate_uvzs`` / ``interpolate_sparse2d``
(utils.py:291-415) and the triangulation of matches behind
``Stereo.get_depth_by_matched_uvs`` (epipolar_geometry.py:84-97).  NumPy in -> NumPy out, torch CUDA tensors in ->
tensors out (csrc/sparse.hip; INTEGRATION.md section E has the tie rules and what is refused).

Arguments are checked before the device is touched: ``inter_type="rbf"`` (SciPy's dense thin-plate solve) and a truthy
``constrained_type`` (``cv2.convexHull`` / ``drawContours``, whose rasterisation nothing here can pin) raise
``NotImplementedError`` on a machine without a GPU too.
"""
import ctypes

import numpy as np

from . import _native, hostio
from ._arrays import VALUE_TYPES, Kinv9, check_array, dtype_name, is_np, mat, positive_hw, to_caller, to_device
from ._native import call

MAX_DISTANCE = _native.NEAREST_MAX_RADIUS  # interpolate_uvzs(inter_type="nearest"): the search window the kernel supports
# the plane fit hands over to np.linalg.lstsq on the host when 1 - corr(u, v)^2 of the samples is not above this
COLLINEAR_TOL = 1e-9


def _require_finite(uv, what):
    """Non-finite coordinates are refused before any kernel is launched (for tensors: one flag read back)."""
    import torch
    ok = bool(np.isfinite(uv).all()) if is_np(uv) else bool(torch.isfinite(uv).all().item())
    if not ok:
        raise ValueError("%s: u, v must be finite" % what)


# ---- a. scatter ------------------------------------------------------------------------------------------------------
def uvzs_to_arr2d(uvs, hw=None, bg_value=0, arr2d=None, values=None):
    """Image of sparse samples (utils.py:291-317): pixel = ``int32(round(u, v))`` (half to even), rows outside are dropped,
    of several rows on one pixel the LAST wins.  ``uvs`` (n, 2) with ``values`` (n,) / (n, C), or (n, 2 + C) without;
    values float64, float32 or uint8; (n, C >= 2) -> (h, w, C), else (h, w); ``bg_value`` elsewhere, cast as
    ``np.ones(hw, dtype) * bg_value`` casts it.  A given ``arr2d`` is updated in place and returned.  ``hw=None`` is the
    reference's ``np.int32(uvs.max(0)[:2].round()) + 1``: (max u + 1, max v + 1) taken as (h, w) -- its quirk, kept."""
    import torch
    check_array(uvs, "uvs")
    if len(uvs.shape) != 2 or uvs.shape[1] < 2:
        raise ValueError("uvs must be (n, >= 2), got %s" % (tuple(uvs.shape),))
    if values is None:
        uvs, values = uvs[:, :2], uvs[:, 2:]
    else:
        check_array(values, "values")
    if len(values.shape) == 1:
        values = values[:, None]
    n = int(uvs.shape[0])
    if len(values.shape) != 2 or values.shape[0] != n or values.shape[1] < 1:
        raise ValueError("values must be (n,) or (n, C >= 1) with n = %d rows, got %s" % (n, tuple(values.shape)))
    if n >= 2 ** 31:
        raise ValueError("%d rows do not fit the 32-bit row index" % n)
    channels = int(values.shape[1])
    vname = dtype_name(values)
    if arr2d is None:
        if vname not in VALUE_TYPES:
            raise ValueError("values must be float64, float32 or uint8, got %s" % vname)
        probe = np.ones((1,), vname) * bg_value  # NumPy decides the image's dtype and the background's value
        oname, bg = probe.dtype.name, float(probe[0])
        if hw is None and n == 0:
            raise ValueError("hw=None needs at least one row")
    else:
        check_array(arr2d, "arr2d")
        oname, bg = dtype_name(arr2d), 0.0
        want = tuple(arr2d.shape[:2]) + ((channels,) if channels >= 2 else ())
        if tuple(arr2d.shape) != want:
            raise ValueError("arr2d %s does not take values of %d channel(s): expected %s" % (tuple(arr2d.shape), channels, want))
    if oname not in VALUE_TYPES:
        raise ValueError("the image would be %s; float64, float32 and uint8 are supported" % oname)
    if oname != vname and not np.can_cast(vname, oname, "safe"):
        raise ValueError("values of %s cannot be stored exactly in an image of %s" % (vname, oname))
    was_np = is_np(uvs)
    uv = to_device(uvs[:, :2], dtype="float64", cast=True)
    v = to_device(values, dtype=oname, cast=True, device=uv.device)
    if arr2d is None:
        if hw is None:
            m = uv.max(0).values.cpu().numpy()
            if not np.isfinite(m).all():
                raise ValueError("hw=None: u, v must be finite")
            hw = np.int32(m.round()) + 1
        h, w = positive_hw(hw)
        out = torch.empty((h, w, channels) if channels >= 2 else (h, w), dtype=v.dtype, device=uv.device)
    else:
        h, w = int(arr2d.shape[0]), int(arr2d.shape[1])
        out = to_device(arr2d, device=uv.device)
        if h == 0 or w == 0:
            return arr2d
    owner = torch.empty((h, w), dtype=torch.int32, device=uv.device)
    call("camd_uvzs_to_arr2d", uv.device, uv.data_ptr(), n, 2, w, h, v.data_ptr(), channels, VALUE_TYPES[oname], bg,
         0 if arr2d is None else 1, out.data_ptr(), owner.data_ptr(), what="uvzs_to_arr2d")
    if arr2d is None:
        return to_caller(out, was_np)
    if is_np(arr2d):
        np.copyto(arr2d, hostio.to_host(out))
    elif out.data_ptr() != arr2d.data_ptr():
        arr2d.copy_(out)
    return arr2d


# ---- b. arr2d_to_uvzs ------------------------------------------------------------------------------------------------
def arr2d_to_uvzs(arr2d, mask=None):
    """(x, y, arr2d[y, x]) rows (utils.py:320-329): without a mask every pixel, x outer and y inner; with one the masked
    pixels in row-major order.  The dtype is NumPy's promotion of int64 grids with ``arr2d`` (float -> float64,
    integers / bool -> int64).  A mask of any dtype is taken as boolean."""
    import torch
    check_array(arr2d, "arr2d")
    if len(arr2d.shape) != 2:
        raise ValueError("arr2d must be (h, w), got %s" % (tuple(arr2d.shape),))
    h, w = (int(s) for s in arr2d.shape)
    oname = np.result_type(np.int64, np.dtype(dtype_name(arr2d))).name
    if oname not in ("float64", "int64"):
        raise ValueError("arr2d of %s is not supported" % dtype_name(arr2d))
    if mask is not None:
        check_array(mask, "mask")
        if tuple(mask.shape) != (h, w):
            raise ValueError("mask %s does not match arr2d %s" % (tuple(mask.shape), (h, w)))
    was_np = is_np(arr2d)
    if h == 0 or w == 0:
        return np.zeros((0, 3), oname) if was_np else torch.zeros((0, 3), dtype=getattr(torch, oname), device=arr2d.device)
    a = to_device(arr2d, dtype=oname, cast=True)
    lib = _native.lib()
    if mask is None:
        rows = torch.empty((h * w, 3), dtype=a.dtype, device=a.device)
        call("camd_arr2d_to_uvzs", a.device, a.data_ptr(), w, h, int(oname == "int64"), rows.data_ptr(), what="arr2d_to_uvzs")
        return to_caller(rows, was_np)
    m = to_device(np.asarray(mask != 0) if is_np(mask) else (mask != 0), device=a.device).view(torch.uint8)
    rows = torch.empty((h * w, 3), dtype=a.dtype, device=a.device)
    count = torch.zeros(1, dtype=torch.int64, device=a.device)
    ws = torch.empty(lib.camd_arr2d_mask_workspace_bytes(h), dtype=torch.uint8, device=a.device)
    call("camd_arr2d_to_uvzs_masked", a.device, a.data_ptr(), m.data_ptr(), w, h, int(oname == "int64"), rows.data_ptr(), h * w,
         count.data_ptr(), ws.data_ptr(), what="arr2d_to_uvzs")
    n = int(count.item())  # synchronises: the output length is data dependent
    return to_caller(rows[:n], was_np)


# ---- c. / d. interpolation -------------------------------------------------------------------------------------------
def _check_interpolation(constrained_type, inter_type):
    if inter_type == "rbf":
        raise NotImplementedError('inter_type="rbf" is SciPy\'s dense thin-plate solve (scipy.interpolate.Rbf); it has no '
                                  'GPU form here -- use "nearest" or "lstsq"')
    if inter_type not in ("lstsq", "nearest"):
        raise ValueError('inter_type must be "lstsq", "nearest" (or the unsupported "rbf"), got %r' % (inter_type,))
    if constrained_type is not None and constrained_type:
        raise NotImplementedError("constrained_type restricts the fill to cv2.convexHull / cv2.drawContours of the samples; "
                                  "that rasterisation cannot be pinned here -- pass constrained_type=None")


def interpolate_sparse2d(sparse2d, constrained_type=None, inter_type="lstsq"):
    """``interpolate_uvzs`` of the non-zero, finite pixels of an image (utils.py:347-353)."""
    import torch
    _check_interpolation(constrained_type, inter_type)
    check_array(sparse2d, "sparse2d")
    if len(sparse2d.shape) != 2:
        raise ValueError("sparse2d must be (h, w), got %s" % (tuple(sparse2d.shape),))
    was_np = is_np(sparse2d)
    s = to_device(sparse2d)
    uvzs = arr2d_to_uvzs(s, (s != 0) & torch.isfinite(s))
    return to_caller(interpolate_uvzs(uvzs, tuple(s.shape[:2]), constrained_type, inter_type), was_np)


def interpolate_uvzs(uvzs, hw=None, constrained_type=None, inter_type="lstsq", distance=2, resize_hw=None):
    """Dense float32 (h, w) image of sparse (u, v, z) rows (utils.py:356-415).

    ``"nearest"``: each pixel takes ``float32(z)`` of the sample nearest to it in (u, v) if that distance -- float64
    ``sqrt(dx*dx + dy*dy)`` -- is ``< distance``, else 0; samples outside the grid take part; equal distances: the lowest
    row wins (SciPy's KDTree leaves that case open).  ``distance`` may be at most ``MAX_DISTANCE``; non-finite u, v are
    refused.  ``"lstsq"``: the least-squares plane z = a u + b v + c evaluated at every pixel.
    Empty ``uvzs`` -> ``zeros(hw, uvzs.dtype)``; ``hw=None`` -> ``(int(max v) + 2, int(max u) + 2)``.

    ``resize_hw`` (not in the reference; "nearest" only): ``hw`` is a low-resolution grid and the result is the
    ``cv2.resize(INTER_NEAREST)`` of its fill to ``resize_hw``, times ``resize_hw[1] / hw[1]`` -- what
    ``FeatureMatchingAsStereoMatching`` does with its 1/8 grid, written once at full resolution."""
    import torch
    _check_interpolation(constrained_type, inter_type)
    check_array(uvzs, "uvzs")
    if len(uvzs.shape) != 2 or uvzs.shape[1] < 3 or (inter_type == "lstsq" and uvzs.shape[1] != 3):
        raise ValueError("uvzs must be (n, 3), got %s" % (tuple(uvzs.shape),))
    if resize_hw is not None and inter_type != "nearest":
        raise ValueError('resize_hw goes with inter_type="nearest"')
    n = int(uvzs.shape[0])
    if n >= 2 ** 31:
        raise ValueError("%d samples do not fit the 32-bit sample index" % n)
    distance = float(distance)
    was_np = is_np(uvzs)
    if hw is None:
        if n == 0:
            raise ValueError("hw=None needs at least one sample")
        m = uvzs[:, :2].max(0) if was_np else uvzs[:, :2].max(0).values.cpu().numpy()
        if not np.isfinite(m).all():
            raise ValueError("interpolate_uvzs: u, v must be finite")
        hw = int(m[1]) + 2, int(m[0]) + 2
    h, w = positive_hw(hw)
    oh, ow = (h, w) if resize_hw is None else positive_hw(resize_hw, "resize_hw")
    if n == 0:
        if was_np:
            return np.zeros((oh, ow), uvzs.dtype)
        return torch.zeros((oh, ow), dtype=uvzs.dtype, device=uvzs.device)
    lib = _native.lib()
    if inter_type == "nearest":
        if distance != distance or distance > MAX_DISTANCE:
            raise ValueError("distance %r: the search window would exceed the %d cells each way the kernel supports "
                             "(distance <= %d)" % (distance, MAX_DISTANCE, MAX_DISTANCE))
        R, bw, bh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _native.check(lib.camd_sparse_bin_grid(w, h, distance, ctypes.byref(R), ctypes.byref(bw), ctypes.byref(bh)),
                      "interpolate_uvzs")
        if h > 65535 or oh > 65535:
            raise ValueError("grids of more than 65535 rows are not supported")
    _require_finite(uvzs[:, :2], "interpolate_uvzs")
    zname = "float32" if dtype_name(uvzs) == "float32" else "float64"
    uv = to_device(uvzs[:, :2], dtype="float64", cast=True)
    z = to_device(uvzs[:, 2], dtype=zname, cast=True, device=uv.device)
    dev, who = uv.device, "interpolate_uvzs"
    out = torch.empty((oh, ow), dtype=torch.float32, device=dev)
    if inter_type == "nearest":
        ncell = bw.value * bh.value
        counts = torch.empty(ncell, dtype=torch.int32, device=dev)
        call("camd_sparse_bin_count", dev, uv.data_ptr(), n, 2, w, h, distance, counts.data_ptr(), what=who)
        start = torch.zeros(ncell + 1, dtype=torch.int32, device=dev)
        torch.cumsum(counts, 0, dtype=torch.int32, out=start[1:])  # the exclusive scan between count and fill
        cursor = start[:-1].clone()
        suv = torch.empty((n, 2), dtype=torch.float64, device=dev)
        sidx = torch.empty(n, dtype=torch.int32, device=dev)
        call("camd_sparse_bin_fill", dev, uv.data_ptr(), n, 2, w, h, distance, cursor.data_ptr(), n, suv.data_ptr(),
             sidx.data_ptr(), what=who)
        call("camd_nearest_fill", dev, suv.data_ptr(), sidx.data_ptr(), start.data_ptr(), z.data_ptr(), VALUE_TYPES[zname],
             w, h, distance, out.data_ptr(), ow, oh, what=who)
    else:
        a, b, c = _fit_plane(lib, uv, z, zname, n)
        call("camd_plane_eval", dev, a, b, c, w, h, out.data_ptr(), what=who)
    return to_caller(out, was_np)


def _fit_plane(lib, uv, z, zname, n):
    """(a, b, c) of z = a u + b v + c: nine sums on the device (fixed reduction order), the 3x3 normal equations on the
    host in float64 -- by elimination of c, i.e. through the centred second moments, which is the same system."""
    import torch
    blocks = lib.camd_plane_sums_blocks(n)
    partials = torch.empty(blocks * 9, dtype=torch.float64, device=uv.device)
    sums = torch.empty(9, dtype=torch.float64, device=uv.device)
    call("camd_plane_sums", uv.device, uv.data_ptr(), 2, z.data_ptr(), VALUE_TYPES[zname], n, partials.data_ptr(),
         sums.data_ptr(), what="interpolate_uvzs")
    suu, suv, su, svv, sv, cnt, suz, svz, sz = (float(x) for x in sums.cpu().numpy())
    mu, mv, mz = su / cnt, sv / cnt, sz / cnt
    cuu, cvv, cuv = suu - su * mu, svv - sv * mv, suv - su * mv
    cuz, cvz = suz - su * mz, svz - sv * mz
    # det(A^T A) = n (cuu cvv - cuv^2).  Fewer than three non-collinear samples <=> it vanishes; decided relative to
    # cuu cvv, i.e. on 1 - corr(u, v)^2 <= COLLINEAR_TOL (also true when all u or all v coincide).  Then the system has
    # no unique solution and the reference's np.linalg.lstsq returns the minimum-norm one: do exactly that, on the host.
    det = cuu * cvv - cuv * cuv
    if n < 3 or not (det > COLLINEAR_TOL * cuu * cvv):
        s = np.concatenate([uv.cpu().numpy(), z.cpu().numpy().astype(np.float64)[:, None]], 1)
        A = s.copy()
        A[:, 2] = 1
        a, b, c = np.linalg.lstsq(A, s[:, 2], rcond=None)[0]
        return float(a), float(b), float(c)
    a = (cuz * cvv - cvz * cuv) / det
    b = (cvz * cuu - cuz * cuv) / det
    return a, b, mz - a * mu - b * mv


# ---- e. triangulation of matches -------------------------------------------------------------------------------------
def matched_uvs_to_zs(uvs1, uvs2, K1, K2, T_1to2):
    """``dict(zs1, zs2)``: the depth of every match along its ray in camera 1 and in camera 2 --
    ``matched_xyz_normals_to_zs(uvs_to_xyz_noramls(uvs1, K1), uvs_to_xyz_noramls(uvs2, K2), T_1to2)``
    (epipolar_geometry.py:84-97): per match the least-squares solution of [-R X1, X2] (z1, z2)^T = t.  ``uvs*`` (n, 2)
    pixels, ``T_1to2`` 4x4 (or 3x4) with X2 = R X1 + t.  float64."""
    import torch
    check_array(uvs1, "uvs1")
    check_array(uvs2, "uvs2")
    if len(uvs1.shape) != 2 or uvs1.shape[1] != 2 or tuple(uvs2.shape) != tuple(uvs1.shape):
        raise ValueError("uvs1, uvs2 must both be (n, 2), got %s and %s" % (tuple(uvs1.shape), tuple(uvs2.shape)))
    T = np.asarray(T_1to2, np.float64)
    if T.shape not in ((4, 4), (3, 4)):
        raise ValueError("T_1to2 must be 4x4 or 3x4, got %s" % (T.shape,))
    T4 = np.eye(4)
    T4[:3] = T[:3]
    Kinv = [Kinv9(K) for K in (K1, K2)]
    n = int(uvs1.shape[0])
    a = to_device(uvs1, dtype="float64", cast=True)
    b = to_device(uvs2, dtype="float64", cast=True, device=a.device)
    T4 = mat(T4, 16)
    zs = torch.empty((2, n), dtype=torch.float64, device=a.device)
    call("camd_matched_uvs_to_zs", a.device, a.data_ptr(), b.data_ptr(), n, Kinv[0].ctypes.data, Kinv[1].ctypes.data,
         T4.ctypes.data, zs[0].data_ptr(), zs[1].data_ptr(), what="matched_uvs_to_zs")
    zs = to_caller(zs, is_np(uvs1))
    return dict(zs1=zs[0], zs2=zs[1])
