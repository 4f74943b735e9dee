"""Sparse (u, v, z) samples <-> dense images on the GPU -- same names, argument order, defaults and returned dtypes as
the reference's ``utils.uvzs_to_arr2d`` / ``arr2d_to_uvzs`` / ``interpolate_uvzs`` / ``interpolate_sparse2d``
(utils.py:291-415) and the triangulation of matches behind
``Stereo.get_depth_by_matched_uvs`` (epipolar_geometry.py:84-97).  NumPy in -> NumPy out, torch CUDA tensors in ->
tensors out (csrc/sparse.hip; INTEGRATION.md section E has the tie rules and what is refused).

Arguments are checked before the device is touched: ``inter_type="rbf"`` (SciPy's dense thin-plate solve) and a truthy
``constrained_type`` (``cv2.convexHull`` / ``drawContours``, whose rasterisation nothing here can pin) raise
``NotImplementedError`` on a machine without a GPU too.  The fill inside the samples' convex hull is a function of its own
with a mask contract of its own: ``interpolate_uvzs_in_hull`` / ``interpolate_sparse2d_in_hull`` / ``convex_hull_mask``
(csrc/hull.hip), batched over frames.  What ``inter_type="rbf"`` computes has names of its own too, a float64 result and a
cap on the samples: ``interpolate_uvzs_rbf`` / ``interpolate_sparse2d_rbf`` (csrc/spline.hip), batched over frames.
"""
import ctypes

import numpy as np

from . import _native, hostio
from ._arrays import VALUE_TYPES, Kinv9, check_array, dtype_name, is_np, mat, positive_hw, to_caller, to_device
from ._native import call

MAX_DISTANCE = _native.NEAREST_MAX_RADIUS  # interpolate_uvzs(inter_type="nearest"): the search window the kernel supports
# the plane fit hands over to np.linalg.lstsq on the host when 1 - corr(u, v)^2 of the samples is not above this
COLLINEAR_TOL = 1e-9
# interpolate_uvzs_in_hull / convex_hull_mask (csrc/hull.hip): the rows one frame may hold, and the bits of its status word
MAX_HULL_POINTS = 4096  # CAMD_HULL_MAX_POINTS
STATUS_NO_SAMPLE, STATUS_DEGENERATE, STATUS_OUT_OF_RANGE = 1, 2, 4
# interpolate_uvzs_rbf (csrc/spline.hip): the rows one frame may hold -- what one workgroup factors -- and its status values
MAX_SPLINE_POINTS = _native.SPLINE_MAX_POINTS
SPLINE_NO_SAMPLE, SPLINE_SINGULAR, SPLINE_NON_FINITE = 1, 2, 4


def _require_finite(uv, what, columns="u, v"):
    """Non-finite coordinates are refused before any kernel is launched (for tensors: one flag read back)."""
    import torch
    ok = bool(np.isfinite(uv).all()) if is_np(uv) else bool(torch.isfinite(uv).all().item())
    if not ok:
        raise ValueError("%s: %s must be finite" % (what, columns))


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


# ---- d'. the plane inside the samples' convex hull -------------------------------------------------------------------
def _hull_layout(rows, width, counts, what, limit=None):
    """(flat rows (N, width), frame lengths, batched) of the three ways the rows are given: (n, width) one frame,
    (f, n, width) a batch, ragged (N, width) with ``counts``.  Refuses everything else; nothing touches the device.
    ``limit``: (rows a frame may hold, that constant's name, advice for the message) where they are not the hull's."""
    check_array(rows, what)
    shape = tuple(int(s) for s in rows.shape)
    if counts is not None:
        lengths = np.asarray(counts)
        if lengths.ndim != 1 or lengths.dtype.kind not in "iu" or len(lengths) == 0 or (lengths < 0).any():
            raise ValueError("counts must be a non-empty 1-d array of non-negative integers")
        lengths = lengths.astype(np.int64)
        if len(shape) != 2 or shape[1] != width or int(lengths.sum()) != shape[0]:
            raise ValueError("with counts, %s is ragged rows (N, %d) with N = sum(counts) = %d, got %s"
                             % (what, width, lengths.sum(), shape))
        batched = True
    elif len(shape) == 2 and shape[1] == width:
        lengths, batched = np.array([shape[0]], np.int64), False
    elif len(shape) == 3 and shape[2] == width and shape[0] >= 1:
        lengths, batched = np.full(shape[0], shape[1], np.int64), True
    else:
        raise ValueError("%s must be (n, %d) or (f, n, %d), got %s" % (what, width, width, shape))
    cap, cap_name, advice = limit or (MAX_HULL_POINTS, "MAX_HULL_POINTS", "")
    if lengths.max() > cap:
        raise ValueError("%s: a frame of %d rows, at most %s = %d are supported%s" % (what, lengths.max(), cap_name, cap, advice))
    return rows.reshape(-1, width), lengths, batched


def _hull_fit(flat, lengths, hw, keep_last_per_pixel, counts_given):
    """Stage A (``camd_hull_fit``) -> the per-frame record on the device: vertices, hull_counts, abc, status."""
    import torch
    frames, capacity = len(lengths), max(1, int(lengths.max()))
    uv = to_device(flat[:, :2], dtype="float64", cast=True)
    dev, z, zname = uv.device, None, "float64"
    if flat.shape[1] == 3:
        zname = "float32" if dtype_name(flat) == "float32" else "float64"
        z = to_device(flat[:, 2], dtype=zname, cast=True, device=dev)
    start = None
    if counts_given:
        start = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)
    rec = dict(vertices=torch.empty((frames, capacity, 2), dtype=torch.int32, device=dev),
               hull_counts=torch.empty(frames, dtype=torch.int32, device=dev),
               abc=torch.empty((frames, 3), dtype=torch.float64, device=dev),
               status=torch.empty(frames, dtype=torch.int32, device=dev), capacity=capacity, frames=frames)
    call("camd_hull_fit", dev, uv.data_ptr(), 2, None if z is None else z.data_ptr(), VALUE_TYPES[zname], int(uv.shape[0]),
         None if start is None else start.data_ptr(), frames, hw[1], hw[0], int(bool(keep_last_per_pixel)), capacity,
         rec["vertices"].data_ptr(), rec["hull_counts"].data_ptr(), rec["abc"].data_ptr(), rec["status"].data_ptr(),
         what="interpolate_uvzs_in_hull")
    return rec


def _rows_that_take_part(uvz, hw, keep_last_per_pixel):
    """Host NumPy: the rows of one frame the kernel fits (valid; with ``keep_last_per_pixel`` inside the image and the
    last of their pixel) -- for the minimum-norm fallback of a degenerate frame."""
    s = np.asarray(uvz, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.rint(s[:, :2])
        ok = np.isfinite(s).all(1) & (s[:, 2] != 0) & (np.abs(r) <= 2 ** 20).all(1)
        if keep_last_per_pixel:
            ok &= (r[:, 0] >= 0) & (r[:, 0] < hw[1]) & (r[:, 1] >= 0) & (r[:, 1] < hw[0])
    idx = np.nonzero(ok)[0]
    if keep_last_per_pixel and len(idx):
        last = {}
        for i in idx:
            last[(r[i, 0], r[i, 1])] = i
        idx = np.array(sorted(last.values()))
    return s[idx]


def convex_hull_mask(uvs, hw, counts=None):
    """uint8 (h, w) -- or (f, h, w) for (f, n, 2) rows or ragged (N, 2) rows with ``counts`` -- that is 1 where the pixel
    lies in the closed convex hull of ``int32(round(u, v))`` (half to even) of the rows with finite u, v within 2**20:
    this package's own, integer-exact mask, not ``cv2.drawContours``'.  Points outside the
    image take part; one point fills its pixel, collinear points the pixels whose centres lie on the segment."""
    import torch
    flat, lengths, batched = _hull_layout(uvs, 2, counts, "uvs")
    h, w = positive_hw(hw)
    was_np = is_np(uvs)
    rec = _hull_fit(flat, lengths, (h, w), False, counts is not None)
    out = torch.empty((rec["frames"], h, w), dtype=torch.uint8, device=rec["abc"].device)
    call("camd_hull_mask", out.device, rec["vertices"].data_ptr(), rec["hull_counts"].data_ptr(), rec["capacity"], rec["frames"],
         w, h, out.data_ptr(), what="convex_hull_mask")
    return to_caller(out if batched else out[0], was_np)


# ---- d''. the hull of any number of samples; the nearest sample inside it (csrc/lidar.hip) -----------------------------
def _cloud_hull_record(uv, uv_stride, n, rows_range=None, what="cloud_hull"):
    """The hull record (vertices (1, capacity, 2), hull_counts (1,), capacity, status (1,)) of ``n`` (u, v) rows on the device,
    ``uv_stride`` doubles apart, however many: the per-row extremes of their pixels (``camd_hull_extremes``) are the candidates,
    ``camd_hull_fit`` takes them in chunks of ``MAX_HULL_POINTS`` and the surviving vertices go round again until one frame
    holds them.  ``rows_range`` = (y0, rows) when the caller knows the pixel rows the samples can reach; else one device
    min / max of the rounded v and one read-back."""
    import torch
    dev = uv.device
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if rows_range is None:
        rng = torch.empty(3, dtype=torch.int32, device=dev)
        call("camd_hull_row_range", dev, uv.data_ptr(), uv_stride, n, rng.data_ptr(), what=what)
        lo, hi = (int(x) for x in rng[:2].cpu().numpy())  # (the status bits come with the extremes)
        rows_range = (lo, hi - lo + 1) if lo <= hi else (0, 1)
    y0, rows = rows_range
    table = torch.empty((rows, 2), dtype=torch.int32, device=dev)
    cand = torch.empty((2 * rows, 2), dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    call("camd_hull_extremes", dev, uv.data_ptr(), uv_stride, n, y0, rows, table.data_ptr(), cand.data_ptr(), count.data_ptr(),
         status.data_ptr(), what=what)
    m = int(count.item())
    cand = cand[:m]
    while True:
        frames = max(1, -(-m // MAX_HULL_POINTS))
        capacity = max(1, min(m, MAX_HULL_POINTS))
        start = torch.from_numpy(np.minimum(np.arange(frames + 1, dtype=np.int64) * MAX_HULL_POINTS, m)).to(dev)
        verts = torch.empty((frames, capacity, 2), dtype=torch.int32, device=dev)
        hull_counts = torch.empty(frames, dtype=torch.int32, device=dev)
        abc = torch.empty((frames, 3), dtype=torch.float64, device=dev)
        fit_status = torch.empty(frames, dtype=torch.int32, device=dev)
        call("camd_hull_fit", dev, cand.data_ptr(), 2, None, VALUE_TYPES["float64"], m, start.data_ptr(), frames, 1, 1, 0, capacity,
             verts.data_ptr(), hull_counts.data_ptr(), abc.data_ptr(), fit_status.data_ptr(), what=what)
        if frames == 1:
            status |= fit_status & STATUS_NO_SAMPLE
            return dict(vertices=verts, hull_counts=hull_counts, capacity=capacity, status=status, table=table, rows_range=rows_range)
        keep = torch.arange(capacity, device=dev)[None, :] < hull_counts[:, None]
        cand = verts[keep].to(torch.float64)  # the frames' vertices in frame order (synchronises: the length is data dependent)
        if int(cand.shape[0]) >= m:
            raise ValueError("%s: a round over %d candidates left %d; the hull has more than MAX_HULL_POINTS = %d vertices"
                             % (what, m, int(cand.shape[0]), MAX_HULL_POINTS))
        m = int(cand.shape[0])


def _one_frame_uv(uvs, what):
    check_array(uvs, what)
    if len(uvs.shape) != 2 or uvs.shape[1] != 2:
        raise ValueError("%s must be one frame (n, 2), got %s" % (what, tuple(uvs.shape)))
    if int(uvs.shape[0]) >= 2 ** 31:
        raise ValueError("%d rows do not fit the 32-bit row index" % uvs.shape[0])
    return int(uvs.shape[0])


def cloud_hull(uvs):
    """(k, 2) int32: the vertices of the convex hull of ``int32(round(u, v))`` (half to even) of ONE frame of any number of
    rows, in ``camd_hull_fit``'s order (from the lowest (x, y), each next vertex the one that leaves every other point on one
    side).  The validity rule and the contract are ``convex_hull_mask``'s."""
    n = _one_frame_uv(uvs, "uvs")
    uv = to_device(uvs, dtype="float64", cast=True)
    rec = _cloud_hull_record(uv, 2, n)
    k = int(rec["hull_counts"].item())
    return to_caller(rec["vertices"][0, :k].contiguous(), is_np(uvs))


def cloud_hull_mask(uvs, hw):
    """``convex_hull_mask`` of ONE frame (n, 2) of any number of rows: uint8 (h, w).  For a frame of at most
    ``MAX_HULL_POINTS`` rows the two are the same bits."""
    import torch
    n = _one_frame_uv(uvs, "uvs")
    h, w = positive_hw(hw)
    uv = to_device(uvs, dtype="float64", cast=True)
    rec = _cloud_hull_record(uv, 2, n, what="cloud_hull_mask")
    out = torch.empty((1, h, w), dtype=torch.uint8, device=uv.device)
    call("camd_hull_mask", out.device, rec["vertices"].data_ptr(), rec["hull_counts"].data_ptr(), rec["capacity"], 1, w, h,
         out.data_ptr(), what="cloud_hull_mask")
    return to_caller(out[0], is_np(uvs))


def _check_nearest_distance(distance):
    distance = float(distance)
    if distance != distance or distance > MAX_DISTANCE:
        raise ValueError("distance %r: the search window would exceed the %d cells each way the kernel supports "
                         "(distance <= %d)" % (distance, MAX_DISTANCE, MAX_DISTANCE))
    return distance


def _nearest_in_hull(rows, n, hw, distance, zname, rows_range=None, z=None, what="interpolate_uvzs_in_hull"):
    """(float32 (h, w) tensor, hull record): ``rows`` is (n, 3) float64 (u, v, z) on the device -- or (n, 2) with ``z`` a
    contiguous tensor of ``zname`` -- read in place; bins as ``interpolate_uvzs("nearest")`` makes them."""
    import torch
    h, w = hw
    dev, stride = rows.device, int(rows.shape[1])
    lib = _native.lib()
    R, bw, bh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _native.check(lib.camd_sparse_bin_grid(w, h, distance, ctypes.byref(R), ctypes.byref(bw), ctypes.byref(bh)), what)
    rec = _cloud_hull_record(rows, stride, n, rows_range, what)
    ncell = bw.value * bh.value
    counts = torch.empty(ncell, dtype=torch.int32, device=dev)
    call("camd_sparse_bin_count", dev, rows.data_ptr(), n, stride, w, h, distance, counts.data_ptr(), what=what)
    start = torch.zeros(ncell + 1, dtype=torch.int32, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int32, out=start[1:])
    cursor = start[:-1].clone()
    suv = torch.empty((max(n, 1), 2), dtype=torch.float64, device=dev)
    sidx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    call("camd_sparse_bin_fill", dev, rows.data_ptr(), n, stride, w, h, distance, cursor.data_ptr(), n, suv.data_ptr(),
         sidx.data_ptr(), what=what)
    zptr, zstride = (rows.data_ptr() + 16, stride) if z is None else (z.data_ptr(), 1)
    out = torch.empty((h, w), dtype=torch.float32, device=dev)
    call("camd_nearest_fill_in_hull", dev, suv.data_ptr(), sidx.data_ptr(), start.data_ptr(), zptr, VALUE_TYPES[zname], zstride, w, h,
         distance, rec["vertices"].data_ptr(), rec["hull_counts"].data_ptr(), rec["capacity"], out.data_ptr(), what=what)
    return out, rec


def _interpolate_nearest_in_hull(uvzs, hw, counts, reciprocal, keep_last_per_pixel, return_info, zero_frames, distance):
    check_array(uvzs, "uvzs")
    if counts is not None or len(uvzs.shape) != 2 or uvzs.shape[1] != 3:
        raise ValueError('inter_type="nearest" takes one frame (n, 3) without counts, got %s%s'
                         % (tuple(uvzs.shape), "" if counts is None else " with counts"))
    if reciprocal or keep_last_per_pixel or zero_frames is not None:
        raise ValueError('reciprocal, keep_last_per_pixel and zero_frames go with inter_type="lstsq"')
    n = int(uvzs.shape[0])
    if n >= 2 ** 31:
        raise ValueError("%d samples do not fit the 32-bit sample index" % n)
    distance = _check_nearest_distance(distance)
    h, w = positive_hw(hw)
    if h > 65535:
        raise ValueError("grids of more than 65535 rows are not supported")
    was_np = is_np(uvzs)
    _require_finite(uvzs[:, :2], "interpolate_uvzs_in_hull")
    zname = "float32" if dtype_name(uvzs) == "float32" else "float64"
    uv = to_device(uvzs[:, :2], dtype="float64", cast=True)
    z = to_device(uvzs[:, 2], dtype=zname, cast=True, device=uv.device)
    out, rec = _nearest_in_hull(uv, n, (h, w), distance, zname, z=z)
    out = to_caller(out, was_np)
    if not return_info:
        return out
    status, hull_counts = to_caller((rec["status"], rec["hull_counts"]), was_np)
    return out, dict(status=status[0], hull_counts=hull_counts[0])


def interpolate_uvzs_in_hull(uvzs, hw, counts=None, reciprocal=False, keep_last_per_pixel=False, return_info=False,
                             zero_frames=None, inter_type="lstsq", distance=2):
    """``inter_type="nearest"`` (with ``distance``): ONE frame (n, 3) of any n < 2**31 -> float32 (h, w) that is
    ``interpolate_uvzs(uvzs, hw, None, "nearest", distance)`` where ``cloud_hull_mask(uvzs[:, :2], hw)`` is 1 and 0 elsewhere,
    without forming either (pixels outside the hull are not searched): what the reference's
    ``interpolate_uvzs(constrained_type="convex_hull", inter_type="nearest")`` is for, a LiDAR sweep as a depth image.  Every
    row with finite u, v takes part, whatever its z; non-finite u, v are refused; ``return_info`` adds ``dict(status,
    hull_counts)`` with the bits 1 and 4 below.  A batch, ``counts``, ``reciprocal``, ``keep_last_per_pixel`` and
    ``zero_frames`` are refused.  The default, ``"lstsq"``, is:

    The least-squares plane z = a u + b v + c of sparse (u, v, z) rows, written only inside their convex hull and 0
    outside: float32 (h, w) for (n, 3) rows, (f, h, w) for a batch (f, n, 3) or ragged rows (N, 3) with ``counts`` (the
    convention of ``pnp.solve_pnp_batch``).  What the reference's ``interpolate_uvzs(..., constrained_type=True)`` is for
    (utils.py:356-415), with the mask of ``convex_hull_mask`` in place of cv2's.  NumPy in -> NumPy out, CUDA in -> CUDA out.

    A row takes part when u, v are finite, z is finite and not 0 and the rounded pixel is within 2**20.
    ``keep_last_per_pixel``: rows whose pixel is outside the image are dropped and of several rows on one pixel the last
    stays -- what a scatter through ``uvzs_to_arr2d`` leaves.  ``reciprocal``: float32 ``1 / that`` is written instead
    (``+inf`` outside the hull, as the reference's ``1 / interpolate_sparse2d(...)`` gives).  At most ``MAX_HULL_POINTS``
    rows per frame.  A frame gets the same bits alone and anywhere in a batch.

    ``return_info`` adds ``dict(status, abc, hull_counts)``; status bits: 1 no row takes part (empty mask), 2 fewer than
    three non-collinear rows, 4 a row beyond 2**20 was left out.  A batch leaves a frame of status 2 NaN inside its
    hull; the (n, 3) form reads its one status word and takes ``np.linalg.lstsq``'s minimum-norm plane on the host, as
    ``interpolate_uvzs`` does for such samples.  ``zero_frames`` (f,) bool, of a batch: the frames written as zeros
    throughout, whatever ``reciprocal`` says -- the frames of a recording that show no board."""
    import torch
    if inter_type == "nearest":
        return _interpolate_nearest_in_hull(uvzs, hw, counts, reciprocal, keep_last_per_pixel, return_info, zero_frames, distance)
    if inter_type != "lstsq":
        raise ValueError('inter_type must be "lstsq" or "nearest", got %r' % (inter_type,))
    flat, lengths, batched = _hull_layout(uvzs, 3, counts, "uvzs")
    h, w = positive_hw(hw)
    was_np = is_np(uvzs)
    if zero_frames is not None:
        check_array(zero_frames, "zero_frames")
        if not batched or tuple(zero_frames.shape) != (len(lengths),):
            raise ValueError("zero_frames goes with a batch and holds one flag per frame (%d), got %s"
                             % (len(lengths), tuple(zero_frames.shape)))
    rec = _hull_fit(flat, lengths, (h, w), keep_last_per_pixel, counts is not None)
    dev = rec["abc"].device
    if not batched and int(rec["status"].item()) & (STATUS_NO_SAMPLE | STATUS_DEGENERATE) == STATUS_DEGENERATE:
        s = _rows_that_take_part(flat if was_np else flat.cpu().numpy(), (h, w), keep_last_per_pixel)
        A = s.copy()
        A[:, 2] = 1
        rec["abc"].copy_(torch.from_numpy(np.linalg.lstsq(A, s[:, 2], rcond=None)[0].reshape(1, 3)))
    out = torch.empty((rec["frames"], h, w), dtype=torch.float32, device=dev)
    zero = None if zero_frames is None else (to_device(zero_frames, device=dev) != 0).view(torch.uint8)
    call("camd_hull_fill", dev, rec["vertices"].data_ptr(), rec["hull_counts"].data_ptr(), rec["abc"].data_ptr(), rec["capacity"],
         rec["frames"], w, h, int(bool(reciprocal)), None if zero is None else zero.data_ptr(), out.data_ptr(),
         what="interpolate_uvzs_in_hull")
    out = to_caller(out if batched else out[0], was_np)
    if not return_info:
        return out
    info = to_caller((rec["status"], rec["abc"], rec["hull_counts"]), was_np)
    return out, dict(zip(("status", "abc", "hull_counts"), info if batched else (x[0] for x in info)))


def interpolate_sparse2d_in_hull(sparse2d, reciprocal=False):
    """``interpolate_uvzs_in_hull`` of the non-zero, finite pixels of an (h, w) image: the image form
    (utils.py:347-353 with ``constrained_type=True``).  More than ``MAX_HULL_POINTS`` such pixels are refused."""
    import torch
    check_array(sparse2d, "sparse2d")
    if len(sparse2d.shape) != 2:
        raise ValueError("sparse2d must be (h, w), got %s" % (tuple(sparse2d.shape),))
    hw = positive_hw(sparse2d.shape)
    was_np = is_np(sparse2d)
    if was_np:  # counted on the host: the refusal comes before the device is touched
        with np.errstate(invalid="ignore"):
            n = int(np.count_nonzero((sparse2d != 0) & np.isfinite(sparse2d)))
        if n > MAX_HULL_POINTS:
            raise ValueError("sparse2d holds %d samples, at most MAX_HULL_POINTS = %d are supported" % (n, MAX_HULL_POINTS))
    s = to_device(sparse2d)
    uvzs = arr2d_to_uvzs(s, (s != 0) & torch.isfinite(s))
    if int(uvzs.shape[0]) > MAX_HULL_POINTS:
        raise ValueError("sparse2d holds %d samples, at most MAX_HULL_POINTS = %d are supported" % (uvzs.shape[0], MAX_HULL_POINTS))
    return to_caller(interpolate_uvzs_in_hull(uvzs, hw, reciprocal=reciprocal), was_np)


# ---- d3. the thin-plate spline through the samples (csrc/spline.hip) ---------------------------------------------------
_SPLINE_LIMIT = (MAX_SPLINE_POINTS, "MAX_SPLINE_POINTS",
                 " (one workgroup factors a frame's matrix): thin the samples first, e.g. scatter them through uvzs_to_arr2d "
                 "on a coarser grid and take arr2d_to_uvzs of that")


def _spline_start(lengths, device):
    import torch
    return torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(device)


def _spline_smooth(smooth):
    smooth = float(smooth)
    if smooth != smooth:
        raise ValueError("smooth must be a number, got nan")
    return smooth


def _spline_rows(rows, counts, what, least):
    """``_hull_layout`` of rows (.., >= least) under the spline's limit, and their width."""
    check_array(rows, what)
    width = int(rows.shape[-1]) if len(rows.shape) >= 2 else 0
    if width < least:
        raise ValueError("%s must be (n, >= %d) or (f, n, >= %d), got %s" % (what, least, least, tuple(rows.shape)))
    return _hull_layout(rows, width, counts, what, _SPLINE_LIMIT) + (width,)


def _check_spline_mask(mask, frames, hw, batched):
    if mask is None:
        return
    check_array(mask, "mask")
    if tuple(mask.shape) != tuple(hw) and not (batched and tuple(mask.shape) == (frames,) + tuple(hw)):
        raise ValueError("mask must be %s%s, got %s" % (tuple(hw), " or %s" % ((frames,) + tuple(hw),) if batched else "",
                                                       tuple(mask.shape)))


def _spline_eval(rows, width, lengths, cap, weights, mask, hw, grid_step):
    """``camd_spline_eval`` -> float64 (frames, h, w); ``mask`` checked by ``_check_spline_mask``: (h, w) is every frame's."""
    import torch
    frames, dev = len(lengths), rows.device
    m = None
    if mask is not None:
        m = (to_device(mask, device=dev) != 0).view(torch.uint8)
        if m.dim() == 2:
            m = m[None].expand(frames, -1, -1)
        m = m.contiguous()
    out = torch.empty((frames,) + tuple(hw), dtype=torch.float64, device=dev)
    call("camd_spline_eval", dev, rows.data_ptr(), width, int(rows.shape[0]), _spline_start(lengths, dev).data_ptr(), frames, cap,
         weights.data_ptr(), None if m is None else m.data_ptr(), hw[1], hw[0], grid_step, out.data_ptr(), what="spline_eval")
    return out


def spline_assemble(uvzs, smooth=0.5, counts=None):
    """Stage 1 of ``interpolate_uvzs_rbf``: float64 A = Phi - smooth I; (n, n) for (n, >= 2) rows, (f, c, c) with c the
    longest frame for a batch (f, n, >= 2) or ragged rows with ``counts`` -- a shorter frame fills its leading block, the
    rest is 0.  Phi[i][j] = r^2 log r of the distance r between rows i and j, 0 at r = 0; symmetric bit for bit."""
    import torch
    flat, lengths, batched, width = _spline_rows(uvzs, counts, "uvzs", 2)
    smooth = _spline_smooth(smooth)
    was_np = is_np(uvzs)
    _require_finite(flat[:, :2], "spline_assemble")
    frames, cap = len(lengths), max(1, int(lengths.max()))
    rows = to_device(flat, dtype="float64", cast=True)
    A = torch.zeros((frames, cap, cap), dtype=torch.float64, device=rows.device)
    call("camd_spline_assemble", rows.device, rows.data_ptr(), width, int(rows.shape[0]),
         _spline_start(lengths, rows.device).data_ptr(), frames, cap, smooth, A.data_ptr(), what="spline_assemble")
    return to_caller(A if batched else A[0, :int(lengths[0]), :int(lengths[0])], was_np)


def spline_solve(A, z, counts=None):
    """Stage 2: ``(weights, status)`` of A w = z by LU with partial pivoting (the largest |a|, of equal ones the lowest row),
    one workgroup per frame.  A (n, n) with z (n,) -> weights (n,) and a scalar status; A (f, c, c) with z (f, c), or with
    ragged z (N,) and ``counts`` (frame f is the leading counts[f] block) -> weights (f, c), 0 beyond a frame's rows, and
    status (f,) int32: 0, ``SPLINE_NO_SAMPLE``, ``SPLINE_SINGULAR`` (a zero or non-finite pivot) or ``SPLINE_NON_FINITE``
    (in A or z); the last two leave NaN weights.  ``A`` is left as it was: the kernel factors a copy in place."""
    import torch
    check_array(A, "A")
    check_array(z, "z")
    shape = tuple(int(v) for v in A.shape)
    if len(shape) == 2 and shape[0] == shape[1] and shape[0] >= 1 and counts is None:
        batched, cap, lengths = False, shape[0], np.array([shape[0]], np.int64)
        ok = tuple(z.shape) == (shape[0],)
    elif len(shape) == 3 and shape[1] == shape[2] and shape[0] >= 1 and shape[1] >= 1:
        batched, cap = True, shape[1]
        if counts is None:
            lengths, ok = np.full(shape[0], cap, np.int64), tuple(z.shape) == shape[:2]
        else:
            lengths = np.asarray(counts)
            if lengths.ndim != 1 or lengths.dtype.kind not in "iu" or len(lengths) != shape[0] or (lengths < 0).any():
                raise ValueError("counts must hold one non-negative integer per frame of A (%d)" % shape[0])
            lengths = lengths.astype(np.int64)
            ok = tuple(z.shape) == (int(lengths.sum()),) and lengths.max() <= cap
    else:
        raise ValueError("A must be (n, n) or (f, c, c) with n, f, c >= 1, got %s" % (shape,))
    if not ok:
        raise ValueError("z %s does not go with A %s%s" % (tuple(z.shape), shape, "" if counts is None else " and counts"))
    if cap > MAX_SPLINE_POINTS:
        raise ValueError("A: a frame of %d rows, at most %s = %d are supported%s" % (cap, _SPLINE_LIMIT[1], MAX_SPLINE_POINTS, _SPLINE_LIMIT[2]))
    was_np, frames = is_np(A), len(lengths)
    work = to_device(A, dtype="float64", cast=True)
    if not was_np and work.data_ptr() == A.data_ptr():
        work = work.clone()
    rhs = to_device(z, dtype="float64", cast=True, device=work.device).reshape(-1)
    weights = torch.zeros((frames, cap), dtype=torch.float64, device=work.device)
    status = torch.empty(frames, dtype=torch.int32, device=work.device)
    call("camd_spline_solve", work.device, rhs.data_ptr(), 1, int(rhs.shape[0]), _spline_start(lengths, work.device).data_ptr(), frames,
         cap, work.data_ptr(), weights.data_ptr(), status.data_ptr(), what="spline_solve")
    return to_caller((weights, status) if batched else (weights[0], status[0]), was_np)


def spline_eval(uvs, weights, hw, counts=None, mask=None, grid_step=1):
    """Stage 3: float64 (h, w) -- (f, h, w) of a batch -- with pixel (x, y) = sum_i w_i phi(|(x, y) * grid_step - (u_i, v_i)|),
    added in row order.  ``uvs`` as ``spline_assemble`` takes them; ``weights`` (n,), of a batch (f, c) with c at least the
    longest frame, as ``spline_solve`` returns them.  ``mask`` (h, w), or (f, h, w) of a batch: where it is 0 the pixel is 0
    and costs nothing.  ``grid_step`` s: ``hw`` is a coarse image whose pixel (x, y) stands at (x s, y s) of the samples'
    frame."""
    import torch
    flat, lengths, batched, width = _spline_rows(uvs, counts, "uvs", 2)
    check_array(weights, "weights")
    frames, longest = len(lengths), int(lengths.max())
    wshape = tuple(int(v) for v in weights.shape)
    if not ((batched and len(wshape) == 2 and wshape[0] == frames and wshape[1] >= max(1, longest)) or
            (not batched and wshape == (longest,))):
        raise ValueError("weights %s do not go with %d frame(s) of at most %d rows" % (wshape, frames, longest))
    h, w = positive_hw(hw)
    grid_step = int(grid_step)
    if grid_step < 1 or h * grid_step >= 2 ** 31 or w * grid_step >= 2 ** 31:
        raise ValueError("grid_step must be a positive integer with hw * grid_step below 2**31, got %r" % (grid_step,))
    _check_spline_mask(mask, frames, (h, w), batched)
    was_np = is_np(uvs)
    _require_finite(flat[:, :2], "spline_eval")
    rows = to_device(flat, dtype="float64", cast=True)
    if longest == 0 and not batched:
        wt = torch.zeros((1, 1), dtype=torch.float64, device=rows.device)
    else:
        wt = to_device(weights, dtype="float64", cast=True, device=rows.device).reshape(frames, -1)
    out = _spline_eval(rows, width, lengths, int(wt.shape[1]), wt, mask, (h, w), grid_step)
    return to_caller(out if batched else out[0], was_np)


def interpolate_uvzs_rbf(uvzs, hw=None, smooth=0.5, counts=None, mask=None, return_info=False):
    """The reference's ``interpolate_uvzs(uvzs, hw, inter_type="rbf")`` (utils.py:373-388), i.e.
    ``scipy.interpolate.Rbf(u, v, z, function="thin_plate", smooth=smooth)`` at every pixel, under a name of its own
    (``interpolate_uvzs(inter_type="rbf")`` keeps raising): float64 (h, w) for (n, 3) rows, (f, h, w) for a batch (f, n, 3)
    or ragged rows (N, 3) with ``counts``.  NumPy in -> NumPy out, CUDA in -> CUDA out.

    With phi(r) = r^2 log r, phi(0) = 0: A = Phi - smooth I over the samples' distances, A w = z by LU with partial
    pivoting, pixel (x, y) = sum_i w_i phi(|(x, y) - (u_i, v_i)|) in row order (``spline_assemble`` / ``spline_solve`` /
    ``spline_eval``, one kernel each).  A frame gets the same bits alone and anywhere in a batch.  At most
    ``MAX_SPLINE_POINTS`` rows per frame: more are refused before the device is touched -- thin them through
    ``uvzs_to_arr2d`` on a coarser grid.  Non-finite u, v, z are refused.  A frame without rows is zeros.
    ``hw=None`` -> ``(int(max v) + 2, int(max u) + 2)``, the reference's rule.  ``mask`` (h, w) or (f, h, w): pixels where
    it is 0 are written 0 and cost nothing; ``convex_hull_mask`` makes the reference's ``constrained_type`` of it.

    ``return_info`` adds ``dict(weights, status)``: status 0, ``SPLINE_NO_SAMPLE`` (1) or ``SPLINE_SINGULAR`` (2: a zero or
    non-finite pivot, e.g. two rows on one (u, v) at smooth = 0 -- the frame is NaN and is not repaired)."""
    import torch
    flat, lengths, batched, _ = _spline_rows(uvzs, counts, "uvzs", 3)
    if int(flat.shape[1]) != 3:
        raise ValueError("uvzs must be (n, 3) or (f, n, 3), got %s" % (tuple(uvzs.shape),))
    smooth = _spline_smooth(smooth)
    was_np, total = is_np(uvzs), int(flat.shape[0])
    if hw is None:
        if total == 0:
            raise ValueError("hw=None needs at least one sample")
        m = flat[:, :2].max(0) if was_np else flat[:, :2].max(0).values.cpu().numpy()
        if not np.isfinite(m).all():
            raise ValueError("interpolate_uvzs_rbf: u, v, z must be finite")
        hw = int(m[1]) + 2, int(m[0]) + 2
    h, w = positive_hw(hw)
    frames, cap = len(lengths), max(1, int(lengths.max()))
    _check_spline_mask(mask, frames, (h, w), batched)
    _require_finite(flat, "interpolate_uvzs_rbf", "u, v, z")
    rows = to_device(flat, dtype="float64", cast=True)
    dev, who = rows.device, "interpolate_uvzs_rbf"
    start = _spline_start(lengths, dev)
    A = torch.empty((frames, cap, cap), dtype=torch.float64, device=dev)
    weights = torch.zeros((frames, cap), dtype=torch.float64, device=dev)
    status = torch.empty(frames, dtype=torch.int32, device=dev)
    call("camd_spline_assemble", dev, rows.data_ptr(), 3, total, start.data_ptr(), frames, cap, smooth, A.data_ptr(), what=who)
    call("camd_spline_solve", dev, rows.data_ptr() + 16, 3, total, start.data_ptr(), frames, cap, A.data_ptr(), weights.data_ptr(),
         status.data_ptr(), what=who)
    out = _spline_eval(rows, 3, lengths, cap, weights, mask, (h, w), 1)
    out = to_caller(out if batched else out[0], was_np)
    if not return_info:
        return out
    if not batched:
        weights, status = weights[0, :int(lengths[0])], status[0]
    return out, dict(zip(("weights", "status"), to_caller((weights, status), was_np)))


def interpolate_sparse2d_rbf(sparse2d, smooth=0.5, mask=None):
    """``interpolate_uvzs_rbf`` of the non-zero, finite pixels of an (h, w) image (utils.py:347-353 with
    ``inter_type="rbf"``): float64 (h, w).  More than ``MAX_SPLINE_POINTS`` such pixels are refused."""
    import torch
    check_array(sparse2d, "sparse2d")
    if len(sparse2d.shape) != 2:
        raise ValueError("sparse2d must be (h, w), got %s" % (tuple(sparse2d.shape),))
    hw = positive_hw(sparse2d.shape)
    was_np = is_np(sparse2d)
    refusal = "sparse2d holds %d samples, at most MAX_SPLINE_POINTS = %d are supported" + _SPLINE_LIMIT[2]
    if was_np:  # counted on the host: the refusal comes before the device is touched
        with np.errstate(invalid="ignore"):
            n = int(np.count_nonzero((sparse2d != 0) & np.isfinite(sparse2d)))
        if n > MAX_SPLINE_POINTS:
            raise ValueError(refusal % (n, MAX_SPLINE_POINTS))
    _check_spline_mask(mask, 1, hw, False)
    s = to_device(sparse2d)
    uvzs = arr2d_to_uvzs(s, (s != 0) & torch.isfinite(s))
    if int(uvzs.shape[0]) > MAX_SPLINE_POINTS:
        raise ValueError(refusal % (int(uvzs.shape[0]), MAX_SPLINE_POINTS))
    m = None if mask is None else to_device(mask, device=s.device)
    return to_caller(interpolate_uvzs_rbf(uvzs, hw, smooth, mask=m), was_np)


def spline_upsize(coarse, hw):
    """``cv2.resize(coarse * hw[1] / coarse.shape[1], hw[::-1], interpolation=INTER_NEAREST)`` of a float64 (h, w) image: the
    last step of the reference's ``FeatureMatchingAsStereoMatching`` (stereo_matching.py:139-140), kept in float64."""
    import torch
    check_array(coarse, "coarse")
    if len(coarse.shape) != 2 or dtype_name(coarse) != "float64":
        raise ValueError("coarse must be float64 (h, w), got %s %s" % (dtype_name(coarse), tuple(coarse.shape)))
    h, w = positive_hw(coarse.shape)
    oh, ow = positive_hw(hw)
    if oh > 65535:
        raise ValueError("images of more than 65535 rows are not supported")
    src = to_device(coarse)
    out = torch.empty((oh, ow), dtype=torch.float64, device=src.device)
    call("camd_spline_upsize", src.device, src.data_ptr(), w, h, 1, out.data_ptr(), ow, oh, what="spline_upsize")
    return to_caller(out, is_np(coarse))


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
