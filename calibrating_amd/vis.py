"""The pictures of ``calibrating/utils.py`` on the GPU (csrc/vis.hip): ``vis_depth`` (utils.py:463-483), ``vis_depth_l1``
(:486-575), ``vis_stereo`` / ``vis_align`` (:673-719).  ndarrays in give ndarrays out; CUDA tensors in give tensors on
their device and its current stream.  A single image (h, w) or a batch (n, h, w); every image of a batch is treated as a
call of its own (its own colour bar, limit and range).

Float32 depths are widened exactly and everything is computed in float64 -- for float32 input the reference computes in
float32, a documented deviation.  INTEGRATION.md also lists what is defined where the reference fails.
"""
import numpy as np

from ._arrays import check_array, dtype_name, is_np, to_caller, to_device
from ._native import VALUE_F32, VALUE_F64, VALUE_U16, call, lib

__all__ = ["vis_depth", "vis_depth_l1", "resolve_max_l1", "vis_stereo", "vis_align", "colormap_table", "COLORMAP_JET",
           "COLORMAP_HSV"]

COLORMAP_JET, COLORMAP_HSV = 2, 9  # cv2's ids
_DEPTH_TYPES = {"float64": VALUE_F64, "float32": VALUE_F32, "uint16": VALUE_U16}
_BAR_PLACES = {"u": 1, "d": 2, "l": 3, "r": 4}  # CAMD_BAR_*
_LIMIT_FIXED, _LIMIT_MAX, _LIMIT_TOP = 0, 1, 2  # CAMD_LIMIT_*
_RANGE_GIVEN, _RANGE_NORMA, _RANGE_MAX = 0, 1, 2  # CAMD_RANGE_*
_INF = float("inf")
_tables = {}


def colormap_table(colormap):
    """(256, 3) uint8 RGB table of ``COLORMAP_JET`` / ``COLORMAP_HSV``.  UNPINNED: cv2 is absent, so
    these restate OpenCV's tables by formula -- JET: r, g, b = clip(1.5 - |4 v - 3|), clip(1.5 - |4 v - 2|),
    clip(1.5 - |4 v - 1|) with v = i / 255; HSV: the hue circle at full saturation and value, hue = 360 v degrees, so that
    index 0 and index 255 are both red -- each rounded to the nearest byte."""
    if colormap not in _tables:
        v = np.arange(256) / 255.0
        if colormap == COLORMAP_JET:
            rgb = [np.clip(1.5 - np.abs(4 * v - c), 0, 1) for c in (3, 2, 1)]
        elif colormap == COLORMAP_HSV:
            h6 = v * 6.0
            rgb = [np.clip(np.abs((h6 + s) % 6 - 3) - 1, 0, 1) for s in (0, 4, 2)]
        else:
            raise ValueError("colormap %r: COLORMAP_JET (2), COLORMAP_HSV (9) or a (256, 3) uint8 RGB table" % (colormap,))
        t = np.uint8(np.rint(np.stack(rgb, -1) * 255))
        t.setflags(write=False)
        _tables[colormap] = t
    return _tables[colormap]


def _jet_bgr_075():
    """``np.uint8(cv2.applyColorMap(x, COLORMAP_JET) * 0.75)`` as a table: BGR order, as ``_to_3x_uint8`` (utils.py:457) and
    ``Cam.vis_depth_alignment`` (camera.py:319) leave it."""
    return np.uint8(colormap_table(COLORMAP_JET)[:, ::-1] * 0.75)


def _plane(a, what, types, like=None):
    """A depth-like input checked before the device is touched -> (n, h, w, batched, type name)."""
    check_array(a, what)
    name = dtype_name(a)
    if name not in types:
        raise TypeError("%s must be %s, got %s" % (what, " or ".join(sorted(types)), name))
    if len(a.shape) not in (2, 3) or min(a.shape) <= 0:
        raise ValueError("%s must be (h, w) or (n, h, w) without an empty side, got %s" % (what, tuple(a.shape)))
    if like is not None and (tuple(a.shape) != tuple(like.shape) or is_np(a) != is_np(like)):
        raise ValueError("%s must have the shape %s and the kind of the first array" % (what, tuple(like.shape)))
    batched = len(a.shape) == 3
    return (int(a.shape[0]) if batched else 1), int(a.shape[-2]), int(a.shape[-1]), batched, name


def _device_table(table, device):
    import torch
    if is_np(table) or not hasattr(table, "is_cuda"):
        t = np.ascontiguousarray(table)
        if t.dtype != np.uint8 or t.shape != (256, 3):
            raise ValueError("a colour table is (256, 3) uint8 RGB")
        return torch.from_numpy(t.copy()).to(device)
    if dtype_name(table) != "uint8" or tuple(table.shape) != (256, 3):
        raise ValueError("a colour table is (256, 3) uint8 RGB")
    return to_device(table, device=device)


def _depth_picture(d, name, n, npix, table, *, divisor=1.0, clip=(-_INF, _INF), given=None, range_mode=_RANGE_GIVEN,
                   slicen=0.0, scale=255.9, zero_mask=True, what="vis_depth"):
    """One ``camd_vis_depth`` (after ``camd_vis_depth_range`` where the range comes from the picture) -> (n * npix, 3)."""
    import torch
    dst = torch.empty((n * npix, 3), dtype=torch.uint8, device=d.device)
    keys, (lo, den) = None, (given or (0.0, 1.0))
    if range_mode != _RANGE_GIVEN:
        keys = torch.empty((n, 2), dtype=torch.int64, device=d.device)
        call("camd_vis_depth_range", d.device, d.data_ptr(), _DEPTH_TYPES[name], npix, n, divisor, clip[0], clip[1],
             keys.data_ptr(), what=what)
    call("camd_vis_depth", d.device, d.data_ptr(), _DEPTH_TYPES[name], npix, n, divisor, clip[0], clip[1], lo, den,
         None if keys is None else keys.data_ptr(), range_mode, float(slicen), scale, table.data_ptr(), int(zero_mask),
         dst.data_ptr(), what=what)
    return dst


def vis_depth(depth, slicen=0, fix_range=None, colormap=None):
    """``utils.vis_depth`` (utils.py:463-483) -> uint8 RGB (..., h, w, 3).

    ``depth``: float64, float32 (widened) or uint16 (millimetres: divided by 1000.0), (h, w) or (n, h, w); an input that
    already is (..., 3 | 4) is returned as it is.  ``fix_range``: (lo, hi) with hi > lo, or a number x for (0, x): clip,
    then (d - lo) / (hi - lo); None (or 0): ``boxx.norma``, recalled as (d - min) / (max - min) per image, min and max
    from a device reduction; a constant image gives index 0.  ``slicen``: (n * slicen) % 1 -- contour bands.  The index
    is uint8(n * 255.9), the colour ``colormap[index]``: a (256, 3) uint8 RGB table (array or tensor) or cv2's
    ``COLORMAP_JET`` / ``COLORMAP_HSV`` (defaults: JET, HSV with ``slicen``; see ``colormap_table``).  Pixels whose raw
    depth is 0 are black."""
    if len(depth.shape) == 3 and depth.shape[-1] in (3, 4):
        return depth
    n, h, w, batched, name = _plane(depth, "depth", _DEPTH_TYPES)
    if slicen < 0:
        raise ValueError("slicen must not be negative, got %r" % (slicen,))
    given, clip = None, (-_INF, _INF)
    if fix_range:
        number = isinstance(fix_range, (int, float, np.number))
        lo, hi = (0.0, float(fix_range)) if number else (float(fix_range[0]), float(fix_range[1]))
        if not (hi > lo and abs(hi) < _INF and abs(lo) < _INF):
            raise ValueError("fix_range must be (lo, hi) with lo < hi, both finite, got %r" % (fix_range,))
        given, clip = (lo, hi - lo), (lo, hi)
    if colormap is None or (isinstance(colormap, (int, np.integer)) and not colormap):
        colormap = COLORMAP_HSV if slicen else COLORMAP_JET
    was_np = is_np(depth)
    d = to_device(depth)
    table = _device_table(colormap_table(int(colormap)) if isinstance(colormap, (int, np.integer)) else colormap, d.device)
    dst = _depth_picture(d, name, n, h * w, table, divisor=1000.0 if name == "uint16" else 1.0,
                         clip=clip, given=given,
                         range_mode=_RANGE_GIVEN if given else _RANGE_NORMA, slicen=slicen)
    return to_caller(dst.view(((n,) if batched else ()) + (h, w, 3)), was_np)


# ---- vis_depth_l1 ------------------------------------------------------------------------------------------------------
def _bar_place(colorbar, h, w):
    if not colorbar:
        return 0, 0
    if not isinstance(colorbar, str):
        raise ValueError("colorbar must be 'u', 'd', 'l', 'r', 'auto' or None, got %r" % (colorbar,))
    if colorbar.startswith("a"):
        colorbar = dict(zip((h, w), "ld"))[min(h, w)]  # the shorter side; a square picture: 'd'
    if colorbar not in _BAR_PLACES:
        raise ValueError("colorbar must be 'u', 'd', 'l', 'r', 'auto' or None, got %r" % (colorbar,))
    width = (h + w) // 100
    if width > (h if colorbar in "ud" else w):
        raise ValueError("a colour bar %d wide does not fit a picture of %d x %d" % (width, h, w))
    return _BAR_PLACES[colorbar], width


def _l1_planes(re, gt, max_l1, overexposed, colorbar):
    """The error pass, the bar and the limit, queued -> (l1, valid, limit (n,), flag, n, h, w, batched)."""
    import torch
    n, h, w, batched, name = _plane(re, "re", ("float64", "float32"))
    gt_value, gt_array = 0.0, None
    if isinstance(gt, (int, float, np.number)):
        gt_value = float(gt)
        if not abs(gt_value) < _INF:
            raise ValueError("gt is not finite")
    else:
        _plane(gt, "gt", (name,), like=re)
        gt_array = gt
    if max_l1 is not None:
        max_l1 = float(max_l1)
        if not abs(max_l1) < _INF:
            raise ValueError("max_l1 is not finite")
    place, width = _bar_place(colorbar, h, w)
    bar_later = place and max_l1 is None  # the reference raises here; defined: the limit first, then the bar from it
    if max_l1 is None:
        max_l1 = -0.05 if overexposed else 0.0
    r = to_device(re)
    g = None if gt_array is None else to_device(gt_array, device=r.device)
    dev, npix = r.device, h * w
    l1 = torch.empty((n, h, w), dtype=torch.float64, device=dev)
    valid = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    maxkey = torch.empty((n,), dtype=torch.int64, device=dev)
    flag = torch.empty((1,), dtype=torch.int32, device=dev)
    limit = torch.empty((n,), dtype=torch.float64, device=dev)
    call("camd_vis_l1_error", dev, r.data_ptr(), None if g is None else g.data_ptr(), gt_value, _DEPTH_TYPES[name], w, h, n,
         0 if bar_later else place, width, max_l1, l1.data_ptr(), valid.data_ptr(), maxkey.data_ptr(), flag.data_ptr(),
         what="vis_depth_l1")
    if max_l1 > 0:
        mode, value, ws = _LIMIT_FIXED, max_l1, None
    elif max_l1 == 0 or max_l1 <= -1:
        mode, value, ws = _LIMIT_MAX, 0.0, None
    else:
        mode, value = _LIMIT_TOP, -max_l1
        ws = torch.empty((lib().camd_vis_l1_limit_workspace_bytes(n),), dtype=torch.uint8, device=dev)
    call("camd_vis_l1_limit", dev, l1.data_ptr(), valid.data_ptr(), npix, n, mode, value, maxkey.data_ptr(),
         None if ws is None else ws.data_ptr(), limit.data_ptr(), what="vis_depth_l1")
    if bar_later:
        call("camd_vis_l1_bar", dev, l1.data_ptr(), valid.data_ptr(), w, h, n, place, width, limit.data_ptr(),
             what="vis_depth_l1")
    return l1, valid, limit, flag, n, h, w, batched


def _raise_if_non_finite(flag):
    bad = int(flag.item())  # the one host read: the counter of the error pass
    if bad:
        raise ValueError("vis_depth_l1: %d pixels of re / gt are NaN or infinite" % bad)


def resolve_max_l1(re, gt=0, max_l1=None, overexposed=True, colorbar=None):
    """The limit ``vis_depth_l1`` would colour with -> float64, a 0-d array / tensor or (n,) for a batch.  ``max_l1`` > 0:
    itself; 0, <= -1, or None with ``overexposed=False``: the maximum of |l1|; inside (-1, 0) (None: -0.05): the |l1| at
    descending rank ``int(-max_l1 * valid_num)`` among the valid pixels, 1.0 where there is none -- an exact selection
    on the device.  With a ``colorbar`` and a ``max_l1`` the bar's pixels take part, as in the reference; with a
    ``colorbar`` and ``max_l1=None`` the limit comes from the picture without the bar."""
    was_np = is_np(re)
    _, _, limit, flag, _, _, _, batched = _l1_planes(re, gt, max_l1, overexposed, colorbar)
    _raise_if_non_finite(flag)
    return to_caller(limit if batched else limit[0], was_np)


def vis_depth_l1(re, gt=0, max_l1=None, overexposed=True, colorbar="auto"):
    """``utils.vis_depth_l1`` (utils.py:486-575) -> uint8 RGB (..., h, w, 3): missing depth black, l1 == 0 grey, re
    behind gt red, in front green, beyond the limit white-ish.  ``re``: float64 or float32 (widened), (h, w) or
    (n, h, w); ``gt``: a number or an array like ``re``; ``max_l1``, ``overexposed``: see ``resolve_max_l1``;
    ``colorbar``: 'u', 'd', 'l', 'r', 'auto' (the shorter side: left or down) or None, (h + w) // 100 wide.

    Raises ``TypeError`` for uint16 (the reference's subtraction wraps) and ``ValueError`` for NaN or infinite depths."""
    import torch
    was_np = is_np(re)
    l1, valid, limit, flag, n, h, w, batched = _l1_planes(re, gt, max_l1, overexposed, colorbar)
    dst = torch.empty(((n,) if batched else ()) + (h, w, 3), dtype=torch.uint8, device=l1.device)
    call("camd_vis_l1_colour", l1.device, l1.data_ptr(), valid.data_ptr(), h * w, n, limit.data_ptr(), int(bool(overexposed)),
         dst.data_ptr(), what="vis_depth_l1")
    _raise_if_non_finite(flag)
    return to_caller(dst, was_np)


# ---- vis_stereo / vis_align --------------------------------------------------------------------------------------------
def line_table(size, n_line, thickness=0.03):
    """(size,) int8: the colour index (i % 6) of the line ``vis_stereo``'s loop (utils.py:689-694) paints over each row of
    a picture ``size`` rows high, -1 where there is none; a later line overwrites an earlier one, and a slice that starts
    before row 0 is Python's (it counts from the end)."""
    t = np.full(size, -1, np.int8)
    _thickness = max(1, int(round(thickness * size / (n_line + 1))))
    gap = size / (n_line + 1)
    for i in range(n_line):
        b = int((i + 1) * gap - _thickness / 2)
        t[b:b + _thickness] = i % 6
    return t


def _picture_shape(img, what):
    """An input of vis_stereo / vis_align checked before the device is touched -> (n, h, w, cn, batched, depth's type name
    or None).  uint8: (h, w), (h, w, 3), (n, h, w) or (n, h, w, 3).  Anything else is a depth, (h, w) or (n, h, w)."""
    check_array(img, what)
    if dtype_name(img) != "uint8":
        n, h, w, batched, name = _plane(img, what, _DEPTH_TYPES)
        return n, h, w, 3, batched, name
    shape = tuple(img.shape)
    if len(shape) not in (2, 3, 4) or min(shape) <= 0 or (len(shape) == 4 and shape[-1] != 3):
        raise ValueError("%s must be (h, w), (h, w, 3), (n, h, w) or (n, h, w, 3), got %s" % (what, shape))
    cn = 3 if len(shape) == 4 or (len(shape) == 3 and shape[-1] == 3) else 1
    batched = len(shape) - (cn == 3) == 3
    h, w = shape[-3:-1] if cn == 3 else shape[-2:]
    return (int(shape[0]) if batched else 1), int(h), int(w), cn, batched, None


def _picture(img, what, n, h, w, name, device=None):
    """The packed uint8 tensor of a checked input; a depth becomes norma, uint8(. * 255.999) (``boxx.uint8`` as
    recalled) and JET * 0.75 in BGR order, as ``_to_3x_uint8`` does."""
    t = to_device(img, device=device)
    if name is None:
        return t
    table = _device_table(_jet_bgr_075(), t.device)
    return _depth_picture(t, name, n, h * w, table, range_mode=_RANGE_NORMA, scale=255.999, zero_mask=False, what=what)


def _lines(img1, img2, n_line, thickness, tiles):
    import torch
    check_array(img1, "img1")
    check_array(img2, "img2")
    if is_np(img1) != is_np(img2):
        raise TypeError("img1 and img2 must both be NumPy arrays or both be CUDA tensors")
    n_line = int(n_line)
    if n_line < 0:
        raise ValueError("n_line must not be negative")
    n, h, w, cn1, batched, name1 = _picture_shape(img1, "img1")
    n2, h2, w2, cn2, batched2, name2 = _picture_shape(img2, "img2")
    if (n, h, w, batched) != (n2, h2, w2, batched2):
        raise ValueError("img1 and img2 must have one size: %s and %s" % (tuple(img1.shape), tuple(img2.shape)))
    a = _picture(img1, "img1", n, h, w, name1)
    b = _picture(img2, "img2", n, h, w, name2, device=a.device)
    rows = torch.from_numpy(line_table(h, n_line, thickness)).to(a.device)
    cols = None
    if tiles == 4:  # the two rot90s of vis_align: row r of the turned mosaic is column 2 w - 1 - r
        cols = torch.from_numpy(line_table(2 * w, int(n_line * w * 2 / h))[::-1].copy()).to(a.device)
        dst = torch.empty(((n,) if batched else ()) + (4, h, w, 3), dtype=torch.uint8, device=a.device)
        pitch, tile, image = w * 3, h * w * 3, 4 * h * w * 3
    else:
        dst = torch.empty(((n,) if batched else ()) + (h, 2 * w, 3), dtype=torch.uint8, device=a.device)
        pitch, tile, image = 2 * w * 3, w * 3, 2 * h * w * 3
    call("camd_vis_lines", a.device, a.data_ptr(), cn1, b.data_ptr(), cn2, w, h, n, rows.data_ptr(),
         None if cols is None else cols.data_ptr(), tiles, dst.data_ptr(), pitch, tile, image, what="vis_stereo")
    return dst, batched


def vis_stereo(img1, img2, n_line=21, thickness=0.03):
    """``utils.vis_stereo`` (utils.py:673-695): the two pictures side by side under ``n_line`` coloured lines -> uint8
    (..., h, 2 w, 3).  Both pictures have one size; see ``vis_align`` for what a picture may be."""
    dst, _ = _lines(img1, img2, n_line, thickness, 2)
    return to_caller(dst, is_np(img1))


def vis_align(img1, img2, n_line=21):
    """``utils.vis_align`` (utils.py:698-719, without ``shows``): [img1, img2, img2, img1], each (..., h, w, 3), the four
    tiles of the mosaic img1 | img2 over img2 | img1 under ``n_line`` row lines per half and
    ``int(n_line * w * 2 / h)`` column lines, which win.  A picture is uint8 -- (h, w) gray (replicated), (h, w, 3), or
    batches (n, h, w) / (n, h, w, 3) -- or a depth (float64, float32, uint16; (h, w) or (n, h, w)), shown as the
    reference's ``_to_3x_uint8`` shows it."""
    dst, batched = _lines(img1, img2, n_line, 0.03, 4)
    out = to_caller(dst, is_np(img1))
    return [out[:, t] if batched else out[t] for t in range(4)]
