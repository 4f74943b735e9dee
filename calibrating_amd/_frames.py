"""The one statement of how uint8 frames reach the image kernels: ``layout`` (host: gray or colour, one or a batch, the
sizes and every refusal) -> ``device_frames`` (upload, colour to gray, rows read in place) -> the kernels -> ``to_result``
(the batch axis dropped for one image, the caller's kind).  ``integer`` is the argument check the front ends share."""
from typing import Any, NamedTuple

import numpy as np

from . import _native
from ._arrays import check_array, is_np, dtype_name, to_caller
from ._native import call

# cv2's fixed-point weights of B, G, R and their shift, by the bits of the fixed point (recalled,
# unpinned).  OpenCV 4.x: 15 bits, older releases: 14.  GRAY_BITS is the switch.
GRAY_WEIGHTS = {15: (3735, 19235, 9798), 14: (1868, 9617, 4899)}
GRAY_BITS = 15


class Frames(NamedTuple):
    """Frames as the kernels take them: ``data`` is a uint8 CUDA tensor of ``f`` frames of ``h`` x ``w`` pixels, gray or
    (``colour``) 3 interleaved channels, rows ``pitch`` and frames ``stride`` bytes apart (these three: ``device_frames``)."""
    data: Any
    f: int
    h: int
    w: int
    pitch: int
    stride: int
    batched: bool
    was_np: bool
    colour: bool


def integer(v, name, within=None, strict=False):
    """``int(v)`` of an argument that is a whole number and no bool -- ``strict``: of an integer type, so ``3.0`` is
    refused -- and lies in ``within`` = (lowest, highest) where given; else ValueError."""
    if isinstance(v, bool) or (not isinstance(v, (int, np.integer)) if strict else int(v) != v):
        raise ValueError("%s must be an integer, got %r" % (name, v))
    if within is not None and not within[0] <= v <= within[1]:
        raise ValueError("%s must be %d .. %d, got %d" % (name, within[0], within[1], v))
    return int(v)


def layout(images, what, max_side=None, min_side=None):
    """``Frames`` without their data (``data`` None, ``pitch`` and ``stride`` 0 until ``device_frames``) of uint8 images (h, w),
    (f, h, w), (h, w, 3) or (f, h, w, 3) -- a last axis of 3 is colour: no gray image a kernel here takes is 3 wide -- with sides
    in ``min_side .. max_side`` where given, or the refusal.  Host only: a tensor may be on any device; nothing is touched."""
    if not is_np(images) and not (hasattr(images, "is_cuda") and hasattr(images, "data_ptr")):
        raise TypeError("%s must be a NumPy array or a torch CUDA tensor, got %s" % (what, type(images).__name__))
    if dtype_name(images) != "uint8":
        raise ValueError("%s must be uint8, got %s" % (what, images.dtype))
    shape = tuple(int(v) for v in images.shape)
    colour = len(shape) in (3, 4) and shape[-1] == 3
    if len(shape) not in (2, 3, 4) or (len(shape) == 4 and not colour):
        raise ValueError("%s must be (h, w), (f, h, w), (h, w, 3) or (f, h, w, 3), got %s" % (what, shape))
    if 0 in shape:
        raise ValueError("%s is empty: %s" % (what, shape))
    batched = len(shape) - colour == 3
    h, w = shape[-3:-1] if colour else shape[-2:]
    f = shape[0] if batched else 1
    if max_side is not None and max(h, w) > max_side:
        raise ValueError("%s of %s; the detector takes sides up to %d" % (what, shape, max_side))
    if min_side is not None and min(h, w) < min_side:
        raise ValueError("%s of %s; the detector takes sides from %d" % (what, shape, min_side))
    if f * h >= 2 ** 31:
        raise ValueError("%s: %d rows in all, the kernels take fewer than 2^31" % (what, f * h))
    return Frames(None, f, h, w, 0, 0, batched, is_np(images), colour)


def _rows(t, lay, channels):
    """``lay`` with the tensor (h, w[, 3]) or (f, h, w[, 3]) as its data: the tensor itself where its pixels are contiguous
    -- rows and images may be apart by more than their bytes (a crop, a slice of a wider batch) -- else its contiguous copy."""
    lead = t.dim() - (3 if channels == 3 else 2)
    f, h, w = lay.f, lay.h, lay.w
    st = t.stride()
    tight = (st[-1] == 1 and st[-2] == 3) if channels == 3 else st[-1] == 1
    pitch = int(st[lead]) if h > 1 else w * channels
    stride = int(st[0]) if lead and f > 1 else h * pitch
    if not tight or pitch < w * channels or stride < (h - 1) * pitch + w * channels:
        t = t.contiguous()
        pitch, stride = w * channels, h * w * channels
    return Frames(t, f, h, w, pitch, stride, lay.batched, lay.was_np, channels == 3)


def _gray(fr, code):  # -> (f, h, w) uint8: the gray of 3-channel frames
    import torch
    by, gy, ry = GRAY_WEIGHTS[GRAY_BITS]
    k = (by, gy, ry) if code == "bgr" else (ry, gy, by)
    dst = torch.empty((fr.f, fr.h, fr.w), dtype=torch.uint8, device=fr.data.device)
    call("camd_bgr_to_gray_u8", dst.device, fr.data.data_ptr(), fr.w, fr.h, fr.pitch, fr.stride, dst.data_ptr(), fr.w, fr.h * fr.w,
         fr.f, k[0], k[1], k[2], GRAY_BITS, what="cvt_gray")
    return dst


def device_frames(images, lay, code=None):
    """The ``Frames`` of images that passed ``layout`` as ``lay``.  An ndarray is uploaded; a tensor is read in place, made
    contiguous only where its pixels are apart.  ``code`` "bgr" or "rgb": colour goes to gray with the first channel taken
    as blue or red; None: colour stays 3 channels."""
    import torch
    if lay.was_np:
        _native.require_device()
    t = torch.from_numpy(np.ascontiguousarray(images)).cuda() if lay.was_np else images
    if lay.colour:
        fr = _rows(t, lay, 3)
        if code is None:
            return fr
        t = _gray(fr, code)
        t = t if lay.batched else t[0]
    return _rows(t, lay, 1)


def gray_frames(images, what="images", code="bgr", max_side=None, min_side=None):
    """``check_array`` -> ``layout`` -> ``device_frames``: gray frames of a front end's images, every refusal first."""
    check_array(images, what)
    return device_frames(images, layout(images, what, max_side, min_side), code)


def cvt_gray(img, code="bgr"):
    """cv2.cvtColor(img, cv2.COLOR_BGR2GRAY) (``code="bgr"``) or COLOR_RGB2GRAY (``"rgb"``) on uint8, on the GPU:
    (h, w, 3) or (f, h, w, 3) -> (h, w) or (f, h, w).  The first channel gets blue's weight with "bgr" and red's with
    "rgb"; the reference hands an RGB image to COLOR_BGR2GRAY (boards.py:159), which ``Chessboard`` repeats.  Weights:
    ``GRAY_WEIGHTS[GRAY_BITS]`` (U32).  A tensor whose rows or images are apart (a crop) is read in place."""
    check_array(img, "img")
    if code not in ("bgr", "rgb"):
        raise ValueError("code must be 'bgr' or 'rgb', got %r" % (code,))
    lay = layout(img, "img")
    if not lay.colour:
        raise ValueError("img must be (h, w, 3) or (f, h, w, 3), got %s" % (tuple(img.shape),))
    return to_result(_gray(device_frames(img, lay), code), lay.batched, lay.was_np)


def to_result(out, batched, was_np):
    """What a front end hands back for a tensor, a tuple of tensors or a dict of them, each with the frames leading: the
    batch axis goes for a single image, NumPy callers get host copies (a tuple in one synchronisation), and a single NumPy
    image's 0-d bool -- its ``found`` -- is a Python bool."""
    if isinstance(out, dict):
        return {k: to_result(v, batched, was_np) for k, v in out.items()}
    if not isinstance(out, tuple):
        return to_caller(out if batched else out[0], was_np)
    out = to_caller(out if batched else tuple(v[0] for v in out), was_np)
    if was_np and not batched:
        out = tuple(bool(v) if v.ndim == 0 and v.dtype == np.bool_ else v for v in out)
    return out
