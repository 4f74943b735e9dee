"""``calibrating/flow_utils.py`` on the GPU: ``warp_flow`` (flow_utils.py:98-129) and, under the names the reference
keeps them here, ``flow_abs_to_normal`` / ``flow_normal_to_abs`` (:83-95; they live in ``epipolar_geometry``).

``vis_flow`` is not offered: its arithmetic is cv2's (cartToPolar, normalize, cvtColor) and its arrows are random host
drawing.
"""
from ._arrays import FLOAT_TYPES, check_array, dtype_name, is_np, to_caller, to_device
from ._native import INTER_LANCZOS4, INTER_LINEAR, INTER_NEAREST, call
from .epipolar_geometry import flow_abs_to_normal, flow_normal_to_abs
from .resize import resize

__all__ = ["warp_flow", "flow_abs_to_normal", "flow_normal_to_abs"]

_INTERPOLATIONS = (INTER_NEAREST, INTER_LINEAR, INTER_LANCZOS4)


def _check(flow, img, what, interpolation):
    """Everything that can be refused before the device is touched -> (n, h, w, batched, flow's dtype name)."""
    check_array(flow, "flow")
    check_array(img, what)
    if is_np(flow) != is_np(img):
        raise TypeError("flow and %s must both be NumPy arrays or both be CUDA tensors" % what)
    name = dtype_name(flow)
    if name not in FLOAT_TYPES:
        raise TypeError("flow must be float32 or float64, got %s" % name)
    if dtype_name(img) != "uint8":
        raise TypeError("%s must be uint8, got %s" % (what, dtype_name(img)))
    batched = len(flow.shape) == 4
    if len(flow.shape) not in (3, 4) or flow.shape[-3] != 2 or min(flow.shape) <= 0:
        raise ValueError("flow must be (2, h, w) or (n, 2, h, w), got %s" % (tuple(flow.shape),))
    n, (h, w) = (flow.shape[0] if batched else 1), flow.shape[-2:]
    if len(img.shape) not in ((4,) if batched else (2, 3)):
        want = "(n, H, W, c)" if batched else "(H, W) or (H, W, 3)"
        raise ValueError("%s must be %s for a flow of shape %s, got %s" % (what, want, tuple(flow.shape), tuple(img.shape)))
    if batched and img.shape[0] != n:
        raise ValueError("%d flows but %d images in %s" % (n, img.shape[0], what))
    cn = 1 if len(img.shape) == 2 else img.shape[-1]
    if cn not in (1, 3) or min(img.shape) <= 0:
        raise ValueError("%s must have 1 or 3 channels and no empty side, got %s" % (what, tuple(img.shape)))
    if int(interpolation) not in _INTERPOLATIONS:
        raise ValueError("interpolation %r not implemented: INTER_NEAREST, INTER_LINEAR or INTER_LANCZOS4" % (interpolation,))
    return int(n), int(h), int(w), batched, name


def warp_flow(flow, img1=None, img2=None, interpolation=INTER_LINEAR):
    """``flow_utils.warp_flow(flow, img1, img2, interpolation)`` (flow_utils.py:98-129) on the GPU.

    ``flow``: normalised, (2, h, w) -- x in units of w, y in units of h -- or (n, 2, h, w) for a batch, float32 or
    float64.  Images: uint8 (H, W), (H, W, 3), or (n, H, W, c) with a batch.  NumPy in -> NumPy out; CUDA tensors in ->
    a tensor on their device and its current stream, without a synchronisation.  Pixel (x, y) moves to
    ``x + flow_x * w``, ``y + flow_y * h``, evaluated in float64 whatever the flow's type, as NumPy does.

    ``img2`` (the next frame; recommended): it is brought to (h, w) with ``resize`` when its size differs, then sampled
    at the float32 of those positions like ``cv2.remap(..., interpolation)`` with a zero border -> (h, w[, c]): the
    previous frame as seen through the flow.  Where the position is NaN, infinite or beyond int32 after cv2's * 32 the
    pixel is 0.

    ``img1`` (the previous frame; wins when both are given): every pixel with a non-zero flow whose rounded (half to
    even) target lies inside (h, w) is pushed there; of several on one target the last in row-major order stays, as in
    NumPy's assignment, and identical calls give identical bytes.  Targets nobody reached show their own position of
    ``img1``, positions outside ``img1`` (its size may differ from (h, w)) are 0.  The result does not depend on
    ``interpolation``: the map holds integers.  A pixel whose target is NaN, infinite or beyond int32 is not pushed."""
    import torch
    if img1 is None and img2 is None:
        raise ValueError("warp_flow needs img1 (push the previous frame forward) or img2 (pull the next frame back)")
    forward = img1 is not None
    img, what = (img1, "img1") if forward else (img2, "img2")
    n, h, w, batched, name = _check(flow, img, what, interpolation)
    was_np = is_np(flow)
    f = to_device(flow)
    s = to_device(img, device=f.device)
    if not forward:
        s = resize(s, (h, w), batched=batched)
    sh, sw = s.shape[1:3] if batched else s.shape[:2]
    cn = 1 if s.dim() == 2 else s.shape[-1]
    dst = torch.empty(((n,) if batched else ()) + (h, w) + (() if s.dim() == 2 else (cn,)), dtype=torch.uint8,
                      device=s.device)
    if forward:
        winner = torch.empty((n, h, w), dtype=torch.int32, device=s.device)
        call("camd_warp_flow_forward_u8", s.device, s.data_ptr(), sw, sh, cn, sw * cn, sh * sw * cn, f.data_ptr(),
             FLOAT_TYPES[name], 2 * h * w, dst.data_ptr(), w, h, w * cn, h * w * cn, int(interpolation), winner.data_ptr(), n,
             what="warp_flow")
    else:
        call("camd_warp_flow_backward_u8", s.device, s.data_ptr(), cn, w * cn, h * w * cn, f.data_ptr(), FLOAT_TYPES[name],
             2 * h * w, dst.data_ptr(), w, h, w * cn, h * w * cn, int(interpolation), n, what="warp_flow")
    return to_caller(dst, was_np)
