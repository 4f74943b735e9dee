"""The one hand-over of arrays and small arguments between a caller and the library (DESIGN.md "How a front end calls
the library"): ``check_array`` -> argument checks -> ``to_device`` -> ``_native.call`` -> ``to_caller``.

Arrays are ndarrays (copied to the GPU and back) or torch CUDA tensors (zero-copy).  Matrices, distortion vectors and
sizes are small host arrays the C ABI reads through a pointer: the helpers below return float64, flat, contiguous arrays
that the caller keeps alive across the call.
"""
import numpy as np

from . import _native, hostio

# dtype name -> value_type / uv_type / z_type of the C ABI
VALUE_TYPES = {"float64": _native.VALUE_F64, "float32": _native.VALUE_F32, "uint8": _native.VALUE_U8}
FLOAT_TYPES = {k: VALUE_TYPES[k] for k in ("float64", "float32")}
DIST_COUNTS = (0, 4, 5, 8, 12, 14)  # the distortion vectors cv2 takes


def is_np(a):
    return isinstance(a, np.ndarray)


def dtype_name(a):
    return str(a.dtype).replace("torch.", "")


def check_array(a, what):
    """ndarray or CUDA tensor, checked without touching the device."""
    if is_np(a):
        return
    if not (hasattr(a, "is_cuda") and hasattr(a, "data_ptr")):
        raise TypeError("%s must be a NumPy array or a torch CUDA tensor, got %s" % (what, type(a).__name__))
    if not a.is_cuda:
        raise ValueError("tensor inputs must live on the GPU (%s)" % what)


def to_device(a, *, dtype=None, cast=False, device=None):
    """Contiguous CUDA tensor of an ndarray (uploaded, to ``device`` if given) or a CUDA tensor (as it is).  ``dtype`` is
    a NumPy dtype name: ``cast=True`` converts to it, ``cast=False`` refuses anything else.  ``device``: where an earlier
    argument lives; a tensor elsewhere is refused.  Every refusal comes before the device is touched."""
    import torch
    if not is_np(a):
        if not (hasattr(a, "is_cuda") and hasattr(a, "data_ptr")):
            raise TypeError("expected a NumPy array or a torch CUDA tensor, got %s" % type(a).__name__)
        if not a.is_cuda:
            raise ValueError("tensor inputs must live on the GPU")
    if dtype is not None and not cast and dtype_name(a) != dtype:
        raise ValueError("expected dtype torch.%s, got torch.%s" % (dtype, dtype_name(a)))
    if is_np(a):
        _native.require_device()
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))
        return t.cuda() if device is None else t.to(device)
    if dtype is not None:
        a = a.to(getattr(torch, dtype))
    if device is not None and a.device != device:
        raise ValueError("inputs live on different devices: %s and %s" % (a.device, device))
    return a.contiguous()


def to_caller(t, was_np):
    """What the caller gets back: the tensor(s) themselves, or for ndarray input their host copies (one
    synchronisation).  A tuple of tensors in -> a tuple out."""
    if not was_np:
        return t
    return tuple(hostio.to_host_list(*t)) if isinstance(t, tuple) else hostio.to_host(t)


def mat(m, n):
    """``m`` as ``n`` float64 numbers, flat."""
    a = np.ascontiguousarray(m, np.float64).reshape(-1)
    if a.size != n:
        raise ValueError("expected %d matrix entries, got %d" % (n, a.size))
    return a


def K9(K):
    """The left 3x3 of a camera matrix (3x3, or the 3x4 of a projection), flat."""
    return mat(np.asarray(K, np.float64)[:3, :3], 9)


def Kinv9(K):
    return mat(np.linalg.inv(np.asarray(K, np.float64)[:3, :3]), 9)


def dist(D):
    """(float64 flat array, its address or None when empty, count) of a distortion vector (None = no distortion)."""
    D = np.zeros(0) if D is None else np.ascontiguousarray(D, np.float64).reshape(-1)
    return D, (D.ctypes.data if D.size else None), int(D.size)


def positive_wh(xy, what="xy"):
    w, h = int(xy[0]), int(xy[1])
    if w <= 0 or h <= 0:
        raise ValueError("%s must be a positive (width, height), got %s" % (what, (xy[0], xy[1])))
    return w, h


def positive_hw(hw, what="hw"):
    h, w = int(hw[0]), int(hw[1])
    if h <= 0 or w <= 0:
        raise ValueError("%s must be a positive (height, width), got %s" % (what, (hw[0], hw[1])))
    return h, w
