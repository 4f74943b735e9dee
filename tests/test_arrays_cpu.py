"""The shared array hand-over (calibrating_amd/_arrays.py) without a GPU: what it refuses is refused before the library
or the device is reached, and the small-argument helpers marshal what the C ABI reads."""
import numpy as np
import pytest

from calibrating_amd import _arrays, _native


@pytest.fixture
def no_device_call(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_native, "require_device", refuse)
    monkeypatch.setattr(_native, "lib", refuse)


def test_bad_arrays_are_refused_before_any_device_call(no_device_call):
    import torch
    with pytest.raises(TypeError, match="x must be a NumPy array or a torch CUDA tensor, got list"):
        _arrays.check_array([1, 2], "x")
    with pytest.raises(TypeError, match="got list"):
        _arrays.to_device([1, 2])
    with pytest.raises(ValueError, match=r"live on the GPU \(x\)"):
        _arrays.check_array(torch.zeros(3), "x")
    with pytest.raises(ValueError, match="live on the GPU"):
        _arrays.to_device(torch.zeros(3))
    with pytest.raises(ValueError, match="expected dtype torch.uint8, got torch.float64"):
        _arrays.to_device(np.zeros(3), dtype="uint8")
    with pytest.raises(ValueError, match="expected dtype torch.int16, got torch.float32"):
        _arrays.to_device(np.zeros((2, 2), np.float32), dtype="int16")
    _arrays.check_array(np.zeros(3), "x")  # an ndarray passes, and nothing was touched


def test_small_arguments():
    D, ptr, n = _arrays.dist(None)
    assert D.size == 0 and D.dtype == np.float64 and ptr is None and n == 0
    D, ptr, n = _arrays.dist([[0.1, 0.2, 0, 0, 0.3]])
    assert D.shape == (5,) and D.dtype == np.float64 and ptr == D.ctypes.data and n == 5
    P = np.arange(12, dtype=np.float32).reshape(3, 4)
    K = _arrays.K9(P)
    assert K.dtype == np.float64 and K.flags.c_contiguous and np.array_equal(K, P[:, :3].reshape(9))
    assert np.allclose(_arrays.Kinv9(np.diag([2.0, 4.0, 1.0])), np.diag([0.5, 0.25, 1.0]).reshape(9))
    assert np.array_equal(_arrays.mat(np.eye(4), 16), np.eye(4).reshape(16))
    with pytest.raises(ValueError, match="expected 16 matrix entries, got 12"):
        _arrays.mat(P, 16)
    with pytest.raises(ValueError, match="positive"):
        _arrays.positive_wh((0, 4))
    assert _arrays.positive_hw((3, 4)) == (3, 4)


def test_value_types_agree_with_the_binding():
    assert _arrays.VALUE_TYPES == {"float64": _native.VALUE_F64, "float32": _native.VALUE_F32, "uint8": _native.VALUE_U8}
    assert _arrays.FLOAT_TYPES == {"float64": _native.VALUE_F64, "float32": _native.VALUE_F32}
    assert _arrays.DIST_COUNTS == (0, 4, 5, 8, 12, 14)
