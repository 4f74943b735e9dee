"""``_native.call`` on the MI355X (-m gpu): it launches on the device it is given and on THAT device's current stream,
and maps a refused argument to the exception under the caller's label."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import _native, imgproc  # noqa: E402


def _image(device="cuda"):
    rng = np.random.default_rng(7)
    return torch.from_numpy(rng.integers(-64, 4096, (8, 8), dtype=np.int16)).to(device)


def _median_through_call(src):
    dst = torch.empty_like(src)
    _native.call("camd_median3_s16", src.device, src.data_ptr(), dst.data_ptr(), 8, 8, 1)
    return dst


def test_call_equals_the_front_end():
    src = _image()
    assert torch.equal(_median_through_call(src), imgproc.medianBlur3_s16(src))


def test_call_takes_the_ambient_stream_of_the_device():
    src = _image()
    want = imgproc.medianBlur3_s16(src)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert _native.current_stream().value == side.cuda_stream
        got = _median_through_call(src)
    side.synchronize()
    assert torch.equal(got, want)


def test_a_refused_argument_raises_under_the_label():
    src = _image()
    dst = torch.empty_like(src)
    with pytest.raises(ValueError, match=r"^the label: "):
        _native.call("camd_median3_s16", src.device, src.data_ptr(), dst.data_ptr(), 0, 8, 1, what="the label")
    with pytest.raises(ValueError, match=r"^camd_median3_s16: "):
        _native.call("camd_median3_s16", src.device, src.data_ptr(), dst.data_ptr(), -1, 8, 1)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_the_tensor_decides_the_device_not_the_current_one():
    src = _image("cuda:1")
    rng = np.random.default_rng(11)
    left = torch.from_numpy(rng.integers(0, 256, (32, 64), dtype=np.uint8)).to("cuda:1")
    right = torch.roll(left, -3, 1)
    with torch.cuda.device(1):
        want = imgproc.medianBlur3_s16(src)
        ref = ca.StereoSGBM_create(numDisparities=16)
        ref.compute(left, right)
        want_raw = ref.debug_volume("raw")
        torch.cuda.synchronize()
    with torch.cuda.device(0):
        got = imgproc.medianBlur3_s16(src)
        sgbm = ca.StereoSGBM_create(numDisparities=16)
        sgbm.compute(left, right)
        got_raw = sgbm.debug_volume("raw")
        sgbm.status()
        torch.cuda.synchronize(1)
    assert got.device == src.device and torch.equal(got, want)
    assert got_raw.device == src.device and got_raw.shape == (32, 64) and torch.equal(got_raw, want_raw)
