"""The frame layer every image front end shares (``calibrating_amd/_frames.py``), on the host: the layout read off a shape
and its refusals, the side limits as arguments, pitched views read in place, the integer rule and the epilogue."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from calibrating_amd import _frames  # noqa: E402
from calibrating_amd._frames import device_frames, integer, layout, to_result  # noqa: E402

# shape -> (colour, batched, f, h, w)
ACCEPTED = [((48, 64), (False, False, 1, 48, 64)), ((2, 48, 64), (False, True, 2, 48, 64)),
            ((48, 64, 3), (True, False, 1, 48, 64)), ((2, 48, 64, 3), (True, True, 2, 48, 64))]


def broadcast(shape):
    """a uint8 array of ``shape`` that owns one byte"""
    return np.broadcast_to(np.zeros(1, np.uint8), shape)


@pytest.mark.parametrize("make", [lambda s: np.zeros(s, np.uint8), lambda s: torch.zeros(s, dtype=torch.uint8)], ids=["numpy", "cpu-tensor"])
def test_the_four_shapes_and_the_refusals(make):
    for shape, want in ACCEPTED:
        got = layout(make(shape), "images")
        assert (got.colour, got.batched, got.f, got.h, got.w) == want and got.data is None
        assert got.was_np == isinstance(make((1, 1)), np.ndarray)
    for shape in [(64,), (1, 1, 2, 48, 64), (2, 3, 48, 64), (0, 64), (48, 0), (0, 48, 64), (2, 0, 64, 3)]:
        with pytest.raises(ValueError):
            layout(make(shape), "images")
    img = make((48, 64))
    with pytest.raises(ValueError, match="uint8"):
        layout(img.astype(np.float32) if isinstance(img, np.ndarray) else img.float(), "images")


def test_what_is_no_array_is_a_type_error_and_the_rows_have_a_limit():
    for bad in ([[0, 1], [2, 3]], None, 7):
        with pytest.raises(TypeError):
            layout(bad, "images")
    assert layout(broadcast((2 ** 20, 2 ** 11 - 1, 4)), "images").f == 2 ** 20
    with pytest.raises(ValueError, match="2\\^31"):
        layout(broadcast((2 ** 20, 2 ** 11, 4)), "images")
    with pytest.raises(ValueError, match="2\\^31"):
        layout(broadcast((2 ** 31, 4)), "images")


def test_the_side_limits_are_arguments():
    for shape in [(16384, 16384), (2, 16384, 7), (7, 16384, 3), (2, 7, 16384, 3)]:
        assert layout(broadcast(shape), "images", max_side=16384)
    for shape in [(16385, 7), (7, 16385), (2, 16385, 7), (16385, 7, 3), (2, 7, 16385, 3)]:
        with pytest.raises(ValueError):
            layout(broadcast(shape), "images", max_side=16384)
        assert layout(broadcast(shape), "images")  # no limit given, none applied
    square = broadcast((16384, 16384))
    assert layout(square, "images", min_side=16384)[1:4] == (1, 16384, 16384)
    with pytest.raises(ValueError):
        layout(square, "images", min_side=16385)
    for shape in [(2, 48), (48, 2), (3, 2, 48), (2, 48, 3)]:
        with pytest.raises(ValueError):
            layout(broadcast(shape), "images", min_side=3)
    assert layout(broadcast((3, 3)), "images", min_side=3, max_side=3)


def test_a_pitched_view_is_read_in_place():
    big = torch.arange(3 * 64 * 96, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(3, 64, 96)
    view = big[1:3, 4:52, 8:72]
    assert not view.is_contiguous()
    fr = device_frames(view, layout(view, "images"))
    assert (fr.f, fr.h, fr.w, fr.pitch, fr.stride, fr.batched, fr.was_np) == (2, 48, 64, 96, 64 * 96, True, False)
    assert fr.data.data_ptr() == view.data_ptr() == big.data_ptr() + 64 * 96 + 4 * 96 + 8
    one = device_frames(view[1], layout(view[1], "images"))
    assert (one.f, one.h, one.w, one.pitch, one.batched) == (1, 48, 64, 96, False) and one.data.data_ptr() == view[1].data_ptr()
    # every second frame: the frames are further apart, still no copy
    apart = big[::2, 4:52, 8:72]
    fr = device_frames(apart, layout(apart, "images"))
    assert (fr.pitch, fr.stride) == (96, 2 * 64 * 96) and fr.data.data_ptr() == apart.data_ptr()
    # colour stays 3 interleaved channels without a code: the same rule in bytes
    colour = torch.zeros((3, 64, 96, 3), dtype=torch.uint8)[1:3, 4:52, 8:72]
    fr = device_frames(colour, layout(colour, "images"))
    assert (fr.f, fr.h, fr.w, fr.pitch, fr.stride) == (2, 48, 64, 96 * 3, 64 * 96 * 3) and fr.data.data_ptr() == colour.data_ptr()


def test_pixels_that_are_apart_are_made_contiguous():
    big = torch.arange(3 * 64 * 96, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(3, 64, 96)
    for view in (big[:, :, ::2], big.transpose(1, 2), big[:, :, :, None].expand(3, 64, 96, 3)):
        assert view.stride(-1) != 1
        lay = layout(view, "images")
        fr = device_frames(view, lay)
        channels = 3 if lay.colour else 1
        assert fr.data.is_contiguous() and torch.equal(fr.data, view)
        assert (fr.pitch, fr.stride) == (lay.w * channels, lay.h * lay.w * channels)


def test_the_integer_rule():
    assert integer(3, "n") == 3 and integer(3.0, "n") == 3 and integer(np.int32(4), "n", (1, 4)) == 4
    assert type(integer(np.int64(5), "n")) is int
    for bad in (True, False, 2.5):
        with pytest.raises(ValueError, match="n must be an integer"):
            integer(bad, "n")
    for bad in (3.0, True, np.float32(2)):
        with pytest.raises(ValueError):
            integer(bad, "n", strict=True)
    assert integer(np.uint8(7), "n", (0, 7), strict=True) == 7
    for bad in (0, 5):
        with pytest.raises(ValueError, match="n must be 1 .. 4"):
            integer(bad, "n", (1, 4))


def test_the_epilogue_drops_the_batch_axis_of_one_image():
    found, corners = torch.tensor([True]), torch.zeros((1, 6, 2))
    out = to_result((found, corners), False, False)
    assert out[0].shape == () and out[1].shape == (6, 2)
    out = to_result((found, corners), True, False)
    assert out[0] is found and out[1] is corners
    assert to_result(corners, False, False).shape == (6, 2) and to_result(corners, True, False) is corners
    info = to_result(dict(status=torch.zeros(1), quads=torch.zeros((1, 4, 2))), False, False)
    assert info["status"].shape == () and info["quads"].shape == (4, 2)
    assert _frames.GRAY_WEIGHTS[_frames.GRAY_BITS] == (3735, 19235, 9798)
