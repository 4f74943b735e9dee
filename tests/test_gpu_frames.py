"""The frame layer on the MI355X (-m gpu): for every front end that reads frames through ``calibrating_amd/_frames.py``, a
pitched view -- a crop of a wider batch, rows and frames apart -- gives the bits of its contiguous copy and of the same
pixels handed over as a NumPy array."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from calibrating_amd import features, imgproc  # noqa: E402

CROP = (slice(1, 3), slice(4, 52), slice(8, 72))  # 2 frames of 48 x 64 out of (3, 64, 96)


@pytest.fixture(scope="module")
def sources():
    rng = np.random.default_rng(11)
    return {"gray": rng.integers(0, 256, (3, 64, 96), dtype=np.uint8), "colour": rng.integers(0, 256, (3, 64, 96, 3), dtype=np.uint8)}


def host(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def same(got, exp):
    got, exp = (tuple(v) if isinstance(v, (tuple, list)) else (v,) for v in (got, exp))
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g, e = host(g), host(e)
        assert g.dtype == e.dtype and g.shape == e.shape, (g.dtype, g.shape, e.dtype, e.shape)
        assert np.array_equal(g.reshape(-1).view(np.uint8), e.reshape(-1).view(np.uint8))


def three_ways(call, source, single=True):
    """``call(images, to)`` on the pitched view, on its contiguous copy and on the NumPy crop -- ``to`` turns an ndarray
    into the kind of ``images`` -- and, with ``single``, on one frame of the view: rows apart, no batch axis."""
    view = torch.from_numpy(source).cuda()[CROP]
    assert not view.is_contiguous() and tuple(view.shape[:3]) == (2, 48, 64)
    cuda = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    pitched = call(view, cuda)
    parts = pitched if isinstance(pitched, tuple) else (pitched,)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in parts)
    same(pitched, call(view.contiguous(), cuda))
    same(pitched, call(np.ascontiguousarray(source[CROP]), lambda a: a))
    if single:
        one = call(view[1], cuda)
        same(one, tuple(v[1] for v in parts) if isinstance(one, tuple) else parts[0][1])
    return pitched


@pytest.mark.parametrize("code", ["bgr", "rgb"])
def test_cvt_gray(sources, code):
    gray = three_ways(lambda images, to: imgproc.cvt_gray(images, code), sources["colour"])
    assert gray.dtype == torch.uint8 and tuple(gray.shape) == (2, 48, 64)


@pytest.mark.parametrize("kind", ["gray", "colour"])
def test_the_stages_that_read_frames(sources, kind):
    source = sources[kind]
    r, rmax = three_ways(lambda images, to: imgproc.chess_response(images), source)
    assert r.dtype == torch.int16 and tuple(r.shape) == (2, 48, 64) and int(rmax.min()) > 0
    mask = three_ways(lambda images, to: imgproc.dark_mask(images), source)
    assert 0 < int(mask.sum()) < mask.numel()
    sums = three_ways(lambda images, to: imgproc.laplacian_sums(images), source)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (2, 2) and int(sums[:, 1].min()) > 0
    score = three_ways(lambda images, to: features._score_plane(images), source)
    assert score.dtype == torch.uint8 and int(score.count_nonzero()) > 0


@pytest.mark.parametrize("kind", ["gray", "colour"])
def test_corner_sub_pix(sources, kind):
    corners = np.array([[[13.0, 13.0], [31.5, 24.25], [50.0, 34.0], [20.75, 30.5]],
                        [[40.0, 20.0], [14.5, 33.0], [49.25, 13.5], [32.0, 32.0]]], np.float32)
    out = three_ways(lambda images, to: imgproc.corner_sub_pix(images, to(corners), return_info=True), sources[kind], single=False)
    assert out[0].dtype == torch.float32 and tuple(out[0].shape) == (2, 4, 2) and tuple(out[2].shape) == (2, 4)
