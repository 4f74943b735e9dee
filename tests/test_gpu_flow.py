"""warp_flow on the GPU (-m gpu), bit-equal throughout: against what the REFERENCE's own flow_utils.warp_flow returned
(tests/golden/reference_flow.npz) and, on shapes and values the fixture does not hold, against its NumPy restatement
tests/flow_ref.py (which tests/test_flow_cpu.py pins to that fixture)."""
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
import flow_cases as cases  # noqa: E402
import flow_ref  # noqa: E402

INTERPOLATIONS = (cases.INTER_NEAREST, cases.INTER_LINEAR, cases.INTER_LANCZOS4)


def _cuda(a):
    return torch.from_numpy(a).cuda()


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %d bytes differ" % (what, (got != want).sum())


def test_golden_cases(oracle):
    fx = cases.load_fixture()
    assert fx is not None
    for name, (flow, img2, interp) in cases.backward_cases().items():
        _same(ca.warp_flow(flow, img2=img2, interpolation=interp), fx[name], name)
        got = ca.warp_flow(_cuda(flow), img2=_cuda(img2), interpolation=interp)
        assert got.is_cuda
        _same(got.cpu().numpy(), fx[name], name + " (tensors)")
    for name, (flow, img1) in cases.forward_inputs().items():
        for tag, interp in cases.FORWARD_INTERPOLATIONS + (("linear", cases.INTER_LANCZOS4),):
            want = fx["%s/%s" % (name, tag)]
            _same(ca.warp_flow(flow, img1=img1, interpolation=interp), want, (name, interp))
            _same(ca.warp_flow(_cuda(flow), _cuda(img1), None, interp).cpu().numpy(), want, (name, interp, "tensors"))
    # img1 wins when both are given; the default interpolation is INTER_LINEAR
    flow, img1 = cases.forward_inputs()["f_outside"]
    _same(ca.warp_flow(flow, img1, cases.image(2, cn=3)), fx["f_outside/linear"], "img1 wins")
    flow, img2, _ = cases.backward_cases()["b_gray_f32_linear"]
    _same(ca.warp_flow(flow, img2=img2), fx["b_gray_f32_linear"], "default interpolation")


def test_a_batch_equals_single_calls(oracle):
    flows = np.stack([cases.smooth_flow(np.float32, seed=s) for s in range(3)])
    gray = np.stack([cases.image(20 + s, cn=1) for s in range(3)])[..., None]
    rgb = np.stack([cases.image(23 + s, cn=3) for s in range(3)])
    big = np.stack([cases.image(26 + s, cases.DOUBLE, cn=3) for s in range(3)])  # backward: one batched resize first
    for batch in (gray, rgb, big):
        for key in ("img2", "img1"):
            for interp in (INTERPOLATIONS if key == "img2" else (cases.INTER_LINEAR,)):
                got = ca.warp_flow(flows, interpolation=interp, **{key: batch})
                assert got.shape == (3, cases.H, cases.W, batch.shape[-1])
                for i in range(3):
                    one = batch[i, ..., 0] if batch.shape[-1] == 1 else batch[i]
                    single = ca.warp_flow(flows[i], interpolation=interp, **{key: one})
                    _same(got[i].reshape(single.shape), single, (key, interp, i))
                    _same(single, flow_ref.warp_flow(flows[i], interpolation=interp, **{key: one}), (key, interp, i, "ref"))


# (w, h): one pixel, one row, one column, less than one block, a block tail of one lane, two blocks and a lane
SHAPES = [(1, 1), (300, 1), (1, 300), (70, 37), (257, 5), (513, 3)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_against_the_restatement(oracle, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    for cn in (1, 3):
        img = cases.image(w + h + cn, (h, w), cn=cn)
        for dtype in (np.float32, np.float64):
            ax, ay = min(3.0, w / 2), min(3.0, h / 2)  # pixels: some targets inside even on a one-pixel side
            flow = np.stack([rng.uniform(-ax, ax, (h, w)) / w, rng.uniform(-ay, ay, (h, w)) / h]).astype(dtype)
            flow[:, rng.random((h, w)) < 0.1] = 0
            for interp in INTERPOLATIONS:
                _same(ca.warp_flow(flow, img2=img, interpolation=interp), flow_ref.warp_flow(flow, img2=img, interpolation=interp),
                      ("backward", cn, dtype.__name__, interp))
            _same(ca.warp_flow(flow, img1=img), flow_ref.warp_flow(flow, img1=img), ("forward", cn, dtype.__name__))


def _unfused_differs_from_fused(w):
    """A float64 flow row (x components) for an image of width ``w`` in which, for as many pixels as can be found,
    x + fx * w evaluated as NumPy does (product rounded, then sum rounded) lands exactly on t + 0.5 with t even, while
    the fused evaluation (one rounding of the exact x + fx * w) lands above it: half-to-even sends the first to t, the
    second rounds to t + 1.  The product cancels most of x, so that its rounding error is visible in the small sum."""
    fx, found = np.zeros(w), []
    for x in range(w // 2, w):
        p0 = (x % 7) * 2 + 0.5 - x                 # the product that puts the sum on t + 0.5, t even
        for f in (p0 / w, np.nextafter(p0 / w, 0.0), np.nextafter(p0 / w, -1.0)):
            exact = Fraction(float(f)) * w
            if f * w == p0 and exact > Fraction(p0) and float(Fraction(x) + exact) > x + f * w:
                fx[x] = f
                found.append(x)
                break
    return fx, found


def test_float64_positions_are_not_fused(oracle):
    w, h = 513, 3
    fx, found = _unfused_differs_from_fused(w)
    assert len(found) >= 10, "no pixel tells fused from unfused evaluation"
    flow = np.zeros((2, h, w))
    flow[0, :] = fx
    flow[1, :] = 1.0 / h  # (every pixel takes part; one row down)
    # the fixture has teeth: rounding the fused positions sends those pixels somewhere else
    unfused = np.rint(flow_ref.positions(flow)[0, 0, found])
    fused = np.array([np.rint(float(Fraction(x) + Fraction(fx[x]) * w)) for x in found])
    assert (unfused != fused).all()
    img = cases.image(40, (h, w), cn=1)
    want = flow_ref.warp_flow(flow, img1=img)
    fused_flow = flow.copy()
    fused_flow[0, :, found] += 1e-12  # what a fused evaluation amounts to: off the tie
    assert not np.array_equal(flow_ref.warp_flow(fused_flow, img1=img), want)
    _same(ca.warp_flow(flow, img1=img), want, "forward")
    for interp in INTERPOLATIONS:
        _same(ca.warp_flow(flow, img2=img, interpolation=interp), flow_ref.warp_flow(flow, img2=img, interpolation=interp),
              ("backward", interp))


def test_non_finite_flow(oracle):
    bad = [(3, 4, 0, np.nan), (5, 6, 1, np.inf), (7, 8, 0, -np.inf), (9, 10, 1, np.nan), (11, 12, 0, 1e30), (13, 14, 1, -3e8)]
    for dtype in (np.float32, np.float64):
        flow = cases.smooth_flow(dtype)
        for y, x, c, v in bad:
            flow[c, y, x] = v
        flow[:, 20, 20] = np.nan
        for cn in (1, 3):
            img = cases.image(50 + cn, cn=cn)
            for interp in INTERPOLATIONS:
                got = ca.warp_flow(flow, img2=img, interpolation=interp)
                for y, x, _, _ in bad + [(20, 20, 0, 0)]:
                    assert (got[y, x] == 0).all(), (dtype.__name__, cn, interp, y, x)
                _same(got, flow_ref.warp_flow(flow, img2=img, interpolation=interp), ("backward", dtype.__name__, cn, interp))
            # forward: such a source is skipped -- the picture is the one of a flow that is zero there
            skipped = flow.copy()
            for y, x, _, _ in bad + [(20, 20, 0, 0)]:
                skipped[:, y, x] = 0
            got = ca.warp_flow(flow, img1=img)
            _same(got, ca.warp_flow(skipped, img1=img), ("forward", dtype.__name__, cn))
            _same(got, flow_ref.warp_flow(flow, img1=img), ("forward ref", dtype.__name__, cn))


def test_forward_collisions_are_deterministic(oracle):
    flow, img1 = cases.forward_inputs()["f_contract"]
    f, s = _cuda(flow), _cuda(img1)
    first = ca.warp_flow(f, img1=s).cpu().numpy()
    second = ca.warp_flow(f, img1=s).cpu().numpy()
    assert first.tobytes() == second.tobytes()


def test_c_abi_pitched_buffers(oracle):
    """Both entry points straight through the ABI: row pitches and image strides larger than the packed sizes, a batch
    of two with a flow each; the padding stays untouched."""
    from calibrating_amd import _native
    lib = _native.lib()
    nb, cn, (h, w), (sh, sw) = 2, 3, (cases.H, cases.W), cases.BIG
    flows = np.stack([cases.smooth_flow(np.float64, seed=s) for s in range(nb)])
    fstride = 2 * h * w + 24                                              # float64 elements
    F = torch.zeros(nb * fstride, dtype=torch.float64, device="cuda")
    for i in range(nb):
        F[i * fstride:i * fstride + 2 * h * w] = _cuda(flows[i].reshape(-1))
    dpitch, dstride = w * cn + 13, (h + 1) * (w * cn + 13) + 5
    ws = torch.empty(nb * h * w, dtype=torch.int32, device="cuda")
    for forward, (ih, iw) in ((False, (h, w)), (True, (sh, sw))):
        imgs = [cases.image(60 + i, (ih, iw), cn=cn) for i in range(nb)]
        pitch, istride = iw * cn + 29, (ih + 2) * (iw * cn + 29) + 64    # bytes
        S = torch.zeros(nb * istride, dtype=torch.uint8, device="cuda")
        for i, img in enumerate(imgs):
            S[i * istride:i * istride + ih * pitch].view(ih, pitch)[:, :iw * cn] = _cuda(img.reshape(ih, iw * cn))
        out = torch.full((nb * dstride,), 201, dtype=torch.uint8, device="cuda")
        if forward:
            rc = lib.camd_warp_flow_forward_u8(S.data_ptr(), iw, ih, cn, pitch, istride, F.data_ptr(), _native.VALUE_F64, fstride,
                                               out.data_ptr(), w, h, dpitch, dstride, cases.INTER_LINEAR, ws.data_ptr(), nb,
                                               _native.current_stream())
        else:
            rc = lib.camd_warp_flow_backward_u8(S.data_ptr(), cn, pitch, istride, F.data_ptr(), _native.VALUE_F64, fstride,
                                                out.data_ptr(), w, h, dpitch, dstride, cases.INTER_LINEAR, nb,
                                                _native.current_stream())
        _native.check(rc)
        res = out.cpu().numpy()
        for i, img in enumerate(imgs):
            got = res[i * dstride:i * dstride + h * dpitch].reshape(h, dpitch)
            want = flow_ref.warp_flow(flows[i], **{"img1" if forward else "img2": img})
            assert np.array_equal(got[:, :w * cn].reshape(h, w, cn), want), (forward, i)
            assert (got[:, w * cn:] == 201).all()                         # padding untouched
