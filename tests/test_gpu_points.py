"""``Cam.undistort_points`` / ``Cam.project_points`` and the kernels under them on the MI355X (-m gpu).  Every result is
compared bit for bit (``np.array_equal(..., equal_nan=True)``) with the NumPy restatement tests/points_ref.py, whose
sanity tests/test_points_cpu.py establishes: float64 arithmetic in one stated order under -ffp-contract=off leaves no
room for a tolerance."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import _native, geometry, imgproc  # noqa: E402

import distort_depth_ref as dref  # noqa: E402
import epipolar_cases as ec  # noqa: E402
import points_cases as pc  # noqa: E402
import points_ref as ref  # noqa: E402

DTYPES = (np.float32, np.float64)
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
EYE, ZERO = np.eye(3), np.zeros(3)


def same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def layouts(rows, width, strides):
    """``rows`` (n, width) as CUDA views whose rows are read in place -> [(name, view, row stride)]: one per row stride in
    ``strides`` (the points are the leading columns of wider rows), plus ``wide[1:, 1:1 + width]`` of an (n + 1, 4) array:
    its stride would allow the 8- / 16-byte loads, its start -- 5 elements into the allocation -- is not aligned for them."""
    n = len(rows)
    out = []
    for s in strides:
        wide = np.full((n, s), 7.5, rows.dtype)
        wide[:, :width] = rows
        out.append(("stride %d" % s, torch.from_numpy(wide).cuda()[:, :width], s))
    wide = np.full((n + 1, 4), -3.25, rows.dtype)
    wide[1:, 1:1 + width] = rows
    view = torch.from_numpy(wide).cuda()[1:, 1:1 + width]
    assert n == 0 or view.data_ptr() % (2 * rows.itemsize) != 0
    out.append(("offset slice", view, 4))
    for _, v, s in out:
        assert tuple(v.shape) == (n, width) and (n < 2 or (v.stride(0) == s and v.stride(1) == 1))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_undistort_points_sizes_and_layouts(dtype):
    D = pc.lens(5)
    for n in pc.SIZES:
        uv = pc.pixels(n, 100 + n, dtype)
        want = ref.undistort_points(uv, pc.K, D)
        got = imgproc.undistort_points(uv, pc.K, D)                       # ndarray in -> ndarray out
        assert isinstance(got, np.ndarray) and same(got, want), n
        for name, view, _ in layouts(uv, 2, (2, 3)):
            t = imgproc.undistort_points(view, pc.K, D)                   # tensor in -> tensor out, rows read in place
            assert isinstance(t, torch.Tensor) and t.device == view.device and t.is_contiguous() and same(t, want), (n, name)
        assert same(ca.Cam(pc.K, D, (pc.W, pc.H)).undistort_points(uv), ref.cam_undistort_points(uv, pc.K, D)), n


@pytest.mark.parametrize("dtype", DTYPES)
def test_project_points_sizes_and_layouts(dtype):
    D = pc.lens(5)
    R = geometry.rodrigues(geometry.T_to_r_t(pc.POSE)[0])
    t = pc.POSE[:3, 3]
    for n in pc.SIZES:
        xyz = pc.points3d(n, 200 + n, dtype)
        want = ref.project_points(xyz, R, t, pc.K, D)
        got = imgproc.project_points(xyz, R, t, pc.K, D)
        assert isinstance(got, np.ndarray) and same(got, want), n
        # stride 3: contiguous rows; 4: float32 rows arrive as one 16-byte load (the last row element by element);
        # 5: xyzuv rows
        for name, view, _ in layouts(xyz, 3, (3, 4, 5)):
            tt = imgproc.project_points(view, R, t, pc.K, D)
            assert isinstance(tt, torch.Tensor) and tt.device == view.device and same(tt, want), (n, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ndist", pc.NDIST)
def test_every_distortion_model(dtype, ndist):
    D = pc.lens(ndist)
    uv, xyz = pc.pixels(1000, 300 + ndist, dtype), pc.points3d(1000, 400 + ndist, dtype)
    und = imgproc.undistort_points(uv, pc.K, D)
    prj = imgproc.project_points(xyz, ZERO, ZERO, pc.K, D)
    assert same(und, ref.undistort_points(uv, pc.K, D)) and same(prj, ref.project_points(xyz, EYE, ZERO, pc.K, D))
    if ndist == 14:  # zero tilt is accepted and is the 12-coefficient model
        assert same(und, imgproc.undistort_points(uv, pc.K, pc.lens(12)))
        assert same(prj, imgproc.project_points(xyz, ZERO, ZERO, pc.K, pc.lens(12)))
    if ndist == 0:  # no lens: nothing is iterated, whatever iters says
        assert same(imgproc.undistort_points(uv, pc.K, None, iters=40), und)
        assert same(imgproc.undistort_points(uv, pc.K, np.zeros(0)), und)
    else:
        assert not same(und, imgproc.undistort_points(uv, pc.K, None))


@pytest.mark.parametrize("ndist", pc.NDIST)
def test_project_points_rebuilds_the_distort_index_table(ndist):
    """k_project_points and k_distort_index_scatter call one forward model (csrc/camera_model.hpp): the pixels of a 16 x 12
    image, normalised and rounded to float32 as U21 does, projected in float64 with R = I, t = 0 and truncated the way
    distort.hip truncates, give ``distort_index_map``'s table -- first index wins, -1 in holes."""
    w, h = 16, 12
    K, D = np.array([[10.3, 0, 7.8], [0, 10.1, 5.7], [0, 0, 1.0]]), pc.lens(ndist)
    assert dref.target_stats(K, D, w, h)["n_out"] == 0  # (CPU: every target of this rig stays inside the image)
    v, u = np.mgrid[0:h, 0:w]
    x = ((u.ravel() - K[0, 2]) * (1.0 / K[0, 0])).astype(np.float32).astype(np.float64)
    y = ((v.ravel() - K[1, 2]) * (1.0 / K[1, 1])).astype(np.float32).astype(np.float64)
    UV = imgproc.project_points(np.stack([x, y, np.ones_like(x)], 1), EYE, ZERO, K, D)
    assert UV.dtype == np.float64
    t = UV.astype(np.float32).astype(np.int32)  # (float) of the float64 pixel, then truncation toward zero
    want = np.full(w * h, w * h, np.int64)
    np.minimum.at(want, t[:, 1] * w + t[:, 0], np.arange(w * h))
    want[want == w * h] = -1
    got = imgproc.distort_index_map(K, D, (w, h)).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got.reshape(-1), want)
    assert (want < 0).any() and (want >= 0).any()  # holes are part of the comparison (without a lens: rounding alone)
    assert np.array_equal(got, dref.index_map_minimum_at(K, D, w, h))


def test_tilted_sensor_is_refused():
    uv, xyz = pc.pixels(10, 1, np.float64), pc.points3d(10, 2, np.float64)
    tu, tx = torch.from_numpy(uv).cuda(), torch.from_numpy(xyz).cuda()
    for a, b in ((uv, xyz), (tu, tx)):
        with pytest.raises(ValueError, match="tilted"):
            imgproc.undistort_points(a, pc.K, pc.TILTED)
        with pytest.raises(ValueError, match="tilted"):
            imgproc.project_points(b, ZERO, ZERO, pc.K, pc.TILTED)
    lib = _native.lib()
    Kc, out = np.ascontiguousarray(pc.K).reshape(9), torch.zeros((10, 2), dtype=torch.float64, device="cuda")
    tilt = (ctypes.c_double * 14)(*pc.TILTED)
    assert lib.camd_undistort_points(tu.data_ptr(), _native.VALUE_F64, 10, 2, Kc.ctypes.data, tilt, 14, 5, out.data_ptr(),
                                     _native.VALUE_F64, None) == _native.CAMD_ERR_UNSUPPORTED
    assert lib.camd_project_points(tx.data_ptr(), _native.VALUE_F64, 10, 3, EYE.ctypes.data, ZERO.ctypes.data, Kc.ctypes.data,
                                   tilt, 14, out.data_ptr(), None) == _native.CAMD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("iters", [1, 5, 40])
def test_iterations_and_the_negative_icdist_exit(dtype, iters):
    p = pc.grid_pixels(4, dtype)
    for D in (pc.MILD, pc.lens(12), pc.STRONG):
        want = ref.undistort_points(p, pc.K, D, iters=iters)
        assert same(imgproc.undistort_points(p, pc.K, D, iters=iters), want), D
        assert same(imgproc.undistort_points(torch.from_numpy(p).cuda(), pc.K, D, iters=iters), want), D
    took = ref.undistort_trace(p, pc.K, pc.STRONG, iters=iters)[1]
    assert took.any() and not took.all()  # (established on the CPU: both sides of the exit are in this grid)
    if iters == 5:
        assert same(imgproc.undistort_points(p, pc.K, pc.STRONG), ref.undistort_points(p, pc.K, pc.STRONG, iters=5))
        assert not same(imgproc.undistort_points(p, pc.K, pc.MILD), ref.undistort_points(p, pc.K, pc.MILD, iters=40))


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_points(dtype):
    uv, xyz = pc.special_pixels(dtype), pc.special_points3d(dtype)
    R = geometry.rodrigues(geometry.T_to_r_t(pc.POSE)[0])
    for D in (None, pc.lens(5), pc.lens(12), pc.STRONG):
        assert same(imgproc.undistort_points(uv, pc.K, D), ref.undistort_points(uv, pc.K, D)), D
        assert same(imgproc.undistort_points(uv, pc.K, D, pixels=True), ref.cam_undistort_points(uv, pc.K, D)), D
        assert same(imgproc.project_points(xyz, ZERO, ZERO, pc.K, D), ref.project_points(xyz, EYE, ZERO, pc.K, D)), D
        assert same(imgproc.project_points(xyz, R, pc.POSE[:3, 3], pc.K, D), ref.project_points(xyz, R, pc.POSE[:3, 3], pc.K, D)), D
    # Z == 0 projects as if Z were 1 (cv2: z = z ? 1 / z : 1), for +0 and -0 alike
    got = imgproc.project_points(xyz, ZERO, ZERO, pc.K, None)
    assert np.isfinite(got[1:4]).all()
    assert np.array_equal(got[1], imgproc.project_points(np.array([[0.3, 0.2, 1.0]], dtype), ZERO, ZERO, pc.K, None)[0])


def test_cam_surface():
    cam = ca.Cam(pc.K, pc.lens(8), (pc.W, pc.H), name="wide")
    D = cam.D
    for dtype in DTYPES:
        uv, xyz = pc.pixels(1500, 500, dtype), pc.points3d(1500, 501, dtype)
        want = ref.cam_undistort_points(uv, pc.K, D)
        assert want.dtype == np.float64
        got = cam.undistort_points(uv)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (1500, 2) and same(got, want)
        assert same(cam.undistort_points(uv[:, None]), want)                              # (n, 1, 2)
        assert same(cam.undistort_points(uv, iters=40), ref.cam_undistort_points(uv, pc.K, D, iters=40))
        t = cam.undistort_points(torch.from_numpy(uv).cuda())
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and same(t, want)
        assert same(cam.undistort_points(torch.from_numpy(uv[:, None]).cuda()), want)
        # project_points: the input's type; T=None is the zero pose, and so is the identity
        want = ref.project_points(xyz, EYE, ZERO, pc.K, D)
        got = cam.project_points(xyz)
        assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == (1500, 2) and same(got, want)
        assert same(cam.project_points(xyz, T=np.eye(4)), want)
        assert same(cam.project_points(xyz[:, None]), want)                               # (n, 1, 3)
        t = cam.project_points(torch.from_numpy(xyz).cuda())
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.from_numpy(xyz).dtype and same(t, want)
        # a pose goes through cv2's two Rodrigues passes on the host
        R = geometry.rodrigues(geometry.T_to_r_t(pc.POSE)[0])
        want = ref.project_points(xyz, R, pc.POSE[:3, 3], pc.K, D)
        assert same(cam.project_points(xyz, pc.POSE), want)
        assert same(cam.project_points(torch.from_numpy(xyz).cuda(), T=pc.POSE), want)
        assert not same(cam.project_points(xyz), want)
    # a camera without a lens record (five zeros) and an empty set
    plain = ca.Cam(pc.K, None, (pc.W, pc.H))
    uv = pc.pixels(300, 502, np.float64)
    assert same(plain.undistort_points(uv), ref.cam_undistort_points(uv, pc.K, np.zeros(5)))
    empty = cam.undistort_points(np.zeros((0, 2), np.float32))
    assert empty.shape == (0, 2) and empty.dtype == np.float64
    assert cam.project_points(torch.zeros((0, 3), dtype=torch.float32, device="cuda")).shape == (0, 2)
    for bad in (uv.astype(np.int32), torch.from_numpy(uv)):
        with pytest.raises(ValueError):
            cam.undistort_points(bad)


def test_runs_on_the_current_stream():
    """A tensor call queues on the caller's stream and hands back a tensor without waiting for it."""
    cam = ca.Cam(pc.K, pc.lens(5), (pc.W, pc.H))
    uv = pc.pixels(65537, 600, np.float32)
    want = ref.cam_undistort_points(uv, pc.K, cam.D)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = torch.from_numpy(uv).cuda()
        got = cam.undistort_points(t)
    side.synchronize()
    assert same(got, want)


def test_raw_matches_to_a_pose():
    """The chain the entry points exist for: matches as a matcher sees them (raw, distorted pixels) -> undistort_points
    -> EssentialMatrixStereo.  The undistorted points equal the restatement's bit for bit, hence so does the rig."""
    case = ec.pose_case(ec.FROM_STEREO_CASE)
    rec = case["record"]
    cams = [ca.Cam().load(dict(rec[k])) for k in ("cam1", "cam2")]
    raw, und, und_ref = [], [], []
    for cam, uvs in zip(cams, (case["uvs1"], case["uvs2"])):
        rays = np.concatenate([(uvs - cam.K[:2, 2]) / [cam.fx, cam.fy], np.ones((len(uvs), 1))], 1)
        r = cam.project_points(rays)                       # the pinhole matches, distorted: what a matcher would report
        assert same(r, ref.project_points(rays, EYE, ZERO, cam.K, cam.D))
        assert np.abs(r - uvs).max() > 1.0                 # the lens moves them by pixels
        u = cam.undistort_points(r)
        want = ref.cam_undistort_points(r, cam.K, cam.D)
        assert same(u, want)
        raw.append(r), und.append(u), und_ref.append(want)
    kw = dict(K1=cams[0].K, K2=cams[1].K, xy1=case["xy1"], xy2=case["xy2"], baseline=0.12)
    a = ca.EssentialMatrixStereo(und[0], und[1], **kw)
    b = ca.EssentialMatrixStereo(und_ref[0], und_ref[1], **kw)
    assert a.candidate == b.candidate
    assert a.R.tobytes() == b.R.tobytes() and a.t.tobytes() == b.t.tobytes()
    for k in ("zs1", "zs2"):
        assert a.epipolar[k].tobytes() == b.epipolar[k].tobytes()
    # and the same on tensors, device to device
    tu = [c.undistort_points(torch.from_numpy(r).cuda()) for c, r in zip(cams, raw)]
    assert same(tu[0], und_ref[0]) and same(tu[1], und_ref[1])
    c = ca.EssentialMatrixStereo(tu[0], tu[1], **kw)
    assert c.R.tobytes() == b.R.tobytes() and c.t.tobytes() == b.t.tobytes()
    assert same(c.epipolar["zs1"], b.epipolar["zs1"]) and same(c.epipolar["zs2"], b.epipolar["zs2"])


def test_c_abi_with_guards():
    """Both entry points straight through the ABI: every type pair, strided rows, guard words around the output untouched,
    n = 0 a no-op, bad arguments a status and a message instead of a launch."""
    lib = _native.lib()
    F = {np.float32: _native.VALUE_F32, np.float64: _native.VALUE_F64}
    Kc, D = np.ascontiguousarray(pc.K).reshape(9), np.ascontiguousarray(pc.lens(12))
    R = np.ascontiguousarray(geometry.rodrigues(geometry.T_to_r_t(pc.POSE)[0])).reshape(9)
    t = np.ascontiguousarray(pc.POSE[:3, 3])
    n, guard, st = 1000, 64, _native.current_stream()
    for dt in DTYPES:
        for stride in (2, 3, 4):
            wide = np.full((n, stride), 1.5, dt)
            wide[:, :2] = pc.pixels(n, 700 + stride, dt)
            src = torch.from_numpy(wide).cuda()
            norm = ref.undistort_points(wide[:, :2], pc.K, D)
            for odt, pixels in ((np.float32, 0), (np.float64, 0), (np.float64, _native.POINTS_PIXELS)):
                out = torch.full((2 * n + 2 * guard,), -7.0, dtype=TORCH[odt], device="cuda")
                _native.check(lib.camd_undistort_points(src.data_ptr(), F[dt], n, stride, Kc.ctypes.data, D.ctypes.data, 12, 5,
                                                        out[guard:].data_ptr(), F[odt] | pixels, st))
                o = out.cpu().numpy()
                assert (o[:guard] == -7).all() and (o[-guard:] == -7).all()
                want = ref.cam_undistort_points(wide[:, :2], pc.K, D) if pixels else norm.astype(odt)
                assert same(o[guard:-guard].reshape(n, 2), want), (dt, stride, odt, pixels)
        for stride in (3, 4, 5, 8):
            wide = np.full((n, stride), 1.5, dt)
            wide[:, :3] = pc.points3d(n, 800 + stride, dt)
            src = torch.from_numpy(wide).cuda()
            out = torch.full((2 * n + 2 * guard,), -7.0, dtype=src.dtype, device="cuda")
            _native.check(lib.camd_project_points(src.data_ptr(), F[dt], n, stride, R.ctypes.data, t.ctypes.data, Kc.ctypes.data,
                                                  D.ctypes.data, 12, out[guard:].data_ptr(), st))
            o = out.cpu().numpy()
            assert (o[:guard] == -7).all() and (o[-guard:] == -7).all()
            assert same(o[guard:-guard].reshape(n, 2), ref.project_points(wide[:, :3], R, t, pc.K, D)), (dt, stride)
    # a float32 buffer of stride 4 that ends with the last point's z: the last row is read element by element
    xyz = pc.points3d(n, 900, np.float32)
    flat = np.full(4 * n + 1, np.nan, np.float32)
    flat[:4 * n].reshape(n, 4)[:, :3] = xyz
    src = torch.from_numpy(flat[:4 * n - 1].copy()).cuda()
    out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    _native.check(lib.camd_project_points(src.data_ptr(), F[np.float32], n, 4, R.ctypes.data, t.ctypes.data, Kc.ctypes.data,
                                          D.ctypes.data, 12, out.data_ptr(), st))
    assert same(out, ref.project_points(xyz, R, t, pc.K, D))

    # n = 0 and the refusals: nothing is launched, the output keeps its fill
    src = torch.from_numpy(pc.pixels(16, 1, np.float64)).cuda()
    pts = torch.from_numpy(pc.points3d(16, 2, np.float64)).cuda()
    out = torch.full((16, 2), -7.0, dtype=torch.float64, device="cuda")
    F64 = _native.VALUE_F64

    def und(uv=src.data_ptr(), ty=F64, n=16, stride=2, iters=5, o=out.data_ptr(), oty=F64):
        return lib.camd_undistort_points(uv, ty, n, stride, Kc.ctypes.data, D.ctypes.data, 12, iters, o, oty, st)

    def proj(p=pts.data_ptr(), ty=F64, n=16, stride=3, o=out.data_ptr()):
        return lib.camd_project_points(p, ty, n, stride, R.ctypes.data, t.ctypes.data, Kc.ctypes.data, D.ctypes.data, 12, o, st)

    assert und(n=0) == _native.CAMD_OK and proj(n=0) == _native.CAMD_OK
    for kw in (dict(uv=None), dict(o=None), dict(stride=1), dict(iters=0), dict(iters=101), dict(ty=2), dict(ty=5), dict(oty=2)):
        assert und(**kw) == _native.CAMD_ERR_BAD_ARG, kw
        assert "camd_undistort_points" in _native.last_error()
    for kw in (dict(p=None), dict(o=None), dict(stride=2), dict(ty=2)):
        assert proj(**kw) == _native.CAMD_ERR_BAD_ARG, kw
        assert "camd_project_points" in _native.last_error()
    torch.cuda.synchronize()
    assert (out == -7).all()
