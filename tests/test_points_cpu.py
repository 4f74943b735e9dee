"""The NumPy restatement of cv2.undistortPoints / cv2.projectPoints (tests/points_ref.py) is sane, so that bit equality
with it on the GPU (tests/test_gpu_points.py) means something; plus what ``Cam.undistort_points`` / ``Cam.project_points``
refuse before any device is touched.  No GPU."""
import ctypes

import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import _native, imgproc

import distort_depth_ref as dref
import points_cases as pc
import points_ref as ref


def test_without_distortion_it_is_the_distort_depth_restatement():
    for pts in (pc.grid_pixels(7, np.float32), pc.pixels(5000, 1, np.float32), pc.special_pixels(np.float32)):
        got = ref.undistort_points(pts, pc.K, None)
        want = dref.undistort_points(pts, pc.K, None)
        assert got.dtype == np.float32 and got.shape == (len(pts), 2)
        assert got.tobytes() == want.reshape(-1, 2).tobytes()
        # iters plays no part without a lens, and (n, 1, 2) is (n, 2)
        assert ref.undistort_points(pts[:, None], pc.K, None, iters=40).tobytes() == got.tobytes()


@pytest.mark.parametrize("ndist", pc.NDIST)
def test_zero_pose_and_unit_depth_is_the_distort_depth_restatement(ndist):
    D = pc.lens(ndist)
    und = dref.undistort_points(pc.grid_pixels(5, np.float32), pc.K, None)
    xyz = dref.convert_points_to_homogeneous(und)
    want = dref.project_points(xyz, np.zeros(3), np.zeros(3), pc.K, D)[0].reshape(-1, 2)
    got = ref.project_points(xyz, np.eye(3), np.zeros(3), pc.K, D)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    if ndist == 14:  # zero tilt is the 12-coefficient model
        assert got.tobytes() == ref.project_points(xyz, np.eye(3), np.zeros(3), pc.K, pc.lens(12)).tobytes()


def test_project_undoes_undistort_and_iters_matters():
    """project(undistort(p)) = p over every pixel of a 640 x 480 image under a mild lens.  The bound is the restatement's
    own: cv2's fixed-point iteration contracts by about 3 |k1| r^2 < 0.3 per round here, so 40 rounds leave only float64
    rounding (a few ulp of a pixel coordinate of some hundreds: 1e-13 .. 1e-12 px, asserted < 1e-9 px) and cv2's 5 rounds
    visibly more."""
    p = pc.grid_pixels(1)
    res = {}
    for iters in (5, 40):
        n = ref.undistort_points(p, pc.K, pc.MILD, iters=iters)
        back = ref.project_points(np.concatenate([n, np.ones((len(n), 1))], 1), np.eye(3), np.zeros(3), pc.K, pc.MILD)
        res[iters] = float(np.abs(back - p).max())
    print("round-trip residual in px: iters=5 %.3e, iters=40 %.3e" % (res[5], res[40]))
    assert res[40] < 1e-9
    assert res[5] > res[40]
    # the Cam form goes back to pixels of the undistorted camera: without a lens it returns its input
    same = ref.cam_undistort_points(p, pc.K, None)
    assert same.dtype == np.float64 and np.abs(same - p).max() < 1e-10
    assert ref.cam_undistort_points(p.astype(np.float32), pc.K, pc.MILD).dtype == np.float64


def test_the_negative_icdist_exit_is_taken_by_some_points_only():
    p = pc.grid_pixels(4)
    n, took = ref.undistort_trace(p, pc.K, pc.STRONG, iters=5)
    start = ref.undistort_trace(p, pc.K, None)[0]
    assert took.any() and not took.all()
    corner = (p == 0).all(1)
    centre = (np.abs(p - [320, 240]) < 2).all(1)
    assert took[corner].all() and not took[centre].any()
    assert n[took].tobytes() == start[took].tobytes()   # a point that takes the exit keeps its start value
    assert (n[~took] != start[~took]).any(1).mean() > 0.99
    # some meet it in the first round, some only after the iteration has carried them outwards
    first = ref.undistort_trace(p, pc.K, pc.STRONG, iters=1)[1]
    assert first.any() and (took & ~first).any()


def test_refusals_need_no_device():
    cam = ca.Cam(pc.K, pc.lens(5), (pc.W, pc.H))
    uv, xyz = pc.pixels(10, 2, np.float64), pc.points3d(10, 3, np.float64)
    for bad in (uv.astype(np.int32), uv.astype(np.float16), uv.astype(np.int64), uv > 0):
        with pytest.raises(ValueError, match="float32 or float64"):
            cam.undistort_points(bad)
    with pytest.raises(ValueError, match="float32 or float64"):
        cam.project_points(xyz.astype(np.int32))
    for bad in (uv[:, :1], uv.reshape(-1), uv.reshape(5, 2, 2), xyz):
        with pytest.raises(ValueError, match=r"\(n, 2\)"):
            cam.undistort_points(bad)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        cam.project_points(uv)
    with pytest.raises(TypeError):
        cam.undistort_points(uv.tolist())
    import torch
    with pytest.raises(ValueError, match="live on the GPU"):
        cam.undistort_points(torch.from_numpy(uv))
    with pytest.raises(ValueError, match="live on the GPU"):
        cam.project_points(torch.from_numpy(xyz))
    for iters in (0, 101, -1, 2.5):
        with pytest.raises(ValueError, match="iters"):
            cam.undistort_points(uv, iters=iters)
    tilted = ca.Cam(pc.K, pc.TILTED, (pc.W, pc.H))
    with pytest.raises(ValueError, match="tilted"):
        tilted.undistort_points(uv)
    with pytest.raises(ValueError, match="tilted"):
        tilted.project_points(xyz)
    for nd in (1, 3, 6, 13):
        with pytest.raises(ValueError, match="coefficients"):
            imgproc.undistort_points(uv, pc.K, np.zeros(nd))
        with pytest.raises(ValueError, match="coefficients"):
            imgproc.project_points(xyz, np.zeros(3), np.zeros(3), pc.K, np.zeros(nd))
    with pytest.raises(ValueError):
        imgproc.project_points(xyz, np.zeros(4), np.zeros(3), pc.K)
    with pytest.raises(ValueError):
        imgproc.project_points(xyz, np.eye(3), np.zeros(2), pc.K)
    if not torch.cuda.is_available():  # good arguments get as far as the device, and no further: there is no CPU fallback
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cam.undistort_points(uv)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cam.project_points(xyz)


def test_the_abi_checks_its_arguments_before_the_device():
    lib = _native.lib()
    Kc = np.ascontiguousarray(pc.K).reshape(9)
    D = np.ascontiguousarray(pc.lens(5))
    R, t = np.eye(3).reshape(9), np.zeros(3)
    buf = np.zeros(64)  # host memory: none of these calls gets as far as a launch
    F64, F32 = _native.VALUE_F64, _native.VALUE_F32

    def und(uv=buf.ctypes.data, ty=F64, n=4, stride=2, K=Kc.ctypes.data, dist=D.ctypes.data, nd=5, iters=5,
            out=buf.ctypes.data + 256, oty=F64):
        return lib.camd_undistort_points(uv, ty, n, stride, K, dist, nd, iters, out, oty, None)

    def proj(xyz=buf.ctypes.data, ty=F64, n=4, stride=3, R=R.ctypes.data, t=t.ctypes.data, K=Kc.ctypes.data,
             dist=D.ctypes.data, nd=5, out=buf.ctypes.data + 256):
        return lib.camd_project_points(xyz, ty, n, stride, R, t, K, dist, nd, out, None)

    assert und(n=0) == _native.CAMD_OK and proj(n=0) == _native.CAMD_OK           # a valid no-op, device or not
    assert und(n=0, uv=None, out=None) == _native.CAMD_OK
    bad_und = [dict(uv=None), dict(out=None), dict(K=None), dict(dist=None), dict(stride=1), dict(stride=0), dict(stride=-2),
               dict(iters=0), dict(iters=101), dict(ty=2), dict(ty=7), dict(oty=2), dict(nd=3), dict(nd=15), dict(nd=-1),
               dict(n=2 ** 31), dict(uv=buf.ctypes.data + 4), dict(out=buf.ctypes.data + 264),
               dict(ty=F32, uv=buf.ctypes.data + 2)]
    for kw in bad_und:
        assert und(**kw) == _native.CAMD_ERR_BAD_ARG, kw
        assert "camd_undistort_points" in _native.last_error(), kw
    bad_proj = [dict(xyz=None), dict(out=None), dict(R=None), dict(t=None), dict(K=None), dict(stride=2), dict(ty=2),
                dict(nd=6), dict(n=2 ** 31), dict(xyz=buf.ctypes.data + 4), dict(out=buf.ctypes.data + 264)]
    for kw in bad_proj:
        assert proj(**kw) == _native.CAMD_ERR_BAD_ARG, kw
        assert "camd_project_points" in _native.last_error(), kw
    tilt = (ctypes.c_double * 14)(*pc.TILTED)
    assert und(dist=tilt, nd=14) == _native.CAMD_ERR_UNSUPPORTED and "tilted" in _native.last_error()
    assert proj(dist=tilt, nd=14) == _native.CAMD_ERR_UNSUPPORTED and "tilted" in _native.last_error()
