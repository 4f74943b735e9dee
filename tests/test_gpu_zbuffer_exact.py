"""Every entry point of the point-cloud and z-buffer family (csrc/pointcloud.hip) against the exact C oracle
(oracle/pointcloud_ref.c), bit for bit: no share, no tolerance (-m gpu).  The oracle is plain serial loops that state
the arithmetic the kernels document -- dot products as the chain fma(a2,b2, fma(a1,b1, a0*b0)), rint, "the smaller zs
wins, the later index wins a bit-equal tie" -- and tests/test_pointcloud_oracle_cpu.py holds it to NumPy and to the
reference's recorded runs.  The shapes are the smallest that reach the edges: 256-thread blocks (n, grid widths),
several blocks per grid row, rows of 5 columns, every payload type, ties by the thousand on one pixel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import _native, pointcloud  # noqa: E402

import pointcloud_exact_cases as exact  # noqa: E402
import reproject_cases as cases  # noqa: E402
from test_gpu_compaction_edges import K, SHAPES, _masks  # noqa: E402


def _same(got, want, what=""):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, \
        (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        diff = (got != want) & ~((got != got) & (want != want))
        raise AssertionError("%s: %d of %d values differ from the oracle, first at %s" % (
            what, diff.sum(), diff.size, tuple(np.argwhere(diff)[0]) if diff.any() else "a sign of zero / NaN payload"))


# ---- depth_to_point_cloud ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [1, 1.5, 0.75])
@pytest.mark.parametrize("h,w", SHAPES)
def test_depth_to_point_cloud(oracle, h, w, rate):
    z = 1.0 + np.random.default_rng(w * 13 + h).random((h, w))
    for name, mask in _masks(h, w).items():
        depth = np.where(mask, z, 0.0)
        _same(pointcloud.depth_to_point_cloud(depth, K, interpolation_rate=rate, return_xyzuv=True),
              oracle.depth_to_point_cloud(depth, K, rate, return_xyzuv=True), name)
    _same(pointcloud.depth_to_point_cloud(depth, K, interpolation_rate=rate), oracle.depth_to_point_cloud(depth, K, rate))


def test_depth_to_point_cloud_uint16_is_millimetres(oracle):
    mm = np.uint16(np.random.default_rng(16).integers(0, 4000, (7, 300)))
    for rate in (1, 1.5):
        _same(pointcloud.depth_to_point_cloud(mm, K, interpolation_rate=rate, return_xyzuv=True),
              oracle.depth_to_point_cloud(mm, K, rate, return_xyzuv=True))


# ---- apply_T_to_point_cloud, point_cloud_to_depth, point_cloud_to_arr2d -------------------------------------------
SMALL_XY = (64, 48)
SMALL_K = np.array([[60.0, 0, 31.7], [0, 61.0, 23.4], [0, 0, 1]])
# the left 3x3 of a projection matrix: a third row that is not (0, 0, 1), so zs is not the point's own Z
SKEW_K = np.array([[60.0, 0.3, 31.7], [-0.2, 61.0, 23.4], [0.01, -0.02, 0.98]])


def _pose():
    T = np.eye(4)
    T[:3, :3] = ca.geometry.rodrigues(np.array([0.02, -0.05, 0.01]))
    T[:3, 3] = [0.06, -0.01, 0.02]
    return T


def _seeded_cloud(n, cols):
    """n points in front of SMALL_K's 64 x 48 image, about one in ten beside it.  z takes one of 4 values, and a
    third of the points sit exactly on a pixel centre of SMALL_K's: several of those share pixel and z bit for bit."""
    rng = np.random.default_rng(n * 8 + cols)
    z = 1.0 + rng.integers(0, 4, n) / 8.0
    px, py = rng.uniform(-3, 67, n), rng.uniform(-3, 51, n)
    snap = rng.random(n) < 1 / 3
    px[snap], py[snap] = np.round(px[snap]), np.round(py[snap])
    cloud = np.stack([(px - 31.7) / 60.0 * z, (py - 23.4) / 61.0 * z, z], 1)
    if cols > 3:
        cloud = np.concatenate([cloud, rng.standard_normal((n, cols - 3))], 1)
    return cloud


def _payloads(n):
    rng = np.random.default_rng(n)
    for channels in (1, 3):
        yield rng.standard_normal((n, channels)), -2.5
        yield np.float32(rng.standard_normal((n, channels))), -2.5
        yield rng.integers(0, 256, (n, channels)).astype(np.uint8), 7


@pytest.mark.parametrize("cols", [3, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025, 20000])
def test_point_arrays(oracle, n, cols):
    cloud, T = _seeded_cloud(n, cols), _pose()
    moved = pointcloud.apply_T_to_point_cloud(T, cloud)
    _same(moved, oracle.apply_T_to_point_cloud(T, cloud), "apply_T")
    assert moved.shape == (n, cols) and moved[:, 3:].tobytes() == cloud[:, 3:].tobytes()
    index = np.arange(n, dtype=np.float64)          # as a payload: the image of owners
    for pts in (cloud, moved):
        for Km in (SMALL_K, SKEW_K):
            _same(pointcloud.point_cloud_to_depth(pts, Km, SMALL_XY, bg_value=-1),
                  oracle.point_cloud_to_depth(pts, Km, SMALL_XY, bg_value=-1), "depth")
            _same(pointcloud.point_cloud_to_arr2d(pts, Km, SMALL_XY, values=index, bg_value=-1),
                  oracle.point_cloud_to_arr2d(pts, Km, SMALL_XY, values=index, bg_value=-1), "owner")
    for values, bg in _payloads(n):
        _same(pointcloud.point_cloud_to_arr2d(moved, SKEW_K, SMALL_XY, values=values, bg_value=bg),
              oracle.point_cloud_to_arr2d(moved, SKEW_K, SMALL_XY, values=values, bg_value=bg),
              "%s x%d" % (values.dtype, values.shape[1]))
    if n == 20000:      # what the large cloud is for: most pixels receive several points, many of them bit-equal ties
        owner = oracle.zbuffer_points(cloud, SMALL_K, SMALL_XY)[0]
        backwards = oracle.zbuffer_points(cloud[::-1], SMALL_K, SMALL_XY)[0]
        hit = owner >= 0
        assert hit.mean() > 0.95
        assert (owner[hit] != n - 1 - backwards[hit]).mean() > 0.2     # the winner of the reversed cloud is another row


def test_half_to_even_and_the_image_edges(oracle):
    pts = exact.half_points()
    index = np.arange(len(pts), dtype=np.float64)
    got = pointcloud.point_cloud_to_arr2d(pts, exact.HALF_K, exact.XY, values=index, bg_value=-1)
    want = np.full((exact.XY[1], exact.XY[0]), -1.0)
    for i, (_, _, pixel) in enumerate(exact.HALF_CASES):
        if pixel is not None:
            want[pixel[1], pixel[0]] = i
    _same(got, want, "owners by construction")
    _same(got, oracle.point_cloud_to_arr2d(pts, exact.HALF_K, exact.XY, values=index, bg_value=-1))
    _same(pointcloud.point_cloud_to_depth(pts, exact.HALF_K, exact.XY), np.where(want >= 0, 1.0, 0.0))


def test_negative_z_wins_and_z_ordering(oracle):
    x, y = exact.CENTRE_PIXEL
    zs_all = exact.Z_ASCENDING
    for first in range(len(zs_all)):
        tail = zs_all[first:]
        for order in (tail, tail[::-1], tail[1:] + tail[:1]):
            pts = exact.centre_points(order)
            depth = pointcloud.point_cloud_to_depth(pts, exact.CENTRE_K, exact.XY, bg_value=9)
            assert depth[y, x].tobytes() == np.float64(tail[0]).tobytes() and (depth != 9).sum() == 1, (first, order)
            _same(depth, oracle.point_cloud_to_depth(pts, exact.CENTRE_K, exact.XY, bg_value=9))
            index = np.arange(len(pts), dtype=np.float32)
            owner = pointcloud.point_cloud_to_arr2d(pts, exact.CENTRE_K, exact.XY, values=index, bg_value=-1)
            assert owner[y, x] == order.index(tail[0]) and (owner >= 0).sum() == 1, (first, order)
    ties = exact.centre_points([2.0, 1.0, 1.0, 3.0, 1.0, 2.0])
    assert pointcloud.point_cloud_to_arr2d(ties, exact.CENTRE_K, exact.XY, values=np.arange(6.0))[y, x] == 4


def test_dropped_points(oracle):
    pts = np.concatenate([exact.DROPPED, exact.KEPT_AMONG_DROPPED[None], exact.DROPPED])
    x, y = exact.KEPT_PIXEL
    depth = pointcloud.point_cloud_to_depth(pts, exact.CENTRE_K, exact.XY, bg_value=-7)
    assert (depth == -7).sum() == depth.size - 1 and depth[y, x] == 2.0
    _same(depth, oracle.point_cloud_to_depth(pts, exact.CENTRE_K, exact.XY, bg_value=-7))
    index = np.arange(len(pts), dtype=np.float64)
    owner = pointcloud.point_cloud_to_arr2d(pts, exact.CENTRE_K, exact.XY, values=index, bg_value=-1)
    assert (owner >= 0).sum() == 1 and owner[y, x] == len(exact.DROPPED)
    # the same through the depth image: huge and negative entries, then non-finite ones too (which the z-buffers drop;
    # depth_to_point_cloud would hand them on as NaN rows, whose payload bits are nobody's contract)
    d2 = cases.depth2().copy()
    d2[5, 8], d2[7, 7] = 1e300, -1.25
    for rate in (1, 1.5):
        _same(pointcloud.depth_to_point_cloud(d2, cases.K2, interpolation_rate=rate),
              oracle.depth_to_point_cloud(d2, cases.K2, rate))
    d2[5, 5:8] = [np.nan, np.inf, -np.inf]
    for rate in (1, 1.5):
        _same(pointcloud.project_depth(d2, cases.K2, cases.pose(), cases.K1, cases.XY1, interpolation_rate=rate),
              oracle.project_depth(d2, cases.K2, cases.pose(), cases.K1, cases.XY1, rate))
        _same(pointcloud.get_reproject_remap(cases.K1, cases.K2, cases.pose(), d2, cases.XY1, interpolation_rate=rate),
              oracle.get_reproject_remap(cases.K1, cases.K2, cases.pose(), d2, cases.XY1, rate))


@pytest.mark.parametrize("spread", [False, True])
def test_contention(oracle, spread):
    """65 536 points on one pixel (or on 4 x 4) with 16 distinct z: the atomics of a whole launch meet on a handful of
    addresses, and the winner is the last of some thousands of bit-equal candidates."""
    cloud = exact.contention_cloud(spread)
    Km, xy = (exact.SPREAD_K, exact.SPREAD_XY) if spread else (exact.CENTRE_K, exact.XY)
    n = len(cloud)
    index = np.arange(n, dtype=np.float64)
    colours = np.random.default_rng(4).integers(0, 256, (n, 3)).astype(np.uint8)
    for _ in range(2):      # twice: the same bits whoever the hardware serves first
        _same(pointcloud.point_cloud_to_depth(cloud, Km, xy, bg_value=-1), oracle.point_cloud_to_depth(cloud, Km, xy, bg_value=-1))
        _same(pointcloud.point_cloud_to_arr2d(cloud, Km, xy, values=index, bg_value=-1),
              oracle.point_cloud_to_arr2d(cloud, Km, xy, values=index, bg_value=-1), "owner")
        _same(pointcloud.point_cloud_to_arr2d(cloud, Km, xy, values=colours, bg_value=7),
              oracle.point_cloud_to_arr2d(cloud, Km, xy, values=colours, bg_value=7), "payload")


# ---- project_depth, get_reproject_remap ---------------------------------------------------------------------------
def _both(oracle, d2, K2, T, K1, xy1, rate, what):
    _same(pointcloud.project_depth(d2, K2, T, K1, xy1, interpolation_rate=rate),
          oracle.project_depth(d2, K2, T, K1, xy1, rate), "project_depth " + what)
    _same(pointcloud.get_reproject_remap(K1, K2, T, d2, xy1, interpolation_rate=rate),
          oracle.get_reproject_remap(K1, K2, T, d2, xy1, rate), "get_reproject_remap " + what)


@pytest.mark.parametrize("rate", [1, 1.5])
@pytest.mark.parametrize("h2,w2", [(3, 255), (3, 256), (3, 257), (3, 513), (5, 257), (257, 5)])
def test_grid_widths(oracle, h2, w2, rate):
    """The grid is ceil(gw / 256) x gh blocks: widths around one and two blocks, and a tall one.  The target has half
    the focal length, so that several cells land on every pixel."""
    d2 = cases.scene_depth(w2 * 7 + h2, h2, w2)
    K2 = np.array([[400.0, 0, w2 / 2 - 0.3], [0, 400.0, h2 / 2 + 0.2], [0, 0, 1]])
    xy1 = (w2 // 2 + 4, h2 // 2 + 3)
    K1 = np.array([[206.0, 0, xy1[0] / 2 + 0.4], [0, 202.0, xy1[1] / 2 - 0.1], [0, 0, 1]])
    _both(oracle, d2, K2, cases.pose(), K1, xy1, rate, "%dx%d" % (w2, h2))
    hit = oracle.zbuffer_grid(d2, K2, cases.pose(), K1, xy1, rate)[0] >= 0
    assert len(oracle.depth_to_point_cloud(d2, K2, rate)) > 2 * hit.sum() > 0


@pytest.mark.parametrize("rate", [1, 1.5, 0.75, cases.RATE_NATIVE])
def test_rotated_rig(oracle, rate):
    d2 = cases.depth2()
    _both(oracle, d2, cases.K2, cases.pose(), cases.K1, cases.XY1, rate, "rate %s" % rate)
    _both(oracle, np.uint16(np.round(d2 * 1000)), cases.K2, cases.pose(), cases.K1, cases.XY1, rate, "uint16, rate %s" % rate)


def test_replicated_cell_ties(oracle):
    """R = I at rate 1.5: more than 10 000 cells share pixel and z bit for bit with another; the later cell wins."""
    _both(oracle, cases.depth2(), cases.K2, cases.pose(rotated=False), cases.K1, cases.XY1, 1.5, "R = I")


def test_cam_entry_points(oracle):
    cam1 = ca.Cam.init_by_K_D(cases.K1, None, cases.XY1)
    cam2 = ca.Cam.init_by_K_D(cases.K2, None, cases.XY2)
    d2, T = cases.depth2(), cases.pose()
    for interpolation, rate in ((1.5, cases.RATE_NATIVE), (1, 420 / 380), (0, 1)):
        _same(cam1.project_cam2_depth(cam2, d2, T=T, interpolation=interpolation),
              oracle.project_depth(d2, cases.K2, T, cases.K1, cases.XY1, rate), "interpolation %s" % interpolation)


def test_batch_with_padded_strides(oracle):
    """camd_reproject_remap through the raw ABI as in test_gpu_reproject.py::test_c_abi_with_strides_and_guards: three
    images whose depth and map planes are not packed, each one equal to the oracle."""
    lib = _native.lib()
    T, rate, nb = cases.pose(), 1.5, 3
    (w2, h2), (w1, h1) = cases.XY2, cases.XY1
    depths = [cases.depth2(seed) for seed in (3, 4, 6)]
    dstride, mstride = w2 * h2 + 13, 2 * w1 * h1 + 7
    dbuf = torch.full((nb * dstride,), float("nan"), dtype=torch.float64, device="cuda")
    for i, d in enumerate(depths):
        dbuf[i * dstride:i * dstride + w2 * h2] = torch.from_numpy(d.reshape(-1)).cuda()
    mbuf = torch.full((nb * mstride,), 12345.0, dtype=torch.float32, device="cuda")
    keys = torch.empty((nb * w1 * h1,), dtype=torch.int64, device="cuda")
    owner = torch.empty((nb * w1 * h1,), dtype=torch.int32, device="cuda")
    K2inv = np.ascontiguousarray(np.linalg.inv(cases.K2)).reshape(9)
    Tm, K1m = np.ascontiguousarray(T).reshape(16), np.ascontiguousarray(cases.K1).reshape(9)
    _native.check(lib.camd_reproject_remap(dbuf.data_ptr(), w2, h2, dstride, K2inv.ctypes.data, Tm.ctypes.data,
                                           K1m.ctypes.data, rate, w1, h1, mbuf.data_ptr(), mbuf.data_ptr() + 4 * w1 * h1,
                                           mstride, keys.data_ptr(), owner.data_ptr(), nb, _native.current_stream()))
    m, o = mbuf.cpu().numpy(), owner.cpu().numpy().reshape(nb, h1, w1)
    gw, _ = oracle.point_cloud_grid(w2, h2, rate)
    for i, d in enumerate(depths):
        _same(m[i * mstride:i * mstride + 2 * w1 * h1].reshape(2, h1, w1),
              oracle.get_reproject_remap(cases.K1, cases.K2, T, d, cases.XY1, rate), "image %d" % i)
        assert (m[i * mstride + 2 * w1 * h1:(i + 1) * mstride] == 12345).all()
        # the owner workspace: 1 + the row-major grid cell, 0 where nobody
        assert np.array_equal(o[i].astype(np.int64) - 1, oracle.zbuffer_grid(d, cases.K2, T, cases.K1, cases.XY1, rate)[0])
    assert gw == 450


def test_full_size_1080p(oracle):
    xy = (1920, 1080)
    K1 = np.array([[1400.0, 0, 961.3], [0, 1404.0, 538.9], [0, 0, 1]])
    K2 = np.array([[1350.0, 0, 950.0], [0, 1350.0, 545.0], [0, 0, 1]])
    rate = 1400.0 / 1350.0 * 1.5
    d2 = cases.scene_depth(11, xy[1], xy[0])
    _both(oracle, d2, K2, cases.pose(), K1, xy, rate, "1080p")
