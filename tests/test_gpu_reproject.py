"""Registering a second camera's image to camera 1 through depth on the MI355X (-m gpu): ``get_reproject_remap``,
``point_cloud_to_arr2d`` with values, ``reproject_img`` / ``Cam.reproject_img`` against the NumPy restatement
(tests/reproject_ref.py) and against what the reference's own Python produced (tests/golden/reference_reproject.npz).

Every map is compared bit for bit, on every pixel, with the exact C oracle (oracle/pointcloud_ref.c) and with the
reference's recorded run -- fixed data that tests/test_pointcloud_oracle_cpu.py shows to equal that oracle.  Only the
comparisons with the NumPy restatement keep a share, ``cases.CAP`` = 0.9999 of the pixels: its matrix products are
NumPy's BLAS, whose rounding belongs to the machine the test runs on, not to the library."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import _native, pointcloud  # noqa: E402

import reproject_cases as cases  # noqa: E402
import reproject_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    f = cases.load_fixture()
    assert f is not None, "tests/golden/reference_reproject.npz is missing"
    return f


def _share(got, want, what):
    """Share of pixels whose map entries (both planes) are bit-equal, and of pixels with the same hit / miss."""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert (got[got < 0] == -1).all() and np.array_equal(got[0] < 0, got[1] < 0)   # the background is -1 in both planes
    same = (got.view(np.int32) == want.view(np.int32)).all(0).mean()
    mask = ((got[0] >= 0) == (want[0] >= 0)).mean()
    print("%s: %.6f of the pixels bit-equal, %.6f same hit mask (%d hit)" % (what, same, mask, (got[0] >= 0).sum()))
    return same, mask


@pytest.mark.parametrize("rate", cases.GPU_RATES)
def test_get_reproject_remap_rotated_rig(fx, rate, oracle):
    d2, T = cases.depth2(), cases.pose()
    got = pointcloud.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, interpolation_rate=rate)
    assert isinstance(got, np.ndarray) and got.shape == (2, 240, 320) and got.dtype == np.float32
    want = ref.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, rate)   # the reference's literal sort
    same, mask = _share(got, want, "rate %s vs restatement" % rate)
    assert same >= cases.CAP and mask >= cases.CAP
    assert got.tobytes() == oracle.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, rate).tobytes()
    if rate in cases.GOLDEN_RATES:
        assert got.tobytes() == fx["remap_rate%s" % rate].tobytes()      # the reference's run, every pixel
    # uint16 depth is millimetres
    mm = np.uint16(np.round(d2 * 1000))
    got_mm = pointcloud.get_reproject_remap(cases.K1, cases.K2, T, mm, cases.XY1, interpolation_rate=rate)
    same, mask = _share(got_mm, ref.get_reproject_remap(cases.K1, cases.K2, T, mm, cases.XY1, rate), "rate %s, uint16" % rate)
    assert same >= cases.CAP and mask >= cases.CAP
    assert got_mm.tobytes() == oracle.get_reproject_remap(cases.K1, cases.K2, T, mm, cases.XY1, rate).tobytes()


def test_tie_rule_larger_index_wins(oracle):
    """R = I at rate 1.5: replicated cells share z bit for bit; the library's winner is the stable sort's."""
    d2, T = cases.depth2(), cases.pose(rotated=False)
    got = pointcloud.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, interpolation_rate=1.5)
    stable = ref.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, 1.5, kind="stable")
    same, mask = _share(got, stable, "R = I, rate 1.5 vs stable sort")
    assert same >= cases.CAP and mask >= cases.CAP
    assert got.tobytes() == oracle.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, 1.5).tobytes()
    default = ref.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, 1.5)
    assert (got != default).any(0).sum() > 1000   # and that is a decision: the literal sort picks others


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.uint8])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_point_cloud_to_arr2d_values(dtype, channels, oracle):
    cloud, _ = cases.coloured_cloud()
    rng = np.random.default_rng(channels * 10 + np.dtype(dtype).itemsize)
    if dtype == np.uint8:
        values, bg = rng.integers(0, 256, (len(cloud), channels)).astype(np.uint8), 7
    else:
        values, bg = rng.standard_normal((len(cloud), channels)).astype(dtype), -2.5
    want = ref.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=values, bg_value=bg, kind="stable")
    assert np.array_equal(want, ref.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=values, bg_value=bg))  # no ties
    for v in ((values, values[:, 0]) if channels == 1 else (values,)):     # (N, 1) and (N,) both give (h, w)
        got = pointcloud.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=v, bg_value=bg)
        assert isinstance(got, np.ndarray) and got.dtype == dtype
        assert got.shape == ((240, 320) if channels == 1 else (240, 320, channels)) == want.shape
        same = (got == want).reshape(240 * 320, -1).all(1).mean()
        print("arr2d %s x%d: %.6f of the pixels equal" % (np.dtype(dtype).name, channels, same))
        assert same >= cases.CAP
        exact = oracle.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=v, bg_value=bg)
        assert got.dtype == exact.dtype and got.tobytes() == exact.tobytes()


def test_coloured_cloud_against_the_reference_run(fx, oracle):
    cloud, colours = cases.coloured_cloud()
    got = pointcloud.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=colours, bg_value=7)
    want = fx["coloured"]
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes()                               # the reference's run, every pixel
    assert got.tobytes() == oracle.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=colours, bg_value=7).tobytes()
    # values=None is point_cloud_to_depth
    assert np.array_equal(pointcloud.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, bg_value=-3),
                          pointcloud.point_cloud_to_depth(cloud, cases.K1, cases.XY1, bg_value=-3))
    # ... and the z-buffer with a payload picks the points the depth-only z-buffer keeps: payload = z itself
    z_as_payload = pointcloud.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=cloud @ cases.K1[2], bg_value=0)
    assert np.array_equal(z_as_payload, pointcloud.point_cloud_to_depth(cloud, cases.K1, cases.XY1))


def test_point_cloud_to_arr2d_behind_camera_outside_and_empty(oracle):
    K = cases.K1
    pts = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 1.0], [0.0, 0.0, -3.0],      # same pixel: the negative z "wins"
                    [50.0, 0.0, 1.0], [0.1, 0.1, 0.0], [0.2, -0.1, 4.0],    # outside / z = 0 / ordinary
                    [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0]])                # not finite
    vals = np.arange(1, 9, dtype=np.float32) * 1.5
    got = pointcloud.point_cloud_to_arr2d(pts, K, (320, 240), values=vals, bg_value=-1)
    keep = [0, 1, 2, 3, 5]                                                   # z = 0 divides by zero in NumPy
    want = ref.point_cloud_to_arr2d(pts[keep], K, (320, 240), values=vals[keep], bg_value=-1, kind="stable")
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert got.tobytes() == oracle.point_cloud_to_arr2d(pts, K, (320, 240), values=vals, bg_value=-1).tobytes()   # all 8
    assert (got != -1).sum() == 2 and got[119, 161] == vals[2]
    empty = pointcloud.point_cloud_to_arr2d(np.zeros((0, 3)), K, (8, 6), values=np.zeros((0, 3), np.uint8), bg_value=9)
    assert empty.shape == (6, 8, 3) and empty.dtype == np.uint8 and (empty == 9).all()
    # two points with the same z on one pixel: the later row wins
    twins = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 2.0], [0.0, 0.0, 2.0]])
    assert pointcloud.point_cloud_to_arr2d(twins, K, (320, 240), values=np.array([5.0, 6.0, 4.0]))[119, 161] == 4.0


@pytest.mark.parametrize("cn", [1, 3])
def test_reproject_img(fx, cn, oracle):
    d2, T = cases.depth2(), cases.pose()
    img = cases.image(1 if cn == 1 else 2, cn=cn)
    key = "gray" if cn == 1 else "rgb"
    for rate in cases.GOLDEN_RATES:
        maps = pointcloud.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, interpolation_rate=rate)
        got = pointcloud.reproject_img(img, d2, cases.K2, T, cases.K1, cases.XY1, interpolation_rate=rate)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (240, 320) + img.shape[2:]
        assert np.array_equal(got, ref.reproject_img(img, maps[0], maps[1]))      # cv2.remap(INTER_LINEAR) on its own map
        assert maps.tobytes() == fx["remap_rate%s" % rate].tobytes()
        assert got.tobytes() == fx["%s_rate%s" % (key, rate)].tobytes()          # the reference's picture, every pixel
        assert got[maps[0] < 0].max(initial=0) == 0 and got.max() > 100
    # Cam.reproject_img: the rate of get_appropriate_interpolation_rate
    cam1 = ca.Cam.init_by_K_D(cases.K1, None, cases.XY1)
    cam2 = ca.Cam.init_by_K_D(cases.K2, None, cases.XY2)
    via_cam = cam1.reproject_img(cam2, d2, img, T=T, interpolation=1.5)
    maps = pointcloud.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, interpolation_rate=cases.RATE_NATIVE)
    assert np.array_equal(via_cam, ref.reproject_img(img, maps[0], maps[1]))
    plain = cam1.reproject_img(cam2, d2, img, T=T, interpolation=0)               # interpolation off: rate 1
    assert np.array_equal(plain, pointcloud.reproject_img(img, d2, cases.K2, T, cases.K1, cases.XY1))


def test_batch_of_five_equals_five_single_calls_and_torch_stays_on_the_device():
    T = cases.pose()
    depths = np.stack([cases.depth2(seed) * (1 + 0.05 * seed) for seed in range(5)])
    grays = np.stack([cases.image(seed, cn=1) for seed in range(5)])
    rgbs = np.stack([cases.image(seed, cn=3) for seed in range(5)])
    for rate in (1, 1.5):
        args = (cases.K1, cases.K2, T)
        singles = [pointcloud.get_reproject_remap(*args, d, cases.XY1, interpolation_rate=rate) for d in depths]
        many = pointcloud.get_reproject_remap(*args, depths, cases.XY1, interpolation_rate=rate)
        assert many.shape == (5, 2, 240, 320) and many.dtype == np.float32
        for i in range(5):
            assert many[i].tobytes() == singles[i].tobytes(), i
        assert len({m.tobytes() for m in many}) == 5
        assert pointcloud.get_reproject_remap(*args, depths[:1], cases.XY1, interpolation_rate=rate).shape == (1, 2, 240, 320)
        for imgs in (grays, rgbs):
            one = [pointcloud.reproject_img(imgs[i], depths[i], cases.K2, T, cases.K1, cases.XY1, rate) for i in range(5)]
            stack = pointcloud.reproject_img(imgs, depths, cases.K2, T, cases.K1, cases.XY1, rate)
            assert stack.shape == (5, 240, 320) + imgs.shape[3:]
            assert all(np.array_equal(stack[i], one[i]) for i in range(5))
        # torch in -> torch out, on the same device
        dt = torch.from_numpy(depths).cuda()
        mt = pointcloud.get_reproject_remap(*args, dt, cases.XY1, interpolation_rate=rate)
        assert isinstance(mt, torch.Tensor) and mt.device == dt.device and mt.dtype == torch.float32
        assert mt.cpu().numpy().tobytes() == many.tobytes()
        it = pointcloud.reproject_img(torch.from_numpy(rgbs).cuda(), dt, cases.K2, T, cases.K1, cases.XY1, rate)
        assert isinstance(it, torch.Tensor) and it.device == dt.device and it.dtype == torch.uint8
        assert np.array_equal(it.cpu().numpy(), pointcloud.reproject_img(rgbs, depths, cases.K2, T, cases.K1, cases.XY1, rate))
    cloud, colours = cases.coloured_cloud()
    ct = pointcloud.point_cloud_to_arr2d(torch.from_numpy(cloud).cuda(), cases.K1, cases.XY1,
                                         values=torch.from_numpy(colours).cuda(), bg_value=7)
    assert isinstance(ct, torch.Tensor) and ct.is_cuda and ct.dtype == torch.uint8
    assert np.array_equal(ct.cpu().numpy(), pointcloud.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=colours, bg_value=7))


def test_c_abi_with_strides_and_guards():
    """camd_reproject_remap straight through the ABI: a batch of 3 whose depth images and map planes are NOT packed
    (strides larger than an image), guard words around every buffer the call writes."""
    lib = _native.lib()
    T, rate, nb, guard = cases.pose(), 1.5, 3, 64
    (w2, h2), (w1, h1) = cases.XY2, cases.XY1
    depths = [cases.depth2(seed) for seed in (3, 4, 6)]
    dstride, mstride = w2 * h2 + 13, 2 * w1 * h1 + 7
    dbuf = torch.full((nb * dstride,), float("nan"), dtype=torch.float64, device="cuda")
    for i, d in enumerate(depths):
        dbuf[i * dstride:i * dstride + w2 * h2] = torch.from_numpy(d.reshape(-1)).cuda()
    mbuf = torch.full((nb * mstride + 2 * guard,), 12345.0, dtype=torch.float32, device="cuda")
    keys = torch.full((nb * w1 * h1 + 2 * guard,), 77, dtype=torch.int64, device="cuda")
    owner = torch.full((nb * w1 * h1 + 2 * guard,), 77, dtype=torch.int32, device="cuda")
    K2inv = np.ascontiguousarray(np.linalg.inv(cases.K2)).reshape(9)
    Tm, K1m = np.ascontiguousarray(T).reshape(16), np.ascontiguousarray(cases.K1).reshape(9)
    mx = mbuf[guard:].data_ptr()
    _native.check(lib.camd_reproject_remap(dbuf.data_ptr(), w2, h2, dstride, K2inv.ctypes.data, Tm.ctypes.data,
                                           K1m.ctypes.data, rate, w1, h1, mx, mx + 4 * w1 * h1, mstride,
                                           keys[guard:].data_ptr(), owner[guard:].data_ptr(), nb, _native.current_stream()))
    m, k, o = mbuf.cpu().numpy(), keys.cpu().numpy(), owner.cpu().numpy()
    assert (m[:guard] == 12345).all() and (m[-guard:] == 12345).all()
    assert (k[:guard] == 77).all() and (k[-guard:] == 77).all() and (o[:guard] == 77).all() and (o[-guard:] == 77).all()
    body = m[guard:-guard]
    for i, d in enumerate(depths):
        got = body[i * mstride:i * mstride + 2 * w1 * h1].reshape(2, h1, w1)
        want = pointcloud.get_reproject_remap(cases.K1, cases.K2, T, d, cases.XY1, interpolation_rate=rate)
        assert got.tobytes() == want.tobytes(), i
        assert (body[i * mstride + 2 * w1 * h1:(i + 1) * mstride] == 12345).all()   # the gap between two images
    # the owner workspace holds 1 + the row-major cell of the sampling grid, 0 where nothing landed
    gw, gh = int(round(w2 * rate)), int(round(h2 * rate))
    own = o[guard:guard + w1 * h1].reshape(h1, w1).astype(np.int64)
    first = body[:2 * w1 * h1].reshape(2, h1, w1)
    assert np.array_equal(own == 0, first[0] < 0) and own.max() <= gw * gh
    hit = own > 0
    assert np.array_equal(np.float32(((own - 1) % gw)[hit] / rate), first[0][hit])
    assert np.array_equal(np.float32(((own - 1) // gw)[hit] / rate), first[1][hit])
    # bad arguments come back as a status, not as a launch
    bad = lib.camd_reproject_remap(dbuf.data_ptr(), w2, h2, w2 * h2 - 1, K2inv.ctypes.data, Tm.ctypes.data, K1m.ctypes.data,
                                   rate, w1, h1, mx, mx, mstride, keys.data_ptr(), owner.data_ptr(), 2, None)
    assert bad == _native.CAMD_ERR_BAD_ARG
    bad = lib.camd_reproject_remap(dbuf.data_ptr(), 70000, 65000, 0, K2inv.ctypes.data, Tm.ctypes.data, K1m.ctypes.data,
                                   1.0, w1, h1, mx, mx, mstride, keys.data_ptr(), owner.data_ptr(), 1, None)
    assert bad == _native.CAMD_ERR_BAD_ARG and "owner index" in _native.last_error()   # 4.55e9 cells >= 2^32 - 1
    pts = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    for kw in (dict(channels=0), dict(vtype=3), dict(vtype=_native.VALUE_U8, bg=-1.0), dict(n=2 ** 32 - 1)):
        rc = lib.camd_point_cloud_to_arr2d(pts.data_ptr(), kw.get("n", 4), 3, K1m.ctypes.data, 8, 6, pts.data_ptr(),
                                           kw.get("channels", 1), kw.get("vtype", 0), kw.get("bg", 0.0), mbuf.data_ptr(),
                                           keys.data_ptr(), owner.data_ptr(), None)
        assert rc == _native.CAMD_ERR_BAD_ARG, kw


def test_identical_calls_give_identical_bits():
    """What the owner pass is for: whoever the hardware serves first, the winner is the same."""
    for rotated, rate in ((False, 1.5), (True, 1.5), (True, 1)):
        d2, T = cases.depth2(), cases.pose(rotated)
        a = pointcloud.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, interpolation_rate=rate)
        for _ in range(3):
            b = pointcloud.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, interpolation_rate=rate)
            assert a.tobytes() == b.tobytes()
    cloud, colours = cases.coloured_cloud()
    twice = np.concatenate([cloud, cloud])                    # every point has a twin with the same z on the same pixel
    tw_col = np.concatenate([colours, 255 - colours])
    a = pointcloud.point_cloud_to_arr2d(twice, cases.K1, cases.XY1, values=tw_col)
    assert a.tobytes() == pointcloud.point_cloud_to_arr2d(twice, cases.K1, cases.XY1, values=tw_col).tobytes()
    assert np.array_equal(a, pointcloud.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=255 - colours))


def test_full_size_1080p(oracle):
    xy = (1920, 1080)
    K1 = np.array([[1400.0, 0, 961.3], [0, 1404.0, 538.9], [0, 0, 1]])
    K2 = np.array([[1350.0, 0, 950.0], [0, 1350.0, 545.0], [0, 0, 1]])
    cam1, cam2 = ca.Cam.init_by_K_D(K1, None, xy), ca.Cam.init_by_K_D(K2, None, xy)
    rate = pointcloud.get_appropriate_interpolation_rate(cam1, cam2, 1.5)
    assert rate == 1400.0 / 1350.0 * 1.5
    d2, T = cases.scene_depth(11, xy[1], xy[0]), cases.pose()
    got = pointcloud.get_reproject_remap(K1, K2, T, d2, xy, interpolation_rate=rate)
    want = ref.get_reproject_remap(K1, K2, T, d2, xy, rate, kind="stable")
    same, mask = _share(got, want, "1920x1080 -> 1920x1080, rate %.4f" % rate)
    assert same >= cases.CAP and mask >= cases.CAP
    assert got.tobytes() == oracle.get_reproject_remap(K1, K2, T, d2, xy, rate).tobytes()
    assert (got[0] >= 0).mean() > 0.8
