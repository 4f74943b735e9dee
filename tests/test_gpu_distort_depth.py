"""``Stereo.distort_depth`` and ``get_depth(return_distort_depth=True)`` on the MI355X (-m gpu).  Everything is compared
bit for bit: the source-index table and the gather against the NumPy restatement (tests/distort_depth_ref.py) and
against what the reference's own Python produced (tests/golden/reference_distort_depth.npz)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import _native, imgproc, synthetic  # noqa: E402

import distort_depth_cases as dc  # noqa: E402
import distort_depth_ref as ref  # noqa: E402
import reference_cases as rc  # noqa: E402  (tests/golden, put on the path by distort_depth_cases)


@pytest.fixture(scope="module")
def fx():
    f = dc.load_fixture()
    assert f is not None, "tests/golden/reference_distort_depth.npz is missing"
    return f


def _stereo(name="barrel", matcher=False):
    st = ca.Stereo.load(dc.rig_record(name))
    if matcher:
        st.set_stereo_matching(ca.SemiGlobalBlockMatching(dict(dc.GET_DEPTH["cfg"])), **dc.GET_DEPTH["setm"])
    return st


@pytest.mark.parametrize("name", dc.GOOD_RIGS)
def test_index_table_of_the_golden_rigs(fx, name):
    K, D, (w, h) = dc.camera(name)
    idx = imgproc.distort_index_map(K, D, (w, h))
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (h, w) and idx.is_cuda
    got = idx.cpu().numpy()
    assert np.array_equal(got, ref.index_map_unique(K, D, w, h))
    assert np.array_equal(got, fx[name + "/src_index"])


@pytest.mark.parametrize("wh", [(1280, 720), (1920, 1080)])
def test_index_table_at_full_size(wh):
    rec = synthetic.rig(*wh)
    K, D = np.array(rec["cam1"]["K"]), rec["cam1"]["D"]
    got = imgproc.distort_index_map(K, D, wh).cpu().numpy()
    want = ref.index_map_unique(K, D, *wh)
    assert np.array_equal(got, want), "%d entries differ" % (got != want).sum()
    assert 0.03 < (want < 0).mean() < 0.12  # a barrel rig leaves holes: the table is not a permutation


@pytest.mark.parametrize("name", dc.GOOD_RIGS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_distort_depth_against_golden_and_restatement(fx, name, dtype):
    st = _stereo(name)
    K, D, (w, h) = dc.camera(name)
    z = dc.depth_input(name, dtype)
    want = fx["%s/distort_depth_%s" % (name, np.dtype(dtype).name)]
    assert np.array_equal(ref.distort_depth(z, K, D, (w, h)), want)
    got = st.distort_depth(z)                                  # ndarray in -> ndarray out
    assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == (h, w)
    assert np.array_equal(got, want)
    t = st.distort_depth(torch.from_numpy(z).cuda())           # tensor in -> tensor out
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.from_numpy(z).dtype
    assert np.array_equal(t.cpu().numpy(), want)
    # batched: (n, h, w), every image its own content (at this size one image per workgroup: the shared-index loop over
    # several images is test_gather_shares_the_index_between_images_of_a_batch's)
    zs = np.stack([np.roll(z, 7 * i, axis=1) * dtype(1 + i) for i in range(5)])
    table = fx[name + "/src_index"]
    for batch in (zs, torch.from_numpy(zs).cuda()):
        gb = st.distort_depth(batch)
        assert type(gb) is type(batch) and tuple(gb.shape) == zs.shape
        gb = gb if isinstance(gb, np.ndarray) else gb.cpu().numpy()
        assert gb.dtype == dtype and np.array_equal(gb, ref.gather(zs, table))
        assert np.array_equal(gb[0], want)
    assert st.distort_depth(zs[:1]).shape == (1, h, w)


@pytest.mark.parametrize("wh,dtype,batch", [
    ((1920, 1080), np.float64, 35),   # 16-byte stores, 16 images per workgroup, a tail group of 3
    ((1920, 1080), np.float64, 3),    # groups of 2, a tail group of 1
    ((1920, 1080), np.float32, 35),
    ((1920, 1080), np.float32, 5),    # (four pixels per lane: half the workgroups) groups of 2, a tail group of 1
    ((1919, 1081), np.float64, 19),   # odd w * h: one pixel per lane, 16 images per workgroup, a tail group of 3
    ((1919, 1081), np.float32, 18),   # odd w * h, a tail group of 2
])
def test_gather_shares_the_index_between_images_of_a_batch(wh, dtype, batch):
    """The hot path at the size it is quoted for: camd_distort_depth lets a workgroup serve up to 16 images of a batch from
    one index load once the grid fills the chip (>= 4096 workgroups), which only full-size images reach.  Every image
    has its own content; all of them against the restatement's gather through the restatement's table."""
    w, h = wh
    rec = synthetic.rig(w, h)
    K, D = np.array(rec["cam1"]["K"]), rec["cam1"]["D"]
    # (the group size the launcher arrives at, restated: the test is about groups of several images with a tail)
    vec = 16 // np.dtype(dtype).itemsize
    lanes = w * h // vec if (w * h) % vec == 0 else w * h
    zb = min(batch, 16)
    while zb > 1 and -(-lanes // 256) * -(-batch // zb) < 4096:
        zb = (zb + 1) // 2
    assert zb > 1 and batch % zb != 0
    table = ref.index_map_unique(K, D, w, h)
    idx = imgproc.distort_index_map(K, D, (w, h))
    assert np.array_equal(idx.cpu().numpy(), table)
    rng = np.random.default_rng(batch * 1000 + w)
    z = rng.integers(1, 1 << 20, (batch, h, w)).astype(dtype) / dtype(1024)
    z[:, ::7, ::5] = 0
    got = imgproc.distort_depth(torch.from_numpy(z).cuda(), idx).cpu().numpy()
    want = ref.gather(z, table)
    assert got.dtype == want.dtype and got.shape == want.shape
    for i in range(batch):
        assert np.array_equal(got[i], want[i]), "image %d of %d (groups of %d)" % (i, batch, zb)
    assert len({got[i].tobytes() for i in range(batch)}) == batch


def test_wrong_shapes_are_refused():
    st = _stereo()
    w, h = st.cam1.xy
    for bad in (np.zeros((h + 1, w)), torch.zeros((w, h), dtype=torch.float64, device="cuda"), np.zeros((h, w, 3))):
        with pytest.raises(ValueError):
            st.distort_depth(bad)
    with pytest.raises(ValueError):
        st.distort_depth(torch.zeros((h, w), dtype=torch.float16, device="cuda"))


def test_the_table_is_built_once():
    st = _stereo()
    z = torch.from_numpy(dc.depth_input("barrel", np.float64)).cuda()
    st.distort_depth(z)
    keys = [k for k in st._dev if k.startswith("distort:")]
    assert len(keys) == 1
    table = st._dev[keys[0]]
    st.distort_depth(z)
    st.distort_depth(z.cpu().numpy())
    assert st._dev[keys[0]] is table and st._distort_table(z.device) is table
    assert st._distort_table("cuda") is table  # one spelling per device
    assert [k for k in st._dev if k.startswith("distort:")] == keys


def test_get_depth_with_return_distort_depth(fx):
    st = _stereo(matcher=True)
    img1, img2 = dc.scene_images()
    assert str(fx["get_depth/img1_sha"]) == rc.sha(img1) and str(fx["get_depth/img2_sha"]) == rc.sha(img2)
    plain = st.get_depth(img1, img2)
    assert sorted(plain) == sorted(ca.Stereo.RESULT_KEYS)
    res = st.get_depth(img1, img2, return_distort_depth=True)
    assert sorted(res) == sorted(ca.Stereo.RESULT_KEYS + ca.Stereo.DISTORT_KEYS)
    assert sorted(res) == sorted(str(k) for k in fx["get_depth/result_keys"])
    assert res["distort_img1"] is img1
    for k in ca.Stereo.RESULT_KEYS:
        assert np.array_equal(res[k], plain[k]), k
    K, D, (w, h) = dc.camera("barrel")
    assert res["distort_depth"].dtype == np.float64 and res["distort_depth"].shape == (h, w)
    assert np.array_equal(res["distort_depth"], ref.distort_depth(res["unrectify_depth"], K, D, (w, h)))
    assert np.array_equal(res["distort_depth"], fx["get_depth/distort_depth"])  # what the reference's own run returned
    # as in the reference the flag implies the unrectify branch
    res2 = st.get_depth(img1, img2, return_unrectify_depth=False, return_distort_depth=True)
    assert sorted(res2) == sorted(res) and np.array_equal(res2["distort_depth"], res["distort_depth"])
    # device tensors in -> device tensors out, the argument itself handed back
    t1, t2 = torch.from_numpy(img1).cuda(), torch.from_numpy(img2).cuda()
    rt = st.get_depth(t1, t2, return_distort_depth=True)
    assert rt["distort_img1"] is t1 and rt["distort_depth"].is_cuda
    assert np.array_equal(rt["distort_depth"].cpu().numpy(), res["distort_depth"])


def test_keys_async_and_batch(fx):
    st = _stereo(matcher=True)
    img1, img2 = dc.scene_images()
    want = fx["get_depth/distort_depth"]
    only = st.get_depth(img1, img2, keys=("distort_depth",))
    assert list(only) == ["distort_depth"] and isinstance(only["distort_depth"], np.ndarray)
    assert np.array_equal(only["distort_depth"], want)
    both = st.get_depth(img1, img2, keys=("distort_img1", "disparity"))
    assert sorted(both) == ["disparity", "distort_img1"] and both["distort_img1"] is img1
    with pytest.raises(ValueError):
        st.get_depth(img1, img2, keys=("distort",))
    # async: several calls in flight, collected out of order
    full = st.get_depth(img1, img2, return_distort_depth=True)
    pend = [st.get_depth_async(img1, img2, return_distort_depth=True), st.get_depth_async(img1, img2, keys="distort_depth"),
            st.get_depth_async(img1, img2)]
    assert sorted(pend[2].result()) == sorted(ca.Stereo.RESULT_KEYS)
    assert list(pend[1].result()) == ["distort_depth"] and np.array_equal(pend[1].result()["distort_depth"], want)
    got = pend[0].result()
    assert sorted(got) == sorted(full) and got["distort_img1"] is img1
    assert all(np.array_equal(got[k], full[k]) for k in full)
    # batch: pair i is the single call's result, bit for bit
    pairs = [(img1, img2), synthetic.render_plane_pair(dc.rig_record("barrel"), (-0.1, 0.2, 1.0), 1.7, seed=5)[:2],
             (img2, img1)]
    singles = [st.get_depth(a, b, return_distort_depth=True) for a, b in pairs]
    s1, s2 = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    many = st.get_depth_batch(s1, s2, return_distort_depth=True)
    assert sorted(many) == sorted(ca.Stereo.RESULT_KEYS + ca.Stereo.DISTORT_KEYS) and many["distort_img1"] is s1
    for i, one in enumerate(singles):
        for k in ca.Stereo.RESULT_KEYS + ("distort_depth",):
            assert np.array_equal(many[k][i], one[k]), (i, k)
    assert len({s["distort_depth"].tobytes() for s in singles}) == 3
    assert sorted(st.get_depth_batch(s1, s2)) == sorted(ca.Stereo.RESULT_KEYS)
    g1 = st.get_depth_batch(s1, s2, keys=("distort_depth",))
    assert list(g1) == ["distort_depth"] and g1["distort_depth"].shape == (3,) + want.shape
    assert all(np.array_equal(g1["distort_depth"][i], singles[i]["distort_depth"]) for i in range(3))


def test_a_rig_whose_targets_leave_the_image_is_refused(fx):
    """An ordinary error path: out-of-range targets are counted by the kernel and never written; the host reads the
    counters once and raises.  A good rig afterwards works as if nothing had happened."""
    assert str(fx[dc.OUT_RIG + "/raised"]).startswith("IndexError")  # the reference cannot serve this rig either
    K, D, (w, h) = dc.camera(dc.OUT_RIG)
    want = ref.target_stats(K, D, w, h)
    st = _stereo(dc.OUT_RIG, matcher=True)
    with pytest.raises(IndexError) as e:
        st.distort_depth(dc.depth_input(dc.OUT_RIG, np.float64))
    msg = str(e.value)
    assert "%d of %d pixels" % (want["n_out"], w * h) in msg
    assert "U in [%d, %d], V in [%d, %d]" % (want["minU"], want["maxU"], want["minV"], want["maxV"]) in msg
    assert not any(k.startswith("distort:") for k in st._dev)  # nothing half-built is kept
    img1, img2 = dc.scene_images()
    with pytest.raises(IndexError):
        st.get_depth(img1, img2, return_distort_depth=True)
    assert sorted(st.get_depth(img1, img2)) == sorted(ca.Stereo.RESULT_KEYS)  # the rest of the rig works
    good = _stereo("barrel")
    z = dc.depth_input("barrel", np.float64)
    assert np.array_equal(good.distort_depth(z), fx["barrel/distort_depth_float64"])
    torch.cuda.synchronize()


def test_c_abi_batched_with_guards(fx):
    """camd_distort_index_map / camd_distort_depth straight through the ABI: batch > 1, odd w * h (no 16-byte stores
    possible past image 0), float64 and float32, guard words around every output buffer untouched."""
    lib = _native.lib()
    K, D, (w, h) = dc.camera("rational12")
    for (w, h) in ((w, h), (199, 151)):
        n, nb = w * h, 5
        Kc = np.ascontiguousarray(K, np.float64).reshape(9)
        Dc = np.ascontiguousarray(D, np.float64)
        guard = 64
        ibuf = torch.full((n + 2 * guard,), 12345, dtype=torch.int32, device="cuda")
        stats = torch.full((6 + 2 * guard,), 777, dtype=torch.int32, device="cuda")
        _native.check(lib.camd_distort_index_map(Kc.ctypes.data, Dc.ctypes.data, Dc.size, w, h,
                                                 ibuf[guard:].data_ptr(), stats[guard:].data_ptr(), _native.current_stream()))
        ih, sh = ibuf.cpu().numpy(), stats.cpu().numpy()
        assert (ih[:guard] == 12345).all() and (ih[-guard:] == 12345).all()
        assert (sh[:guard] == 777).all() and (sh[-guard:] == 777).all()
        ts = ref.target_stats(Kc.reshape(3, 3), D, w, h)
        assert list(sh[guard:guard + 6]) == [0, ts["minU"], ts["maxU"], ts["minV"], ts["maxV"], 0]
        table = ih[guard:-guard].reshape(h, w)
        assert np.array_equal(table, ref.index_map_unique(Kc.reshape(3, 3), D, w, h))
        for dtype in (np.float64, np.float32):
            rng = np.random.default_rng(n)
            z = rng.standard_normal((nb, h, w)).astype(dtype)
            z[rng.random(z.shape) < 0.1] = -0.0
            zin = torch.from_numpy(z).cuda()
            out = torch.full((nb * n + 2 * guard,), -7.0, dtype=zin.dtype, device="cuda")
            _native.check(lib.camd_distort_depth(zin.data_ptr(), z.itemsize, w, h, ibuf[guard:].data_ptr(),
                                                 out[guard:].data_ptr(), nb, _native.current_stream()))
            o = out.cpu().numpy()
            assert (o[:guard] == -7).all() and (o[-guard:] == -7).all()
            want = ref.gather(z, table)
            assert o[guard:-guard].tobytes() == want.tobytes(), (w, h, dtype)
    # bad arguments come back as a status, not as a launch
    buf = torch.zeros(16, dtype=torch.float64, device="cuda")
    i4 = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert lib.camd_distort_depth(buf.data_ptr(), 2, 4, 4, i4.data_ptr(), buf.data_ptr(), 1, None) == _native.CAMD_ERR_BAD_ARG
    assert lib.camd_distort_depth(buf.data_ptr(), 8, 4, 4, i4.data_ptr(), buf.data_ptr(), 1, None) == _native.CAMD_ERR_BAD_ARG
    tilt, eye = (ctypes.c_double * 14)(*([0.0] * 12 + [0.01, 0.0])), np.eye(3)
    assert lib.camd_distort_index_map(eye.ctypes.data, tilt, 14, 4, 4, i4.data_ptr(), i4.data_ptr(),
                                      None) == _native.CAMD_ERR_UNSUPPORTED
    # a foreign table with indices outside [0, n): nothing is read, zeros come back
    wild = torch.tensor([-5, 16, 2 ** 31 - 1, 3] * 4, dtype=torch.int32, device="cuda")
    src = torch.arange(1, 17, dtype=torch.float64, device="cuda")
    dst = torch.empty(16, dtype=torch.float64, device="cuda")
    _native.check(lib.camd_distort_depth(src.data_ptr(), 8, 4, 4, wild.data_ptr(), dst.data_ptr(), 1, None))
    assert dst.cpu().tolist() == [0.0, 0.0, 0.0, 4.0] * 4


def test_fuzz_slice():
    rep = dc.fuzz_on_gpu()
    assert not rep["mismatches"], rep["mismatches"][:5]
    assert rep["refused"] <= dc.FUZZ_MAX_REFUSED * rep["cases"]
