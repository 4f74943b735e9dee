"""CPU tests of ``Stereo.distort_depth`` (no GPU): the NumPy restatement against what the reference's own Python
produced (tests/golden/reference_distort_depth.npz), its two formulations against each other, the public surface, the
refusals that must come before any device call, and the fuzz generator's refusal share."""
import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import imgproc, synthetic

import distort_depth_cases as dc
import distort_depth_ref as ref


@pytest.fixture(scope="module")
def fx():
    f = dc.load_fixture()
    assert f is not None, "tests/golden/reference_distort_depth.npz is missing (python tests/golden/make_distort_depth_golden.py)"
    return f


@pytest.mark.parametrize("name", dc.GOOD_RIGS)
def test_restatement_reproduces_the_reference_run(fx, name):
    """Pixel order, float32 hand-overs, truncation, first-index-wins, zeros in holes and the dtype, as the reference's
    unmodified code produced them."""
    K, D, (w, h) = dc.camera(name)
    table = fx[name + "/src_index"]
    assert table.dtype == np.int32 and table.shape == (h, w)
    assert np.array_equal(ref.index_map_unique(K, D, w, h), table)
    for dtype in (np.float64, np.float32):
        want = fx["%s/distort_depth_%s" % (name, np.dtype(dtype).name)]
        z = dc.depth_input(name, dtype)
        got = ref.distort_depth(z, K, D, (w, h))
        assert want.dtype == dtype and got.dtype == dtype
        assert np.array_equal(got, want)
        assert np.array_equal(ref.gather(z, table), want)
        assert np.array_equal(ref.gather(np.stack([z, z[::-1, ::-1]]), table)[1], ref.gather(z[::-1, ::-1], table))


def test_zero_distortion_is_not_the_identity_table(fx):
    """The float32 hand-overs move some pixels even with D = 0: nobody may special-case it."""
    _, _, (w, h) = dc.camera("zero")
    assert not np.array_equal(fx["zero/src_index"], np.arange(w * h, dtype=np.int32).reshape(h, w))


@pytest.mark.parametrize("name,wh", [(n, None) for n in dc.GOOD_RIGS] + [("barrel", (1280, 720))])
def test_lowest_index_form_equals_the_unique_form(name, wh):
    K, D, size = dc.camera(name)
    if wh is not None:
        K, size = np.array(synthetic.rig(*wh)["cam1"]["K"]), wh
    assert np.array_equal(ref.index_map_minimum_at(K, D, *size), ref.index_map_unique(K, D, *size))


def test_the_out_of_range_rig_is_one_the_reference_cannot_serve(fx):
    """Targets beyond the far edges: the reference raised IndexError.  The same rig also has negative targets, which the
    reference would wrap around to the far edge; the product refuses both sides."""
    assert str(fx[dc.OUT_RIG + "/raised"]).startswith("IndexError")
    K, D, (w, h) = dc.camera(dc.OUT_RIG)
    st = ref.target_stats(K, D, w, h)
    assert st["n_out"] > 0 and st["n_nonfinite"] == 0 and st["maxU"] >= w and st["minU"] < 0
    with pytest.raises(IndexError):
        ref.index_map_unique(K, D, w, h)


def test_result_keys(fx):
    assert ca.Stereo.RESULT_KEYS == ("rectify_img1", "rectify_img2", "disparity", "rectify_depth", "unrectify_depth",
                                     "undistort_img1")
    assert ca.Stereo.DISTORT_KEYS == ("distort_img1", "distort_depth")
    assert sorted(fx["get_depth/result_keys"]) == sorted(ca.Stereo.RESULT_KEYS + ca.Stereo.DISTORT_KEYS)
    assert bool(fx["get_depth/distort_img1_is_the_argument"])


def test_distort_depth_is_implemented_and_fails_loudly_without_gpu():
    """No NotImplementedError any more; without a device the call fails like every other entry point."""
    import torch
    st = ca.Stereo.load(dc.rig_record("barrel"))
    z = dc.depth_input("barrel", np.float64)
    if torch.cuda.is_available():
        assert st.distort_depth(z).shape == z.shape
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.distort_depth(z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imgproc.distort_index_map(*dc.camera("barrel"))
    st.set_stereo_matching(ca.SemiGlobalBlockMatching({}))
    img1, img2 = dc.scene_images()
    with pytest.raises(RuntimeError):
        st.get_depth(img1, img2, return_distort_depth=True)


def test_bad_input_is_refused_before_any_device_call(monkeypatch):
    from calibrating_amd import _native

    def no_device_call(*a, **k):
        raise AssertionError("a device call was made")

    st = ca.Stereo.load(dc.rig_record("barrel"))
    st.set_stereo_matching(ca.SemiGlobalBlockMatching({}))
    monkeypatch.setattr(_native, "require_device", no_device_call)
    monkeypatch.setattr(_native, "lib", no_device_call)
    w, h = st.cam1.xy
    for bad in (np.zeros((h, w + 1)), np.zeros((w, h)), np.zeros(h * w), np.zeros((2, 2, h, w)), np.zeros((h, w, 1)), None):
        with pytest.raises(ValueError, match="distort_depth"):
            st.distort_depth(bad)
    for bad in (np.zeros((h, w), np.int32), np.zeros((h, w), np.float16), np.zeros((h, w), np.uint8)):
        with pytest.raises(ValueError, match="float64 or float32"):
            st.distort_depth(bad)
    import torch
    with pytest.raises(ValueError, match="GPU"):
        st.distort_depth(torch.zeros((h, w), dtype=torch.float64))
    # tilted-sensor coefficients (D[12:14]), as everywhere else in the library
    rec = dc.rig_record("barrel")
    rec["cam1"]["D"] = [list(dc.RIGS["rational12"]["D"]) + [0.01, 0.0]]
    tilted = ca.Stereo.load(rec)
    with pytest.raises(ValueError, match="tilted"):
        tilted.distort_depth(np.zeros((h, w)))
    with pytest.raises(ValueError, match="tilted"):
        imgproc.distort_index_map(tilted.cam1.K, tilted.cam1.D, (w, h))
    rec["cam1"]["D"] = [list(dc.RIGS["rational12"]["D"]) + [0.0, 0.0]]  # 14 coefficients with a zero tilt are fine
    imgproc.check_distortion(ca.Stereo.load(rec).cam1.D)
    # unknown keys, and the new ones are known
    with pytest.raises(ValueError, match="unknown"):
        st.get_depth(np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.uint8), keys=("distorted_depth",))
    want, unrect, distort = st._asked("get_depth", ("distort_depth",), True, False)
    assert (want("distort_depth"), want("unrectify_depth"), unrect, distort) == (True, False, True, True)
    assert st._asked("get_depth", None, False, True)[1:] == (True, True)
    assert st._asked("get_depth", None, True, False)[1:] == (True, False)
    assert st._asked("get_depth", ("disparity",), True, True)[1:] == (False, False)


def test_a_bundle_rig_does_not_rebuild_the_distort_table():
    import torch
    src = ca.Stereo.load(synthetic.rig(96, 64))
    tabs = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in src.table_bundle().items()}
    st = ca.Stereo.from_bundle(tabs, "cpu")
    with pytest.raises(RuntimeError, match="table bundle"):
        st._distort_table(torch.device("cpu"))
    assert not any(k.startswith("distort:") for k in st._dev)


def test_the_fuzz_slice_is_mostly_servable():
    """The seeds the GPU test runs: odd widths, w * h off the workgroup size, all three coefficient counts -- and at
    most a quarter of them rigs that must be refused, so the GPU test cannot hide behind refusals."""
    refused, nds, dtypes, batches = 0, set(), set(), set()
    for i in range(dc.FUZZ_CASES):
        c = dc.gen_case(dc.FUZZ_SEED, i)
        assert c["w"] % 2 == 1 and (c["w"] * c["h"]) % 256 != 0 and c["D"][0] <= 0
        assert abs(c["K"][0, 2] - c["w"] / 2) > 1e-3 and abs(c["K"][1, 2] - c["h"] / 2) > 1e-3
        nds.add(len(c["D"]))
        if ref.target_stats(c["K"], c["D"], c["w"], c["h"])["n_out"]:
            refused += 1
        else:
            dtypes.add(np.dtype(c["dtype"]).name)
            batches.add(c["batch"])
    assert nds == {5, 8, 12} and dtypes == {"float32", "float64"} and batches >= {1, 2}
    assert refused <= dc.FUZZ_MAX_REFUSED * dc.FUZZ_CASES, "%d of %d refused" % (refused, dc.FUZZ_CASES)
