"""The reference's UNMODIFIED default matcher, ``SemiGlobalBlockMatching({})`` (max_size 1000, D=218, block 11), at the
camera sizes its users run it on (-m gpu): 1920x1080 and 3840x2160, through ``Stereo.get_depth`` and
``get_depth_batch`` against tests/oracle_pipeline.oracle_get_depth.  On the GPU that is rectify x2 -> resize to
1000x562 -> SGBM -> k_disp16_up_to_depth back to full size -> unrectify / undistort.  Only at these sizes do the resize
kernels' x blocks meet outputs of 1000, 1920 and 3840 px, the real ratios 1000/1920 and 1000/3840, and the target
height ``round(562.5) == 562`` together.  Every entry is compared bit for bit (depths: first within 1e-4 m with the
same invalid set, then the same float64 bits).  Oracle results are computed in a thread pool (its C stages release
the GIL); batches hold distinct pairs."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import resize, synthetic  # noqa: E402
from oracle_pipeline import compare, oracle_get_depth  # noqa: E402

PLANES = (((0.3, 0.1, 1.0), 2.0), ((-0.2, 0.15, 1.0), 1.6), ((0.0, 0.0, 1.0), 2.5), ((0.1, -0.25, 1.0), 1.3))
POOL = 16


def _pool_map(fn, items):
    with ThreadPoolExecutor(min(POOL, len(items))) as ex:
        return list(ex.map(fn, items))


@pytest.fixture(scope="module")
def pairs_1080p():
    rec = synthetic.rig(1920, 1080)
    return rec, _pool_map(lambda i: synthetic.render_plane_pair(rec, *PLANES[i], seed=i)[:2], range(4))


def _matched_size(W, H):
    """The size the default matcher runs SGBM at (boxx.resize by max_size / max(h, w)): 1000 x 562 here."""
    return resize.target_hw((H, W), min(1000 / max(H, W), 1))


def _check(oracle, stereo, pairs, max_depth, single):
    """get_depth of pair ``single`` and get_depth_batch of all pairs against the oracle, pair by pair."""
    refs = _pool_map(lambda ab: oracle_get_depth(oracle, stereo, {}, *ab), pairs)
    got = stereo.get_depth(*pairs[single])
    bad, inexact = compare(got, refs[single])
    assert not bad and not inexact, ("get_depth", bad, inexact)
    gb = stereo.get_depth_batch(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]))
    for i, ref in enumerate(refs):
        bad, inexact = compare({k: np.asarray(v[i]) for k, v in gb.items()}, ref)
        assert not bad and not inexact, ("get_depth_batch", i, bad, inexact)
        assert (ref["rectify_depth"] > 0).mean() > 0.5, (i, "the comparison must run on real depths, not on zeros")


@pytest.mark.parametrize("max_depth", [None, 3.0])
def test_default_matcher_1080p(oracle, pairs_1080p, max_depth):
    """Four rendered planes at 1920x1080 (matched at 1000x562), one call and a batch of the four."""
    rec, pairs = pairs_1080p
    assert _matched_size(1920, 1080) == (562, 1000)
    stereo = ca.Stereo.load(rec)
    stereo.set_stereo_matching(ca.SemiGlobalBlockMatching({}), max_depth=max_depth)
    _check(oracle, stereo, pairs, max_depth, 2)


def test_default_matcher_4k(oracle, pairs_1080p):
    """Two distinct pairs at 3840x2160 (matched at 1000x562: the ratio 1000/3840), one call and a batch.  The pairs are
    two of the rendered 1080p planes doubled in both axes (rendering at 4K by ray casting takes a minute per image):
    the 4K rig's cameras see about the same scene, so the matcher finds real depths."""
    W, H = 3840, 2160
    assert _matched_size(W, H) == (562, 1000)
    up = lambda a: np.ascontiguousarray(a.repeat(2, 0).repeat(2, 1))  # noqa: E731
    pairs = [(up(a), up(b)) for a, b in pairs_1080p[1][:2]]
    stereo = ca.Stereo.load(synthetic.rig(W, H))
    stereo.set_stereo_matching(ca.SemiGlobalBlockMatching({}))
    _check(oracle, stereo, pairs, None, 1)


@pytest.mark.parametrize("W,H", [(1920, 1080), (3840, 2160)])
def test_resize_round_trip_at_full_size(oracle, W, H):
    """The kernel-level round trip of the default matcher, batched: u8 RGB down to 1000x562, float32 disparities back
    up to full size, every image against oracle.resize_linear bit for bit."""
    hw = _matched_size(W, H)
    assert hw == (562, 1000)
    rng = np.random.default_rng(W)
    imgs = np.stack([synthetic.scene_pair(s, W, H, 3)[0] for s in range(3)])
    imgs[2, : H // 3] = 255  # a saturated band: 255 must stay 255 through the 11-bit weights
    down = resize.resize(torch.from_numpy(imgs).cuda(), hw, batched=True).cpu().numpy()
    assert down.shape == (3,) + hw + (3,)
    for i in range(3):
        assert np.array_equal(down[i], oracle.resize_linear(imgs[i], hw)), ("u8 down", i)
    assert (down[2, :100] == 255).all()
    disp = (rng.integers(-16, 16 * 218, (3,) + hw) / np.float32(16)).astype(np.float32)
    disp[1, ::7] = -0.0
    up = resize.resize(torch.from_numpy(disp).cuda(), (H, W), batched=True).cpu().numpy()
    assert up.shape == (3, H, W)
    for i in range(3):
        want = oracle.resize_linear(disp[i], (H, W))
        assert np.array_equal(up[i].view(np.uint32), want.view(np.uint32)), ("f32 up", i)
