"""The feature matcher without a GPU: the contract on hand-made inputs through its NumPy restatement (tests/features_ref.py),
the host side of calibrating_amd/features.py (the pattern table, every refusal before the device is touched), and the
geometric floors of the rendered scene (tests/features_cases.py)."""
import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import features

import essential_ref as er
import features_cases as fc
import features_ref as fr

# Measured with the restatement on the rendered scene (features_cases.pose_pair / rectified_pair, seed 20), defaults
# threshold 20, cell 8, ratio (4, 5), max_distance 64, cross_check: 879 and 873 keypoints, 311 matches, 0.8875 of them within
# 2 px of the true correspondence; the robust pose (essential_ref.find, defaults) is 0.0308 rad off in rotation and 0.3574 rad
# in translation direction, status "ok" with 274 inliers; on the rectified pair 364 matches with a median absolute disparity
# error of 0.3173 px.  The floors: half the count, 0.9 of the share, twice the errors.
MEASURED = dict(matches=311, share=0.8875, rotation=0.0308, direction=0.3574, disparity=0.3173)
FLOORS = dict(matches=MEASURED["matches"] / 2, share=0.9 * MEASURED["share"], rotation=2 * MEASURED["rotation"],
              direction=2 * MEASURED["direction"], disparity=2 * MEASURED["disparity"])


def test_a_lone_pixel_scores_its_height_and_a_flat_image_has_no_keypoints():
    img = np.full((40, 48), 100, np.uint8)
    assert not fr.score_plane(img, 1).any() and len(fr.keypoints(fr.score_plane(img, 1))[0]) == 0
    img[20, 25] = 150
    s = fr.score_plane(img, 20)
    assert s[20, 25] == 50 and np.count_nonzero(s) == 1
    xy, scores = fr.keypoints(s)
    assert xy.tolist() == [[25, 20]] and scores.tolist() == [50]
    assert not fr.score_plane(img, 51).any()           # below the threshold
    dark = np.full((40, 48), 100, np.uint8)
    dark[20, 25] = 70
    assert fr.score_plane(dark, 20)[20, 25] == 30      # darker counts alike
    img[:] = 100
    img[15, 25] = 150                                  # within BORDER of the top edge
    assert not fr.score_plane(img, 1).any()
    assert not fr.score_plane(np.full((32, 100), 7, np.uint8), 1).any()  # no interior at all


def test_equal_scores_resolve_to_the_lower_pixel_index():
    img = fc.dots_image()
    s = fr.score_plane(img, 20)
    dots = np.argwhere(s)
    assert len(dots) == 64 and set(s[s != 0].tolist()) == {150}  # 8 x 8 dots inside the border, all alike
    xy8, _ = fr.keypoints(s, 8)
    assert len(xy8) == 64                                         # one per block
    xy16, _ = fr.keypoints(s, 16)
    assert len(xy16) == 16 and all(x % 16 == 4 and y % 16 == 4 for x, y in xy16.tolist())  # of four equals the top-left
    flat = np.zeros((40, 40), np.uint8)
    flat[20, 20:22] = 9   # two equal neighbours: only the first in pixel order is a peak
    key = fr.keys_of(flat)
    assert key[20, 20] > key[20, 21]
    assert fr.keypoints(flat, 8)[0].tolist() == [[20, 20]]


def test_the_pattern_table():
    t = features.brief_pattern(0)
    assert t.shape == (32, 256, 4) and t.dtype == np.int8
    assert np.abs(t[0]).max() <= 10 and np.abs(t).max() <= 14
    assert not ((t[0, :, 0] == t[0, :, 2]) & (t[0, :, 1] == t[0, :, 3])).any()  # no test compares a box with itself
    features._PATTERNS.clear()
    again = features.brief_pattern(0)
    assert again is not t and np.array_equal(again, t)
    assert not np.array_equal(features.brief_pattern(1), t)
    # rotation k is the rounded rotation of rotation 0; a half turn negates, a quarter turn maps (x, y) to (-y, x)
    assert np.array_equal(t[16], -t[0])
    assert np.array_equal(t[8, :, 0::2], -t[0, :, 1::2]) and np.array_equal(t[8, :, 1::2], t[0, :, 0::2])
    with pytest.raises(ValueError):
        features.brief_pattern(0.5)


def test_the_matcher_tie_rule_and_its_sentinel():
    rng = np.random.default_rng(0)
    d2 = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    d2[4] = d2[1]                                      # a duplicated train row
    d1 = d2[[1]].copy()
    best, dbest, dsecond = fr.search(d1, d2)
    assert best.tolist() == [1] and dbest.tolist() == [0] and dsecond.tolist() == [0]  # the lowest index; the twin is second
    best, dbest, dsecond = fr.search(d1, d2[:1])
    assert best.tolist() == [0] and dsecond.tolist() == [257]                          # no second row
    best, dbest, dsecond = fr.search(d1, d2[:0])
    assert best.tolist() == [-1] and dbest.tolist() == [257] and dsecond.tolist() == [257]
    assert len(fr.match(d1, d2[:0])[0]) == 0 and len(fr.match(d2[:0], d1)[0]) == 0      # an empty side: no matches
    # a twin at distance 0 passes the ratio test (0 * 5 <= 4 * 0), a lone row passes on the sentinel
    assert fr.match(d1, d2)[0].tolist() == [[0, 1]]
    assert fr.match(d1, d2[1:2])[0].tolist() == [[0, 0]]
    zeros, ones = np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8)
    assert fr.search(zeros, ones)[1].tolist() == [256]
    assert len(fr.match(zeros, ones, 255, (1, 1))[0]) == 0 and fr.match(zeros, ones, 256, (1, 1))[1].tolist() == [256]
    assert len(fr.match(zeros, ones, 256)[0]) == 0  # 256 * 5 > 4 * 257: the default ratio refuses it on the sentinel
    # cross-check: two queries share a best train row, only the nearer one is its best
    d2 = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    d1 = np.stack([d2[0], d2[0]])
    d1[1, 0] ^= 1
    assert fr.match(d1, d2, ratio=(1, 1))[0].tolist() == [[0, 0]]
    assert fr.match(d1, d2, ratio=(1, 1), cross_check=False)[0].tolist() == [[0, 0], [1, 0]]


def test_a_turned_patch_visits_all_32_bins():
    patches = fc.turned_patches()
    c = patches.shape[1] // 2
    bins = [fr.orientation(p, c, c) for p in patches]
    assert sorted(bins) == list(range(32))
    assert fr.orientation(np.full((33, 33), 90, np.uint8), 16, 16) == 0  # a flat patch: every bin ties, the lowest wins
    desc, b = fr.describe(patches[0], np.array([[c, c], [3, c]], np.int32))
    assert b.tolist() == [bins[0], -1] and desc[0].any() and not desc[1].any()


GOOD = np.zeros((40, 48), np.uint8)
DESC = np.zeros((4, 32), np.uint8)


@pytest.mark.parametrize("call", [
    lambda: features.detect_and_describe(GOOD.astype(np.float32)),
    lambda: features.detect_and_describe(GOOD.astype(np.int8)),
    lambda: features.detect_and_describe(np.zeros((2, 40, 48, 4), np.uint8)),
    lambda: features.detect_and_describe(np.zeros(40, np.uint8)),
    lambda: features.detect_and_describe(np.zeros((0, 48), np.uint8)),
    lambda: features.detect_and_describe(GOOD, threshold=0),
    lambda: features.detect_and_describe(GOOD, threshold=256),
    lambda: features.detect_and_describe(GOOD, threshold=20.5),
    lambda: features.detect_and_describe(GOOD, cell=3),
    lambda: features.detect_and_describe(GOOD, cell=65),
    lambda: features.match_images(GOOD, GOOD, max_distance=-1),
    lambda: features.match_images(GOOD, GOOD, max_distance=257),
    lambda: features.match_images(GOOD, GOOD, ratio=(5, 4)),
    lambda: features.match_images(GOOD, GOOD, ratio=(0, 4)),
    lambda: features.match_images(GOOD, GOOD, ratio=(0.8, 1)),
    lambda: features.match_images(GOOD, GOOD, ratio=4),
    lambda: features.match_images(GOOD, GOOD.astype(np.uint16)),
    lambda: features.match_images(GOOD[None], GOOD),
    lambda: features.match_descriptors(DESC, DESC, ratio=(3, 2)),
    lambda: features.match_descriptors(DESC, DESC, max_distance=300),
    lambda: features.match_descriptors(DESC.astype(np.int32), DESC),
    lambda: features.match_descriptors(np.zeros((4, 16), np.uint8), DESC),
    lambda: features.match_descriptors(DESC, DESC[None]),
    lambda: features.match_descriptors(DESC[None], DESC[None], pairs=[[0, 1]]),
    lambda: features.match_descriptors(DESC[None], DESC[None], pairs=[[-1, 0]]),
    lambda: features.match_descriptors(DESC[None], DESC[None], pairs=[0, 0]),
    lambda: features.match_descriptors(DESC[None], DESC[None], counts1=np.array([5], np.int32)),
    lambda: features.match_descriptors(DESC[None], DESC[None], counts2=np.array([-1], np.int32)),
    lambda: features.match_descriptors(DESC[None], DESC[None], counts1=np.array([1, 1], np.int32)),
    lambda: features.match_descriptors(DESC[None], np.stack([DESC, DESC])),
    lambda: features.match_descriptors(DESC, DESC, counts1=np.array([1], np.int32)),
    lambda: features.BinaryFeatureMatching(dict(cell=2)),
    lambda: features.BinaryFeatureMatching()(GOOD.astype(np.float64), GOOD),
    lambda: features.match_views([GOOD, GOOD[:, :40]]),
    lambda: features.match_views(GOOD[None]),
    lambda: features.match_views(np.stack([GOOD] * 3), pairs=[[0, 3]]),
    lambda: features.match_views(np.stack([GOOD] * 3), pairs=[[1, 1]]),
    lambda: features.match_views(np.stack([GOOD] * 3).astype(np.float32)),
    lambda: features.match_views(np.stack([GOOD] * 3), cell=100),
])
def test_refused_before_the_device_is_touched(call):
    with pytest.raises(ValueError):
        call()


def test_mixed_kinds_and_unknown_knobs_are_type_errors():
    import torch

    class FakeCuda(torch.Tensor):  # a tensor that says it lives on the GPU: the checks must not look any further
        is_cuda = True
    t = torch.zeros((40, 48), dtype=torch.uint8).as_subclass(FakeCuda)
    d = torch.zeros((4, 32), dtype=torch.uint8).as_subclass(FakeCuda)
    with pytest.raises(TypeError):
        features.match_images(GOOD, t)
    with pytest.raises(TypeError):
        features.match_descriptors(DESC, d)
    with pytest.raises(TypeError):
        features.match_views([GOOD, t])
    with pytest.raises(TypeError):
        features.match_images(GOOD, GOOD, radius=3)
    with pytest.raises(TypeError):
        features.detect_and_describe([[1, 2], [3, 4]])
    with pytest.raises(ValueError):
        features.detect_and_describe(torch.zeros((40, 48), dtype=torch.uint8))  # a CPU tensor


def test_exports():
    for name in ("BinaryFeatureMatching", "detect_and_describe", "match_descriptors", "match_images", "match_views"):
        assert name in ca.__all__ and getattr(ca, name) is getattr(features, name)
    assert features.BinaryFeatureMatching(dict(cell=16, shape=(240, 320))).cfg == dict(cell=16, shape=(240, 320))
    assert features.BinaryFeatureMatching.accepts_device_tensors is True


def test_empty_sides_are_not_an_error_and_need_no_device():
    m, d = features.match_descriptors(DESC[:0], DESC)
    assert m.shape == (0, 2) and d.shape == (0,) and m.dtype == np.int32
    m, d, c = features.match_descriptors(DESC[None, :0], DESC[None])
    assert m.shape == (1, 0, 2) and d.shape == (1, 0) and c.tolist() == [0]


def test_geometric_floors_of_the_rendered_scene():
    """The restatement on the rendered scene; see MEASURED above for the figures the floors come from."""
    p = fc.pose_pair()
    u1, u2, _ = fr.match_images(p["img1"], p["img2"])
    err = np.linalg.norm(fc.truth(p, u1) - u2, axis=1)
    share = float((err <= 2).mean())
    info = er.find(u1, u2, p["K"], p["K"])
    rotation, direction = er.pose_error(info["E"], p["R"], p["t"])
    r = fc.rectified_pair()
    v1, v2, _ = fr.match_images(r["img1"], r["img2"])
    disparity = float(np.median(np.abs((v1 - v2)[:, 0] - (v1 - fc.truth(r, v1))[:, 0])))
    print("matches %d share %.4f rotation %.4f direction %.4f disparity %.4f (rectified matches %d, inliers %d)"
          % (len(u1), share, rotation, direction, disparity, len(v1), info["n_inliers"]))
    assert len(u1) >= 8 and info["status"] != "degenerate"   # the two fixed conditions
    assert len(u1) >= FLOORS["matches"]
    assert share >= FLOORS["share"]
    assert rotation <= FLOORS["rotation"] and direction <= FLOORS["direction"]
    assert disparity <= FLOORS["disparity"]
