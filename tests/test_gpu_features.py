"""The feature matcher on the GPU (-m gpu): every stage of csrc/features.hip alone, bit for bit against the NumPy restatement
(tests/features_ref.py), then ``match_images`` / ``BinaryFeatureMatching`` / ``match_views`` end to end on the ray-cast scene
of tests/features_cases.py.  ndarrays and CUDA tensors take turns."""
import functools

import numpy as np
import pytest
import torch

import calibrating_amd as ca
from calibrating_amd import features

import essential_ref as er
import features_cases as fc
import features_ref as fr
from test_features_cpu import FLOORS

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _kind(a, cuda):
    return _cuda(a) if cuda else a


@functools.lru_cache(maxsize=None)
def _image(name):
    if name == "scene":
        return fc.pose_pair()["img1"]
    if name == "scene2":
        return fc.pose_pair()["img2"]
    if name == "colour":
        return fc.colour_of(fc.pose_pair()["img1"])
    if name == "dots":
        return fc.dots_image()
    if name == "flat":
        return np.full((67, 93), 90, np.uint8)
    kind, h, w = name.split("_")
    assert kind == "noise"
    return fc.noise_image(int(h), int(w), seed=int(h) * 1000 + int(w))


@functools.lru_cache(maxsize=None)
def _reference(name, threshold, cell):
    """the restatement's (score, xy, scores, descriptors, bins) of a named image: computed once, shared, never written to"""
    gray = fr.gray_of(_image(name))
    score = fr.score_plane(gray, threshold)
    xy, scores = fr.keypoints(score, cell)
    desc, bins = fr.describe(gray, xy)
    return score, xy, scores, desc, bins


# (image, threshold, cell): 40 x 48 is the smallest size with an interior, 32 x 100 has none, 67 x 93 is no multiple of a
# cell or of the score kernel's 64 x 16 tile; threshold 1 on noise occupies every block, 255 none
STAGE_A = [("noise_40_48", 20, 8), ("noise_32_100", 1, 8), ("noise_67_93", 20, 8), ("noise_67_93", 1, 4), ("noise_67_93", 1, 13),
           ("noise_67_93", 1, 64), ("noise_67_93", 255, 8), ("flat", 1, 8), ("dots", 20, 8), ("dots", 20, 4), ("dots", 20, 13),
           ("dots", 20, 64), ("scene", 20, 8), ("colour", 20, 8), ("scene", 1, 8)]


@pytest.mark.parametrize("case", range(len(STAGE_A)))
def test_score_plane_and_keypoints(case):
    name, threshold, cell = STAGE_A[case]
    img, cuda = _image(name), case % 2 == 1
    score, xy, scores, _, _ = _reference(name, threshold, cell)
    got = features._score_plane(_kind(img, cuda), threshold)
    assert isinstance(got, torch.Tensor) == cuda and got.dtype == (torch.uint8 if cuda else np.uint8)
    assert np.array_equal(_host(got), score)
    gxy, gscores, gcounts = (_host(v) for v in features._keypoints_of(_kind(score[None], cuda), cell))
    h, w = score.shape
    cap = -(-h // cell) * -(-w // cell)
    n = len(xy)
    assert gxy.shape == (1, cap, 2) and gxy.dtype == np.int32 and gcounts.tolist() == [n]
    assert np.array_equal(gxy[0, :n], xy) and np.array_equal(gscores[0, :n], scores)
    assert (gxy[0, n:] == -1).all() and not gscores[0, n:].any()
    if name == "noise_32_100" or name == "flat" or threshold == 255:
        assert n == 0


@pytest.mark.parametrize("cuda", [False, True])
def test_a_batch_of_different_frames_and_each_alone(cuda):
    names = ["noise_67_93", "flat", "noise_67_93"]
    frames = np.stack([_image(n) for n in names])
    frames[2] = frames[2][::-1, ::-1]  # a third, different frame
    out = features.detect_and_describe(_kind(frames, cuda), return_info=True)
    assert list(out) == ["xy", "descriptors", "counts", "bins", "scores"]
    assert all(isinstance(v, torch.Tensor) == cuda for v in out.values())
    again = features.detect_and_describe(_kind(frames, cuda), return_info=True)
    for k in out:
        assert _host(out[k]).tobytes() == _host(again[k]).tobytes()  # two runs give the same bytes
    counts = _host(out["counts"])
    assert counts[1] == 0
    for f in range(3):
        ref = fr.detect_and_describe(frames[f])
        n = len(ref["xy"])
        assert counts[f] == n
        for k in ("xy", "descriptors", "bins", "scores"):
            assert np.array_equal(_host(out[k])[f, :n], ref[k]), (f, k)
        assert (_host(out["xy"])[f, n:] == -1).all() and not _host(out["descriptors"])[f, n:].any()
        alone = features.detect_and_describe(_kind(frames[f], cuda), return_info=True)
        for got, k in zip(alone, ("xy", "descriptors", "bins", "scores")):
            assert _host(got).shape[0] == n and np.array_equal(_host(got), ref[k])


def test_a_pitched_view_and_colour_are_read_in_place():
    img = _image("scene")
    big = torch.zeros((2, 240 + 9, 320 + 21), dtype=torch.uint8, device="cuda")
    big[0, 4:244, 7:327] = _cuda(img)
    big[1, 4:244, 7:327] = _cuda(_image("scene2"))
    view = big[:, 4:244, 7:327]
    assert not view.is_contiguous()
    out = features.detect_and_describe(view)
    for f, name in enumerate(("scene", "scene2")):
        _, xy, _, desc, _ = _reference(name, 20, 8)
        n = len(xy)
        assert int(out["counts"][f]) == n and np.array_equal(_host(out["xy"][f, :n]), xy)
        assert np.array_equal(_host(out["descriptors"][f, :n]), desc)
    colour = _image("colour")
    _, xy, _, desc, _ = _reference("colour", 20, 8)
    gxy, gdesc = features.detect_and_describe(colour)
    assert np.array_equal(gxy, xy) and np.array_equal(gdesc, desc)
    wide = torch.zeros((240, 330, 3), dtype=torch.uint8, device="cuda")
    wide[:, 5:325] = _cuda(colour)
    gxy, gdesc = features.detect_and_describe(wide[:, 5:325])
    assert np.array_equal(_host(gxy), xy) and np.array_equal(_host(gdesc), desc)


@pytest.mark.parametrize("cuda", [False, True])
def test_descriptors_and_bins_for_given_keypoints(cuda):
    img = _image("noise_67_93")
    h, w = img.shape
    B = fr.BORDER
    # exactly BORDER from each edge, one step too near each edge, and the middle
    xy = np.array([[B, B], [w - B - 1, B], [B, h - B - 1], [w - B - 1, h - B - 1], [B - 1, 30], [w - B, 30], [40, B - 1], [40, h - B],
                   [w // 2, h // 2], [0, 0]], np.int32)
    flat = np.full((h, w), 77, np.uint8)
    frames = np.stack([img, flat])
    xys = np.stack([xy, xy])
    counts = np.array([len(xy) - 1, len(xy)], np.int32)  # the last slot of frame 0 lies beyond its count
    desc, bins = (_host(v) for v in features._describe_at(_kind(frames, cuda), _kind(xys, cuda), _kind(counts, cuda)))
    for f in range(2):
        rd, rb = fr.describe(frames[f], xy[:counts[f]])
        assert np.array_equal(desc[f, :counts[f]], rd) and np.array_equal(bins[f, :counts[f]], rb)
    assert bins[0, :4].min() >= 0 and bins[0, 4:8].tolist() == [-1] * 4 and not desc[0, 4:8].any()
    assert bins[0, 9] == -1 and not desc[0, 9].any()          # beyond the count: the fill stays
    assert bins[1, 8] == 0 and not desc[1, 8].any()           # a flat patch: bin 0, no box is below its equal
    patches = fc.turned_patches()
    c = patches.shape[1] // 2
    xy = np.tile(np.array([[[c, c]]], np.int32), (len(patches), 1, 1))
    desc, bins = (_host(v) for v in features._describe_at(_kind(patches, cuda), _kind(xy, cuda),
                                                          _kind(np.ones(len(patches), np.int32), cuda)))
    assert sorted(bins[:, 0].tolist()) == list(range(32))
    for k, p in enumerate(patches):
        rd, rb = fr.describe(p, xy[k])
        assert np.array_equal(desc[k], rd) and np.array_equal(bins[k], rb)


SIZES = [(0, 5), (5, 0), (1, 1), (2, 1), (1, 2), (63, 64), (64, 65), (65, 63), (255, 256), (256, 257), (257, 255), (1000, 1000),
         (1000, 257), (2, 1000)]


@functools.lru_cache(maxsize=None)
def _sets(n1, n2):
    d1, d2 = fc.planted_sets(n1, n2, seed=31 * n1 + n2)
    return d1, d2, fr.search(d1, d2), fr.search(d2, d1)


@pytest.mark.parametrize("case", range(len(SIZES)))
def test_search_and_filter_against_the_restatement(case):
    n1, n2 = SIZES[case]
    d1, d2, fwd, back = _sets(n1, n2)
    cuda = case % 2 == 0
    if n1 and n2:  # the search alone, both directions in one launch
        t1, t2 = _cuda(d1)[None], _cuda(d2)[None]
        c1, c2 = (torch.tensor([n], dtype=torch.int32, device="cuda") for n in (n1, n2))
        best12, dist12, best21, dist21 = (_host(v) for v in features._search(t1, c1, t2, c2, torch.zeros((1, 2), dtype=torch.int32,
                                                                                                           device="cuda")))
        for best, dist, ref in ((best12, dist12, fwd), (best21, dist21, back)):
            assert np.array_equal(best[0], ref[0]) and np.array_equal(dist[0, :, 0], ref[1]) and np.array_equal(dist[0, :, 1], ref[2])
    for knobs in (dict(), dict(cross_check=False), dict(ratio=(1, 1)), dict(max_distance=0), dict(max_distance=256, ratio=(1, 1)),
                  dict(max_distance=256, ratio=(1, 1), cross_check=False)):
        m, d = features.match_descriptors(_kind(d1, cuda), _kind(d2, cuda), **knobs)
        assert isinstance(m, torch.Tensor) == cuda
        rm, rd = fr.match(d1, d2, **knobs)
        assert _host(m).dtype == np.int32 and np.array_equal(_host(m), rm) and np.array_equal(_host(d), rd), knobs
    if n1 == 1000 and n2 == 1000:
        assert len(fr.match(d1, d2)[0]) > 100 and len(fr.match(d1, d2, max_distance=0)[0]) > 0  # the planted rows are found


def test_all_zeros_against_all_ones_and_the_sentinel():
    zeros, ones = np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8)
    m, d = features.match_descriptors(zeros, ones, max_distance=256, ratio=(1, 1))
    assert m.tolist() == [[0, 0]] and d.tolist() == [256]
    assert len(features.match_descriptors(zeros, ones, max_distance=255, ratio=(1, 1))[0]) == 0
    assert len(features.match_descriptors(zeros, ones, max_distance=256)[0]) == 0  # 256 * 5 > 4 * 257
    out = features._search(_cuda(zeros)[None], torch.ones(1, dtype=torch.int32, device="cuda"), _cuda(ones)[None],
                           torch.ones(1, dtype=torch.int32, device="cuda"), torch.zeros((1, 2), dtype=torch.int32, device="cuda"))
    assert _host(out[0]).tolist() == [[0]] and _host(out[1]).tolist() == [[[256, 257]]]


@pytest.mark.parametrize("cuda", [False, True])
def test_a_batch_of_pairs_with_different_counts(cuda):
    cap = 300
    d = np.stack([fc.planted_sets(cap, cap, seed=s)[k] for s, k in ((1, 0), (1, 1), (2, 1))])
    counts = np.array([cap, 0, 37], np.int32)  # frame 1 is empty
    pairs = np.array([[0, 1], [0, 2], [2, 0], [1, 1], [0, 0]], np.int32)
    for knobs in (dict(), dict(ratio=(1, 1), cross_check=False)):
        m, dist, n = (_host(v) for v in features.match_descriptors(_kind(d, cuda), _kind(d, cuda), _kind(counts, cuda),
                                                                   _kind(counts, cuda), pairs, **knobs))
        assert m.shape == (5, cap, 2) and dist.shape == (5, cap) and n.shape == (5,)
        for p, (a, b) in enumerate(pairs.tolist()):
            rm, rd = fr.match(d[a, :counts[a]], d[b, :counts[b]], **knobs)
            assert n[p] == len(rm) and np.array_equal(m[p, :n[p]], rm) and np.array_equal(dist[p, :n[p]], rd)
            assert (m[p, n[p]:] == -1).all() and (dist[p, n[p]:] == -1).all()
        assert n[0] == 0 and n[3] == 0 and n[4] > 0
    # a pair alone gives what it gives in the batch
    alone = features.match_descriptors(d[0], d[2, :37])
    assert np.array_equal(alone[0], fr.match(d[0], d[2, :37])[0])


@functools.lru_cache(maxsize=None)
def _scene_matches(which):
    p = fc.pose_pair() if which == "pose" else fc.rectified_pair()
    return fr.match_images(p["img1"], p["img2"])


@pytest.mark.parametrize("cuda", [False, True])
def test_match_images_feeds_the_essential_matrix(cuda):
    """Measured with the restatement (tests/test_features_cpu.py, MEASURED): 311 matches, 0.8875 of them within 2 px, the
    robust pose 0.0308 rad / 0.3574 rad off.  The GPU's matches are the restatement's bits; the floors are asserted on them."""
    p = fc.pose_pair()
    u1, u2 = features.match_images(_kind(p["img1"], cuda), _kind(p["img2"], cuda))
    assert isinstance(u1, torch.Tensor) == cuda and _host(u1).dtype == np.float64
    r1, r2, _ = _scene_matches("pose")
    assert np.array_equal(_host(u1), r1) and np.array_equal(_host(u2), r2)
    err = np.linalg.norm(fc.truth(p, _host(u1)) - _host(u2), axis=1)
    assert len(r1) >= max(8, FLOORS["matches"]) and (err <= 2).mean() >= FLOORS["share"]
    info = ca.find_essential_matrix(u1, u2, p["K"], return_info=True)
    ref = er.find(r1, r2, p["K"], p["K"])
    assert info["status"] == "ok" and info["n_inliers"] == ref["n_inliers"]
    assert np.array_equal(_host(info["inliers"]), ref["inliers"]) and np.array_equal(info["E"], ref["E"])
    rotation, direction = er.pose_error(info["E"], p["R"], p["t"])
    assert rotation <= FLOORS["rotation"] and direction <= FLOORS["direction"]
    st = ca.EssentialMatrixStereo(u1, u2, p["K"], p["K"], baseline=float(np.linalg.norm(p["t"])), xy1=(fc.W, fc.H), xy2=(fc.W, fc.H),
                                  robust=True)
    assert st.robust_info["status"] == "ok" and np.array_equal(st.epipolar["E"], ref["E"])
    angle = np.arccos(np.clip((np.trace(st.R @ p["R"].T) - 1) / 2, -1, 1))
    assert angle <= FLOORS["rotation"]


@pytest.mark.parametrize("cuda", [False, True])
def test_the_matcher_through_stereo_get_depth(cuda):
    """``FeatureMatchingAsStereoMatching(BinaryFeatureMatching(), downscale=1)`` as the matcher of a rectified rig: the
    matches are the restatement's of the rectified images the call itself returns, and the disparity image holds
    u1 - u2 at every match."""
    r = fc.rectified_pair()
    Kl = r["K"].tolist()
    rig = dict(R=np.eye(3).tolist(), t=[[float(v)] for v in r["t"]], cam1=dict(K=Kl, D=[[0.0] * 5], xy=[fc.W, fc.H], name="cam1"),
               cam2=dict(K=Kl, D=[[0.0] * 5], xy=[fc.W, fc.H], name="cam2"))
    stereo = ca.Stereo.load(rig)
    matcher = ca.BinaryFeatureMatching()
    stereo.set_stereo_matching(ca.FeatureMatchingAsStereoMatching(matcher, downscale=1))
    res = stereo.get_depth(_kind(r["img1"], cuda), _kind(r["img2"], cuda))
    matched = res["matched"]  # (the plugin is handed the rectified CUDA tensors, so its matches are tensors either way)
    assert isinstance(matched["uvs1"], torch.Tensor) and isinstance(res["disparity"], torch.Tensor) == cuda
    r1, r2, rd = fr.match_images(_host(res["rectify_img1"]), _host(res["rectify_img2"]))
    wh = np.array([fc.W, fc.H], np.float64)
    assert len(r1) >= 8
    assert np.array_equal(_host(matched["uvs1"]), r1 / wh) and np.array_equal(_host(matched["uvs2"]), r2 / wh)
    assert np.array_equal(_host(matched["distance"]), rd)
    assert _host(matched["uvs1"]).max() < 1 and _host(matched["uvs1"]).min() >= 0
    at = r1.astype(int)  # the nearest fill leaves a sample's own value on its own pixel (inside the rig's valid mask)
    valid = np.asarray(stereo.rectify_valid_mask1).astype(bool)[at[:, 1], at[:, 0]]
    assert np.array_equal(_host(res["disparity"])[at[:, 1], at[:, 0]], np.where(valid, (r1 - r2)[:, 0], 0).astype(np.float32))
    if np.array_equal(_host(res["rectify_img1"]), r["img1"]) and np.array_equal(_host(res["rectify_img2"]), r["img2"]):
        # the rig is rectified already: the true correspondence of the scene applies to what was matched
        disparity = (r1 - r2)[:, 0]
        assert np.median(np.abs(disparity - (r1 - fc.truth(r, r1))[:, 0])) <= FLOORS["disparity"]


@pytest.mark.parametrize("cuda", [False, True])
def test_match_views_gives_set2ds(cuda):
    p, r = fc.pose_pair(), fc.rectified_pair()
    views = [p["img1"], p["img2"], r["img2"]]
    set2ds = features.match_views([_kind(v, cuda) for v in views])
    assert sorted(tuple(sorted(k)) for k in set2ds) == [(0, 1), (0, 2), (1, 2)]
    for key, d in set2ds.items():
        i, j = sorted(key)
        r1, r2, _ = fr.match_images(views[i], views[j])
        assert isinstance(d["uvs_i"], torch.Tensor) == cuda and sorted(d) == ["uvs_i", "uvs_j"]
        assert np.array_equal(_host(d["uvs_i"]), r1) and np.array_equal(_host(d["uvs_j"]), r2)
    one = features.match_views(np.stack(views), pairs=[[2, 0]])
    assert list(one) == [frozenset((0, 2))]
    assert np.array_equal(one[frozenset((0, 2))]["uvs_i"], _host(set2ds[frozenset((0, 2))]["uvs_i"]))
