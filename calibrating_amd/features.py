"""Keypoints, binary descriptors and a brute-force Hamming matcher on the GPU: matches from two pictures alone
(csrc/features.hip).

A contract of this package's OWN, stated operation by operation in ``include/calibrating_amd.h`` and restated in NumPy by
``tests/features_ref.py`` -- NOT ``cv2.ORB`` / ``cv2.BFMatcher`` (UNPINNED): integers end to end,
every tie defined, the same bits on every run.

  A  FAST-9 corner score (0 below ``threshold`` and within ``BORDER`` = 16 px of an edge); a pixel is a peak when its key
     ``score << 32 | (0xFFFFFFFF - (y * w + x))`` is the largest of its 3 x 3; every ``cell`` x ``cell`` block (aligned at
     pixel (0, 0)) keeps its peak of the largest key; a frame's keypoints are listed in row-major order of their blocks.
     The capacity ``ceil(h / cell) * ceil(w / cell)`` is a keypoint per block, so nothing is ever dropped.
  B  Orientation: one of 32 bins from the intensity centroid over a disc of radius 13; descriptor: 256 comparisons of 5 x 5
     box sums at the ends of ``brief_pattern(seed)``'s tests turned by the bin, 32 bytes.
  C  Hamming distance; ``best`` = the train row of the smallest (distance, index), ``second`` = the smallest distance among
     the others (257 when there is none); kept: ``d_best <= max_distance``, ``d_best * den <= num * d_second``, and with
     ``cross_check`` the best of its train row, searched the other way, is this query.  Matches come in query order.

Out of scope: a scale pyramid (the views must have comparable scale, as a rig's or a walk-around's do), sub-pixel
keypoints, rotation beyond what 32 bins resolve, cv2 parity, ``vis_flow``, passing ``robust`` through
``ReconstructionExtrinsics``.  For a camera with a lens, ``cam.undistort_points`` the matches first.
"""
import numpy as np

from . import _native
from ._arrays import check_array, dtype_name, is_np, to_device
from ._frames import device_frames, integer, layout
from ._native import call
from .boards import _splitmix64
from .hostio import to_host_list

BORDER = 16               # CAMD_FEATURE_BORDER: the reach of a descriptor (14) plus the box (2)
MAX_SIDE = 16384
MAX_RATIO = 1 << 20
NO_SECOND = 257           # d_second where a query has no second train row
DEFAULTS = dict(threshold=20, cell=8, seed=0, max_distance=64, ratio=(4, 5), cross_check=True)
_DETECT_KNOBS, _MATCH_KNOBS = ("threshold", "cell", "seed"), ("max_distance", "ratio", "cross_check")

_PATTERNS = {}         # seed -> the host table
_DEVICE_PATTERNS = {}  # (seed, device) -> the table on that device: uploaded once, not once per call


def brief_pattern(seed=0):
    """The descriptor's tests, (32, 256, 4) int8: ``[k, i] = (x1, y1, x2, y2)`` of test i at rotation k.  Made on the host
    with plain integers drawn through ``boards._splitmix64`` from the state ``seed``: per test the coordinates x1, y1, x2,
    y2 in that order, each ``(z_a % 11) + (z_b % 11) - 10`` of two successive draws (-10 .. 10, peaked at 0); a test whose
    two ends coincide is drawn again.  Rotation k is ``rint`` of the float64 rotation of both ends by ``2 pi k / 32``
    (x' = x cos - y sin, y' = x sin + y cos: towards +y, which is down in an image), so the reach is at most 14.  The
    same seed gives the same table everywhere."""
    seed = integer(seed, "seed") & 0xFFFFFFFFFFFFFFFF
    if seed not in _PATTERNS:
        state, base = seed, np.empty((256, 4), np.int64)
        for i in range(256):
            while True:
                c = []
                for _ in range(4):
                    state, za = _splitmix64(state)
                    state, zb = _splitmix64(state)
                    c.append(za % 11 + zb % 11 - 10)
                if (c[0], c[1]) != (c[2], c[3]):
                    break
            base[i] = c
        table = np.empty((32, 256, 4), np.int8)
        for k in range(32):
            a = 2.0 * np.pi * k / 32.0
            co, si = np.cos(a), np.sin(a)
            x, y = base[:, 0::2].astype(np.float64), base[:, 1::2].astype(np.float64)
            table[k, :, 0::2] = np.rint(x * co - y * si)
            table[k, :, 1::2] = np.rint(x * si + y * co)
        table.setflags(write=False)
        if len(_PATTERNS) >= 64:
            _PATTERNS.clear()
        _PATTERNS[seed] = table
    return _PATTERNS[seed]


def _device_pattern(seed, device):
    import torch
    key = (int(seed) & 0xFFFFFFFFFFFFFFFF, str(device))
    if key not in _DEVICE_PATTERNS:
        if len(_DEVICE_PATTERNS) >= 64:
            _DEVICE_PATTERNS.clear()
        _DEVICE_PATTERNS[key] = torch.from_numpy(np.array(brief_pattern(seed))).to(device)
    return _DEVICE_PATTERNS[key]


# ---- the refusals: all of them before the device is touched (the knobs take integer types only: 3.0 is refused) ------
def _detect_knobs(threshold, cell, seed):
    brief_pattern(seed)
    return integer(threshold, "threshold", (1, 255), strict=True), integer(cell, "cell", (4, 64), strict=True), int(seed)


def _match_knobs(max_distance, ratio, cross_check):
    max_distance = integer(max_distance, "max_distance", (0, 256), strict=True)
    try:
        num, den = ratio
        num, den = integer(num, "num", strict=True), integer(den, "den", strict=True)
    except (TypeError, ValueError):
        raise ValueError("ratio must be (num, den), two positive integers with num <= den, got %r" % (ratio,))
    if not 1 <= num <= den <= MAX_RATIO:
        raise ValueError("ratio must be (num, den), two positive integers with num <= den <= %d, got %r" % (MAX_RATIO, ratio))
    return max_distance, num, den, bool(cross_check)


def _split_knobs(knobs):
    unknown = sorted(set(knobs) - set(DEFAULTS))
    if unknown:
        raise TypeError("unknown argument(s) %s; the knobs are %s" % (", ".join(unknown), ", ".join(DEFAULTS)))
    k = dict(DEFAULTS, **knobs)
    return _detect_knobs(*(k[n] for n in _DETECT_KNOBS)), _match_knobs(*(k[n] for n in _MATCH_KNOBS))


def _layout(images, what):
    """the frames of a detector's images as ``layout`` reads them off the shape, checked on the host"""
    check_array(images, what)
    return layout(images, what, max_side=MAX_SIDE)


def _same_kind(arrays, names):
    if len({is_np(a) for a in arrays}) > 1:
        raise TypeError("%s must all be NumPy arrays or all be CUDA tensors" % ", ".join(names))


# ---- the stages on device tensors --------------------------------------------------------------------------------------
def _score(gray, f, h, w, pitch, stride, threshold):
    import torch
    score = torch.empty((f, h, w), dtype=torch.uint8, device=gray.device)
    call("camd_feature_score", gray.device, gray.data_ptr(), w, h, pitch, stride, f, threshold, score.data_ptr(),
         what="feature_score")
    return score


def _keypoints(score, cell):
    import torch
    f, h, w = (int(v) for v in score.shape)
    cap = -(-h // cell) * -(-w // cell)
    xy = torch.full((f, cap, 2), -1, dtype=torch.int32, device=score.device)
    scores = torch.zeros((f, cap), dtype=torch.int32, device=score.device)
    counts = torch.empty(f, dtype=torch.int32, device=score.device)
    ws = torch.empty(_native.lib().camd_feature_keypoints_workspace_bytes(w, h, f, cell), dtype=torch.uint8, device=score.device)
    call("camd_feature_keypoints", score.device, score.data_ptr(), w, h, f, cell, ws.data_ptr(), xy.data_ptr(), scores.data_ptr(),
         counts.data_ptr(), what="feature_keypoints")
    return xy, scores, counts


def _describe(gray, f, h, w, pitch, stride, xy, counts, seed):
    import torch
    cap = int(xy.shape[1])
    desc = torch.zeros((f, cap, 32), dtype=torch.uint8, device=gray.device)
    bins = torch.full((f, cap), -1, dtype=torch.int32, device=gray.device)
    call("camd_feature_describe", gray.device, gray.data_ptr(), w, h, pitch, stride, f, xy.data_ptr(), counts.data_ptr(), cap,
         _device_pattern(seed, gray.device).data_ptr(), desc.data_ptr(), bins.data_ptr(), what="feature_describe")
    return desc, bins


def _search(d1, c1, d2, c2, pairs):
    """(best12 (P, cap1), dist12 (P, cap1, 2), best21 (P, cap2), dist21 (P, cap2, 2)) int32 on the device"""
    import torch
    (f1, cap1), (f2, cap2), P, dev = d1.shape[:2], d2.shape[:2], int(pairs.shape[0]), d1.device
    best12 = torch.empty((P, cap1), dtype=torch.int32, device=dev)
    dist12 = torch.empty((P, cap1, 2), dtype=torch.int32, device=dev)
    best21 = torch.empty((P, cap2), dtype=torch.int32, device=dev)
    dist21 = torch.empty((P, cap2, 2), dtype=torch.int32, device=dev)
    call("camd_feature_search", dev, d1.data_ptr(), c1.data_ptr(), int(f1), int(cap1), d2.data_ptr(), c2.data_ptr(), int(f2),
         int(cap2), pairs.data_ptr(), P, best12.data_ptr(), dist12.data_ptr(), best21.data_ptr(), dist21.data_ptr(),
         what="feature_search")
    return best12, dist12, best21, dist21


def _filter(c1, f1, cap2, pairs, best12, dist12, best21, max_distance, num, den, cross_check):
    """(matches (P, cap1, 2) filled with -1, distances (P, cap1) filled with -1, counts (P,)) int32 on the device"""
    import torch
    P, cap1, dev = int(best12.shape[0]), int(best12.shape[1]), best12.device
    matches = torch.full((P, cap1, 2), -1, dtype=torch.int32, device=dev)
    distances = torch.full((P, cap1), -1, dtype=torch.int32, device=dev)
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    ws = torch.empty(_native.lib().camd_feature_filter_workspace_bytes(P), dtype=torch.uint8, device=dev)
    call("camd_feature_filter", dev, c1.data_ptr(), int(f1), cap1, int(cap2), pairs.data_ptr(), P, best12.data_ptr(), dist12.data_ptr(),
         best21.data_ptr(), max_distance, num, den, int(cross_check), ws.data_ptr(), matches.data_ptr(), distances.data_ptr(),
         counts.data_ptr(), what="feature_filter")
    return matches, distances, counts


def _match(d1, c1, d2, c2, pairs, match_knobs):
    best12, dist12, best21, _ = _search(d1, c1, d2, c2, pairs)
    return _filter(c1, d1.shape[0], d2.shape[1], pairs, best12, dist12, best21, *match_knobs)


def _detect(images, lay, detect_knobs):
    """dict(xy, scores, counts, descriptors, bins) on the device for checked images"""
    threshold, cell, seed = detect_knobs
    fr = device_frames(images, lay, "rgb")
    xy, scores, counts = _keypoints(_score(fr.data, fr.f, fr.h, fr.w, fr.pitch, fr.stride, threshold), cell)
    desc, bins = _describe(fr.data, fr.f, fr.h, fr.w, fr.pitch, fr.stride, xy, counts, seed)
    return dict(xy=xy, scores=scores, counts=counts, descriptors=desc, bins=bins)


def _host(d, was_np):
    """a dict of tensors as the caller's kind (one synchronisation)"""
    if not was_np:
        return d
    keys = list(d)
    return dict(zip(keys, to_host_list(*(d[k] for k in keys))))


# ---- the stages alone, for tests and measurements (NumPy in -> NumPy out) ------------------------------------------------
def _score_plane(images, threshold=20):
    """Stage A's score plane, uint8 in the shape of the gray image(s)."""
    threshold = _detect_knobs(threshold, 8, 0)[0]
    lay = _layout(images, "images")
    fr = device_frames(images, lay, "rgb")
    score = _score(fr.data, fr.f, fr.h, fr.w, fr.pitch, fr.stride, threshold)
    return _host(dict(s=score if lay.batched else score[0]), is_np(images))["s"]


def _keypoints_of(score, cell=8):
    """Stage A's keypoints of score planes (f, h, w) uint8 -> (xy (f, cap, 2) filled with -1, scores (f, cap), counts (f,))."""
    cell = _detect_knobs(20, cell, 0)[1]
    if _layout(score, "score").colour or score.ndim != 3:
        raise ValueError("score must be (f, h, w), got %s" % (tuple(score.shape),))
    out = _keypoints(to_device(score), cell)
    return tuple(_host(dict(enumerate(out)), is_np(score)).values())


def _describe_at(images, xy, counts, seed=0):
    """Stage B for given keypoints: images (f, h, w[, 3]), xy (f, cap, 2) int32, counts (f,) int32 -> (descriptors
    (f, cap, 32), bins (f, cap)); a slot beyond its frame's count keeps zeros and -1."""
    _detect_knobs(20, 8, seed)
    lay = _layout(images, "images")
    check_array(xy, "xy")
    check_array(counts, "counts")
    _same_kind((images, xy, counts), ("images", "xy", "counts"))
    if dtype_name(xy) != "int32" or dtype_name(counts) != "int32":
        raise ValueError("xy and counts must be int32, got %s and %s" % (xy.dtype, counts.dtype))
    if not lay.batched or xy.ndim != 3 or tuple(xy.shape[::2]) != (lay.f, 2) or xy.shape[1] < 1 or tuple(counts.shape) != (lay.f,):
        raise ValueError("images (f, h, w[, 3]) take xy (f, cap, 2) with cap >= 1 and counts (f,), got %s, %s and %s"
                         % (tuple(images.shape), tuple(xy.shape), tuple(counts.shape)))
    fr = device_frames(images, lay, "rgb")
    dev = fr.data.device
    out = _describe(fr.data, fr.f, fr.h, fr.w, fr.pitch, fr.stride, to_device(xy, device=dev), to_device(counts, device=dev), seed)
    return tuple(_host(dict(enumerate(out)), is_np(images)).values())


# ---- the public calls --------------------------------------------------------------------------------------------------
def detect_and_describe(images, threshold=20, cell=8, seed=0, return_info=False):
    """Keypoints and their 32-byte descriptors (stages A and B of the module's contract), every frame in one pass.

    ``images``: uint8 gray (h, w) / (f, h, w) or colour (h, w, 3) / (f, h, w, 3) (through ``cvt_gray(code="rgb")``), NumPy
    arrays or CUDA tensors (pitched views are read in place; the results stay on the tensor's device and current stream).
    One image -> ``(xy (n, 2) int32, descriptors (n, 32) uint8)``, trimmed to its keypoints; a batch -> ``dict(xy (f, cap,
    2) filled with -1, descriptors (f, cap, 32), counts (f,) int32)`` with ``cap = ceil(h / cell) * ceil(w / cell)``.
    ``return_info`` adds the orientation bin and the score (int32): two more arrays, or ``bins`` and ``scores`` in the
    dict.  An image with a side below 33 has no keypoints.  ``threshold`` 1 .. 255, ``cell`` 4 .. 64."""
    knobs = _detect_knobs(threshold, cell, seed)
    lay = _layout(images, "images")
    d = _detect(images, lay, knobs)
    keys = ("xy", "descriptors") + (("bins", "scores") if return_info else ())
    if lay.batched:
        return _host({k: d[k] for k in keys[:2] + ("counts",) + keys[2:]}, is_np(images))
    n = int(d["counts"][0])
    out = _host({k: d[k][0, :n] for k in keys}, is_np(images))
    return tuple(out[k] for k in keys)


def _check_descriptors(desc, what):
    check_array(desc, what)
    if dtype_name(desc) != "uint8" or desc.ndim not in (2, 3) or desc.shape[-1] != 32:
        raise ValueError("%s must be uint8 (n, 32) or (f, cap, 32), got %s %s" % (what, desc.dtype, tuple(desc.shape)))


def _check_counts(counts, frames, cap, what, host_only=False):
    """counts (f,) checked against the capacity; ``host_only``: a tensor is left for later (its check reads the device)"""
    if counts is None or (host_only and hasattr(counts, "is_cuda")):
        return counts
    c = counts if hasattr(counts, "is_cuda") else np.asarray(counts)
    check_array(c, what)
    if dtype_name(c) not in ("int32", "int64") or tuple(c.shape) != (frames,):
        raise ValueError("%s must be %d integers (int32 or int64), got %s %s" % (what, frames, c.dtype, tuple(c.shape)))
    if int(c.min()) < 0 or int(c.max()) > cap:
        raise ValueError("%s must lie in 0 .. %d (the capacity), got %d .. %d" % (what, cap, int(c.min()), int(c.max())))
    return c


def _device_counts(counts, frames, cap, device):
    import torch
    if counts is None:
        return torch.full((frames,), cap, dtype=torch.int32, device=device)
    return to_device(counts, dtype="int32", cast=True, device=device)


def _check_pairs(pairs, f1, f2):
    """pairs as a host (P, 2) int32 array inside the frames; None: (i, i)"""
    if pairs is None:
        if f1 != f2:
            raise ValueError("without pairs the two sets need the same number of frames, got %d and %d" % (f1, f2))
        return np.repeat(np.arange(f1, dtype=np.int32)[:, None], 2, 1)
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in "iu":
        raise ValueError("pairs must be (P, 2) integers, got %s %s" % (p.dtype, p.shape))
    if len(p) > 65535:
        raise ValueError("at most 65535 pairs in one call, got %d" % len(p))
    if len(p) and (p.min() < 0 or p[:, 0].max() >= f1 or p[:, 1].max() >= f2):
        raise ValueError("pairs index outside the frames: %d and %d frames" % (f1, f2))
    return np.ascontiguousarray(p, np.int32)


def match_descriptors(desc1, desc2, counts1=None, counts2=None, pairs=None, max_distance=64, ratio=(4, 5), cross_check=True):
    """Stage C of the module's contract, single or batched.

    Single: ``desc1`` (n1, 32), ``desc2`` (n2, 32) uint8 -> ``(matches (m, 2) int32 of (row of desc1, row of desc2),
    distances (m,) int32)`` in query order.  Batched: ``desc1`` (f1, cap1, 32) with ``counts1`` (f1,), ``desc2`` (f2, cap2,
    32) with ``counts2`` (None: every row counts) and ``pairs`` (P, 2) of (frame of desc1, frame of desc2) -- default
    (i, i) -- -> ``(matches (P, cap1, 2) filled with -1, distances (P, cap1) filled with -1, counts (P,))``, all pairs
    searched in one launch.  The two sets may be the same array.  An empty side gives no matches and is not an error.
    NumPy arrays or CUDA tensors, not mixed; identical calls give identical bits."""
    import torch
    knobs = _match_knobs(max_distance, ratio, cross_check)
    _check_descriptors(desc1, "desc1")
    _check_descriptors(desc2, "desc2")
    _same_kind((desc1, desc2), ("desc1", "desc2"))
    if desc1.ndim != desc2.ndim:
        raise ValueError("desc1 and desc2 must both be (n, 32) or both be (f, cap, 32), got %s and %s"
                         % (tuple(desc1.shape), tuple(desc2.shape)))
    was_np, single = is_np(desc1), desc1.ndim == 2
    if single and not (counts1 is None and counts2 is None and pairs is None):
        raise ValueError("counts and pairs go with batched descriptors (f, cap, 32)")
    (f1, cap1), (f2, cap2) = ((1, int(d.shape[0])) if single else (int(d.shape[0]), int(d.shape[1])) for d in (desc1, desc2))
    if not single and (f1 < 1 or f2 < 1):
        raise ValueError("batched descriptors need at least one frame each, got %d and %d" % (f1, f2))
    device = None if was_np else desc1.device
    if not was_np and desc2.device != device:
        raise ValueError("inputs live on different devices: %s and %s" % (desc2.device, device))
    host_pairs = _check_pairs(pairs, f1, f2)
    counts1 = _check_counts(counts1, f1, cap1, "counts1", host_only=True)  # (host counts: before the device is touched)
    counts2 = _check_counts(counts2, f2, cap2, "counts2", host_only=True)
    P = len(host_pairs)
    if P == 0 or cap1 == 0:  # nothing to ask
        empty = np.zeros if was_np else (lambda s, t: torch.zeros(s, dtype=getattr(torch, np.dtype(t).name), device=device))
        if single:
            return empty((0, 2), np.int32), empty((0,), np.int32)
        return empty((P, cap1, 2), np.int32), empty((P, cap1), np.int32), empty((P,), np.int32)
    d1 = to_device(desc1).reshape(f1, cap1, 32)
    d2 = to_device(desc2, device=d1.device).reshape(f2, cap2, 32)
    c1 = _device_counts(_check_counts(counts1, f1, cap1, "counts1"), f1, cap1, d1.device)
    c2 = _device_counts(_check_counts(counts2, f2, cap2, "counts2"), f2, cap2, d1.device)
    if cap2 == 0:  # an empty train side: one row that does not count
        d2 = torch.zeros((f2, 1, 32), dtype=torch.uint8, device=d1.device)
    matches, distances, counts = _match(d1, c1, d2, c2, torch.from_numpy(host_pairs).to(d1.device), knobs)
    if single:
        m = int(counts[0])
        matches, distances = matches[0, :m], distances[0, :m]
        return tuple(to_host_list(matches, distances)) if was_np else (matches, distances)
    return tuple(to_host_list(matches, distances, counts)) if was_np else (matches, distances, counts)


def _uvs(xy, rows):
    """float64 pixel coordinates (m, 2) of keypoint rows (m,) int32 of one frame's xy"""
    import torch
    return xy[rows.long()].to(torch.float64)


def _match_two(img1, img2, knobs):
    """(uvs1, uvs2, distances) on the device, (w, h) of the first image"""
    import torch
    detect_knobs, match_knobs = _split_knobs(knobs)
    layouts = [_layout(img, name) for img, name in ((img1, "img1"), (img2, "img2"))]
    _same_kind((img1, img2), ("img1", "img2"))
    for lay, name in zip(layouts, ("img1", "img2")):
        if lay.batched:
            raise ValueError("%s must be one image (h, w) or (h, w, 3); match_views takes batches" % name)
    a = _detect(img1, layouts[0], detect_knobs)
    dev = a["xy"].device
    b = _detect(img2, layouts[1], detect_knobs)
    if b["xy"].device != dev:
        raise ValueError("inputs live on different devices: %s and %s" % (b["xy"].device, dev))
    pairs = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    matches, distances, counts = _match(a["descriptors"], a["counts"], b["descriptors"], b["counts"], pairs, match_knobs)
    m = int(counts[0])
    return (_uvs(a["xy"][0], matches[0, :m, 0]), _uvs(b["xy"][0], matches[0, :m, 1]), distances[0, :m]), layouts[0].w, layouts[0].h


def match_images(img1, img2, **knobs):
    """Matched points of two pictures: ``(uvs1, uvs2)``, float64 pixel coordinates (m, 2) of the caller's kind, in the
    order of the first image's keypoints -- straight into ``find_essential_matrix`` or ``EssentialMatrixStereo(...,
    robust=True)`` (wrong pairs are what a classical matcher produces; the robust estimator is made for them).  For a
    camera with a lens, ``cam.undistort_points`` both first.  ``knobs``: threshold, cell, seed, max_distance, ratio,
    cross_check, as in ``detect_and_describe`` and ``match_descriptors``.  The images may differ in size."""
    (uvs1, uvs2, _), _, _ = _match_two(img1, img2, knobs)
    return tuple(to_host_list(uvs1, uvs2)) if is_np(img1) else (uvs1, uvs2)


class BinaryFeatureMatching:
    """The matcher ``FeatureMatchingAsStereoMatching`` expects: ``__call__(img1, img2)`` -> ``dict(uvs1, uvs2, distance)``
    with ``uvs*`` (m, 2) float64 normalised by (w, h) into [0, 1) and ``distance`` (m,) int32.  ``cfg``: a dict of
    ``match_images``' knobs (and whatever else the caller keeps there).  CUDA images give CUDA matches."""

    accepts_device_tensors = True

    def __init__(self, cfg=None):
        self.cfg = dict(cfg or {})
        _split_knobs({k: v for k, v in self.cfg.items() if k in DEFAULTS})

    def __call__(self, img1, img2):
        import torch
        (uvs1, uvs2, distance), w, h = _match_two(img1, img2, {k: v for k, v in self.cfg.items() if k in DEFAULTS})
        if tuple(img2.shape[:2]) != (h, w):
            raise ValueError("img1 and img2 must share one size, got %s and %s" % (tuple(img1.shape), tuple(img2.shape)))
        wh = torch.tensor([w, h], dtype=torch.float64, device=uvs1.device)
        out = dict(uvs1=uvs1 / wh, uvs2=uvs2 / wh, distance=distance)
        return _host(out, is_np(img1))


def match_views(images, pairs=None, **knobs):
    """Every view described once, all pairs matched in ONE search launch -> ``set2ds`` as ``ReconstructionExtrinsics(viewds,
    set2ds=...)`` takes it: ``{frozenset((i, j)): dict(uvs_i, uvs_j)}`` with i < j, float64 pixels (m, 2) of the caller's
    kind.  ``images``: (f, h, w[, 3]) uint8 or a sequence of f images of one size; ``pairs``: (P, 2) view indices with
    ``i != j`` (default: all i < j).  ``knobs`` as ``match_images``."""
    import torch
    detect_knobs, match_knobs = _split_knobs(knobs)
    if isinstance(images, (list, tuple)):
        if not images:
            raise ValueError("images is empty")
        for k, img in enumerate(images):
            check_array(img, "images[%d]" % k)
        _same_kind(images, ("the views",))
        if len({tuple(img.shape) for img in images}) != 1:
            raise ValueError("views must share one size, got %s" % sorted({tuple(img.shape) for img in images}))
        if len({str(img.dtype) for img in images}) != 1:
            raise ValueError("views must share one dtype")
        images = np.stack(images) if is_np(images[0]) else torch.stack(list(images))
    lay = _layout(images, "images")
    if not lay.batched:
        raise ValueError("images must be a batch (f, h, w[, 3]) or a sequence of views, got %s" % (tuple(images.shape),))
    f = lay.f
    if pairs is None:
        pairs = [(i, j) for i in range(f) for j in range(i + 1, f)]
    host_pairs = _check_pairs(np.asarray(pairs, np.int64).reshape(-1, 2) if len(pairs) else np.zeros((0, 2), np.int64), f, f)
    if len(host_pairs) == 0:
        raise ValueError("at least one pair of views is required (%d view(s))" % f)
    if (host_pairs[:, 0] == host_pairs[:, 1]).any():
        raise ValueError("a pair needs two different views")
    host_pairs = np.sort(host_pairs, 1)
    if len({tuple(p) for p in host_pairs.tolist()}) != len(host_pairs):
        raise ValueError("pairs repeat")
    d = _detect(images, lay, detect_knobs)
    dev = d["xy"].device
    matches, _, counts = _match(d["descriptors"], d["counts"], d["descriptors"], d["counts"], torch.from_numpy(host_pairs).to(dev),
                                match_knobs)
    ms = [int(c) for c in counts.tolist()]
    out = {}
    for p, ((i, j), m) in enumerate(zip(host_pairs.tolist(), ms)):
        out[frozenset((i, j))] = (_uvs(d["xy"][i], matches[p, :m, 0]), _uvs(d["xy"][j], matches[p, :m, 1]))
    if is_np(images):
        flat = to_host_list(*(t for v in out.values() for t in v))
        out = {k: (flat[2 * n], flat[2 * n + 1]) for n, k in enumerate(out)}
    return {k: dict(uvs_i=v[0], uvs_j=v[1]) for k, v in out.items()}
