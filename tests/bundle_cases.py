"""Inputs of the bundle-adjustment tests (tests/test_bundle_cpu.py, tests/test_gpu_bundle.py, tests/bundle_tolerance.py) and
of tools/gpu_bundle_time.py.  Only DATA lives here: seeded, built on ``reconstruction_cases.scene`` (48 x 64 images, the true
poses known), regenerated on both sides of a comparison.

A pair's matches are the pixel centres of view a that land inside view b with where the flow takes them, subsampled by a
seeded choice (kept in row order) so that no test moves more than a few thousand points.  ``sigma`` adds Gaussian pixel
noise to both sides; ``NOISE_SIGMA`` = 0.03 px: the images are 64 px wide (f = 70 px), so this is the 0.3 .. 0.9 px of a 640 .. 1920 px frame that the other solvers' cases use; at 0.3 px here the poses are no better determined than the start perturbation.  The start poses are the truth turned
by up to ``START_ROTATION`` rad about a seeded axis and shifted by up to ``START_SHIFT`` per coordinate."""
import numpy as np

import reconstruction_cases as rc

NOISE_SIGMA = 0.03
SEED, NOISY_SEED = 11, 12
START_ROTATION, START_SHIFT = 0.02, 0.03
THRESHOLD = 4.0  # pixels, for the planted wrong matches: a planted one lies 16 px and more off its epipolar line

# name -> views, the scene's seed, matches a pair (one number for all pairs, or a list over the pairs in rising order)
CASES = {
    "three": dict(views=3, scene=1, per_pair=300),
    "five": dict(views=5, scene=2, per_pair=200),
    "sixteen": dict(views=16, scene=3, per_pair=20),
    "borders": dict(views=5, scene=2, per_pair=[1, 63, 64, 65, 255, 256, 257, 100, 100, 100]),
    "bad_pair": dict(views=4, scene=4, per_pair=150, bad_pair=2),
}
NAMES = tuple(CASES)
_SCENES = {}


def all_pairs(views):
    return [(a, b) for a in range(views) for b in range(a + 1, views)]


def scene(views, seed):
    if (views, seed) not in _SCENES:
        _SCENES[views, seed] = rc.scene(views, seed)
    return _SCENES[views, seed]


def pair_matches(flowd, n, rng):
    """n matches (uvs_a, uvs_b) float64 of one ordered pair's flow, a seeded choice in row order"""
    ys, xs = np.nonzero(flowd["common_fov_mask"])
    pick = np.sort(rng.choice(len(xs), size=n, replace=False))
    ua = np.stack([xs[pick] + 0.5, ys[pick] + 0.5], 1).astype(np.float64)
    return ua, ua + flowd["flow_abs"][ys[pick], xs[pick]].astype(np.float64)


def perturbed(Ts, rng):
    out = []
    for T in Ts:
        axis = rng.normal(size=3)
        P = np.eye(4)
        P[:3, :3] = rc._rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.5, 1.0) * START_ROTATION)
        P[:3, 3] = rng.uniform(-START_SHIFT, START_SHIFT, 3)
        out.append(T @ P)
    return np.array(out)


def case(name, sigma=0.0, seed=SEED, dtype=np.float64):
    """dict(K (N, 3, 3), T_true, T0 (N, 4, 4), pairs (P, 2), uvs_a, uvs_b (M, 2) of ``dtype``, counts (P,))"""
    c = CASES[name]
    viewds, flowds, Ts = scene(c["views"], c["scene"])
    rng = np.random.default_rng(seed)
    pairs = all_pairs(c["views"])
    per_pair = c["per_pair"] if isinstance(c["per_pair"], list) else [c["per_pair"]] * len(pairs)
    uas, ubs = [], []
    for (a, b), n in zip(pairs, per_pair):
        ua, ub = pair_matches(flowds[(a, b)], n, rng)
        if sigma:
            ua, ub = ua + rng.normal(0, sigma, ua.shape), ub + rng.normal(0, sigma, ub.shape)
        uas.append(ua), ubs.append(ub)
    if "bad_pair" in c:  # every match of this pair is bad: non-finite, or behind the views
        p = c["bad_pair"]
        uas[p][::2] = np.nan
        ubs[p][1::2] = uas[p][1::2] + (ubs[p][1::2] - uas[p][1::2]) * -40.0
    T0 = perturbed(Ts, rng)
    return dict(name=name, K=np.array([viewds[k]["K"] for k in range(c["views"])]), T_true=np.array(Ts), T0=T0,
                pairs=np.array(pairs, np.int32), uvs_a=np.concatenate(uas).astype(dtype), uvs_b=np.concatenate(ubs).astype(dtype),
                counts=np.array(per_pair, np.int64))


def epipolar_distance(c, p, ua, ub):
    """distance in px of ub from the epipolar line of ua in view b of pair p, under the case's START poses"""
    a, b = (int(v) for v in c["pairs"][p])
    Tab = np.linalg.inv(c["T0"][b]) @ c["T0"][a]  # view a's camera frame -> view b's
    R, t = Tab[:3, :3], Tab[:3, 3]
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    F = np.linalg.inv(c["K"][b]).T @ E @ np.linalg.inv(c["K"][a])
    line = np.c_[ua, np.ones(len(ua))] @ F.T
    return np.abs((line * np.c_[ub, np.ones(len(ub))]).sum(1)) / np.hypot(line[:, 0], line[:, 1])


def planted(c, swaps_per_pair=3, seed=5, min_distance=4.0):
    """(the case with wrong matches planted, the rows planted): in every pair of at least 20 rows, ``swaps_per_pair`` times
    two rows exchange their view-b pixels, chosen so that both then lie at least ``min_distance`` x THRESHOLD px off their
    epipolar lines under the start poses (a swap along the line is a wrong depth, which no reprojection error shows).
    ``without(planted case, rows)`` is the input without those rows."""
    rng = np.random.default_rng(seed)
    ua, ub = c["uvs_a"].astype(np.float64), c["uvs_b"].copy()
    rows, at = [], 0
    for p, n in enumerate(c["counts"]):
        n = int(n)
        taken = set()
        for _ in range(swaps_per_pair if n >= 20 else 0):
            for _try in range(500):
                i, j = (int(v) for v in rng.choice(n, 2, replace=False))
                d = epipolar_distance(c, p, ua[[at + i, at + j]], ub[[at + j, at + i]].astype(np.float64))
                if i in taken or j in taken or d.min() < min_distance * THRESHOLD:
                    continue
                ub[[at + i, at + j]] = ub[[at + j, at + i]]
                taken.update((i, j))
                rows += [at + i, at + j]
                break
        at += n
    return dict(c, uvs_b=ub), np.array(sorted(rows))


def without(c, rows):
    keep = np.ones(len(c["uvs_a"]), bool)
    keep[rows] = False
    bounds = np.concatenate([[0], np.cumsum(c["counts"])])
    counts = np.array([int(keep[bounds[p]:bounds[p + 1]].sum()) for p in range(len(c["counts"]))], np.int64)
    return dict(c, uvs_a=c["uvs_a"][keep], uvs_b=c["uvs_b"][keep], counts=counts), keep


def reverse(c):
    """the same problem with its pairs and the rows of every pair in reversed order, and how to put per-row and per-pair
    results back: (case, row permutation, pair permutation) with reversed[i] = original[perm[i]]"""
    bounds = np.concatenate([[0], np.cumsum(c["counts"])])
    order = list(range(len(c["counts"])))[::-1]
    perm = np.concatenate([np.arange(bounds[p], bounds[p + 1])[::-1] for p in order]).astype(np.int64)
    return dict(c, pairs=c["pairs"][order], counts=c["counts"][order], uvs_a=c["uvs_a"][perm], uvs_b=c["uvs_b"][perm]), perm, np.array(order)


def single_pair(c, p):
    """the rows of pair p alone"""
    bounds = np.concatenate([[0], np.cumsum(c["counts"])])
    return slice(int(bounds[p]), int(bounds[p + 1]))
