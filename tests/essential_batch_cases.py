"""The fixtures of the batched RANSAC estimator (tests/test_essential_batch_cpu.py, tests/test_gpu_essential_batch.py) and of
the robust reconstruction (tests/test_gpu_reconstruction_robust.py).  Only DATA lives here: everything is regenerated from
seeds on both sides of a comparison.

The batch.  Four views that differ in K: views 0 and 1 are the two cameras of tests/essential_cases.py, views 2 and 3 show
the same pictures scaled and shifted (K' = A K, pixels' = A pixels), so a pair of any two of them is a scene of that rig.
Pair p holds ``SIZES[p]`` matches of a scene of its own seed; from 63 rows up about 30 % of them are wrong pairs."""
import functools

import numpy as np

import essential_cases as es

# the edges of a wave (64), of the score workgroup (1024) and of the moments' 256-row blocks (4097 = 16 blocks and one row);
# the empty pair and the 7-row pair stand in the middle
SIZES = (9, 63, 1024, 8, 0, 65, 1023, 7, 4097, 64, 1025)
# (view of uvs_a, view of uvs_b): even views show camera 1 of the rig, odd views camera 2; pair 5 is given as (b, a), b > a
VIEW_PAIRS = ((0, 1), (2, 1), (0, 3), (2, 3), (0, 1), (3, 0), (2, 1), (0, 3), (2, 3), (0, 1), (1, 2))
HYPOTHESES = (1, 64, 65, 300)
SEED = 11
AFFINE = {0: (1.0, 0.0, 0.0), 1: (1.0, 0.0, 0.0), 2: (1.25, -17.0, 9.5), 3: (0.75, 31.0, -12.25)}  # view -> (scale, du, dv)


def _A(view):
    s, du, dv = AFFINE[view]
    return np.array([[s, 0, du], [0, s, dv], [0, 0, 1.0]])


def intrinsics():
    """K (4, 3, 3) of the four views"""
    s = es.scene(n=8, noise=0.0)
    return np.stack([_A(v) @ (s["K1"] if v % 2 == 0 else s["K2"]) for v in range(4)])


def pair_rows(n, views, seed):
    """(uvs_a, uvs_b) float64 of ``n`` matches as the views ``views = (a, b)`` see them"""
    if n == 0:
        return np.zeros((0, 2)), np.zeros((0, 2))
    s = es.scene(n=n, noise=0.3, wrong=0.3 if n >= 63 else 0.0, seed=seed)
    out = []
    for v in views:
        uv = s["uvs1"] if v % 2 == 0 else s["uvs2"]
        sc, du, dv = AFFINE[v]
        out.append(uv * sc + np.array([du, dv]))
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def batch(dtype="float64", sizes=SIZES, view_pairs=VIEW_PAIRS):
    """dict(K, pairs (P, 2) int32, uvs_a, uvs_b (M, 2) of ``dtype``, counts (P,) int64, bounds (P + 1,)) -- shared, never
    written to"""
    rows = [pair_rows(n, vp, 5000 + 13 * p + n) for p, (n, vp) in enumerate(zip(sizes, view_pairs))]
    counts = np.array(sizes, np.int64)
    return dict(K=intrinsics(), pairs=np.array(view_pairs, np.int32), uvs_a=np.concatenate([r[0] for r in rows]).astype(dtype),
                uvs_b=np.concatenate([r[1] for r in rows]).astype(dtype), counts=counts, bounds=np.concatenate([[0], np.cumsum(counts)]))


def rows_of(b, p):
    return slice(int(b["bounds"][p]), int(b["bounds"][p + 1]))


def reordered(b, order):
    """the batch with its pairs in the order ``order`` (any subset)"""
    order = list(order)
    counts = b["counts"][order]
    return dict(K=b["K"], pairs=b["pairs"][order], uvs_a=np.concatenate([b["uvs_a"][rows_of(b, p)] for p in order]),
                uvs_b=np.concatenate([b["uvs_b"][rows_of(b, p)] for p in order]), counts=counts,
                bounds=np.concatenate([[0], np.cumsum(counts)]))


STAGE_SIZES, STAGE_VIEW_PAIRS, STAGE_HYPOTHESES = (65, 300, 7, 1025), ((0, 1), (3, 0), (0, 1), (2, 3)), 65


def with_degenerate():
    """three pairs, the middle one eight copies of one match (essential_cases.degenerate_inputs)"""
    b = batch("float64", (300, 65), ((0, 1), (0, 1)))
    d1, d2, _, _ = es.degenerate_inputs()
    counts = np.array([300, 8, 65], np.int64)
    return dict(K=b["K"], pairs=np.array([(0, 1), (0, 1), (0, 1)], np.int32), counts=counts, bounds=np.concatenate([[0], np.cumsum(counts)]),
                uvs_a=np.concatenate([b["uvs_a"][:300], d1, b["uvs_a"][300:]]), uvs_b=np.concatenate([b["uvs_b"][:300], d2, b["uvs_b"][300:]]))


# ---- the block tables -------------------------------------------------------------------------------------------------
def table_counts():
    """row counts for the block-table builder: the batch's own and a seeded random set"""
    rng = np.random.default_rng(77)
    return [list(SIZES), [int(v) for v in rng.integers(0, 6000, 40)], [300000, 0, 8], [262144, 262145]]


# ---- the robust reconstruction ------------------------------------------------------------------------------------------
# In every pair of a reconstruction case the uvs_j of a seeded share WRONG of the rows are permuted among themselves: wrong
# pairs with plausible coordinates.  ROBUST are the estimator's keywords the test passes as cfg["robust"].
WRONG = 0.3
WRONG_SEED = 1
ROBUST = dict(threshold=0.01, hypotheses=1024, seed=0)
# The bound on bundle_ref.pose_errors of the robust constructor = 4 x what the CPU composition leaves on the same scene:
# every pair filtered with essential_ref.find(**ROBUST), then the reference's own class on the filtered matches, printed by
#     python tests/golden/make_essential_batch_bound.py
# (build container only: it runs the reference checkout; its rigs take the estimator's matrix, as the constructor's do).  E
# and the masks of the GPU are bit-equal to the restatement's; the margin is for the class's later sums, which are equal only
# to its one-ulp sensitivity.  The scenes are 48 x 64 px and noise-free: at the default 1 px, 3.5 % of the inliers are wrong
# pairs and the CPU composition itself is 0.1 .. 0.2 rad off; at 0.01 px 3 of 9540 / 21 of 33462 are, and it lands within
# 0.05 rad and 5 % of the mean distance of the centres from view 0's (0.5419 / 0.2871), which the maker checks.
# name -> (rotation rad, centre) of the CPU composition, as printed
CPU_ERRORS = {"one_triple": (0.0005831869254383311, 0.0033898064974160107), "ten_triples": (0.0008413249113633054, 0.004391235652462689)}
BOUND_FACTOR = 4


def contaminated(set2ds, wrong=WRONG, seed=WRONG_SEED):
    """new set2ds (uvs_i, uvs_j only): in every pair, pairs in sorted order, a seeded share of uvs_j's rows permuted"""
    rng = np.random.default_rng(seed)
    out = {}
    for set2 in sorted(set2ds, key=sorted):
        ui, uj = np.array(set2ds[set2]["uvs_i"]), np.array(set2ds[set2]["uvs_j"])
        n = len(ui)
        bad = np.sort(rng.permutation(n)[: int(round(wrong * n))])
        uj[bad] = uj[rng.permutation(bad)]
        out[set2] = dict(uvs_i=ui, uvs_j=uj)
    return out
