"""find_essential_matrices without a GPU: every refusal comes before the device is touched, and the block tables (pure
Python, counts in, table out) cover every row of every taken pair exactly once with no block across two pairs."""
import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import epipolar_geometry as eg

import essential_batch_cases as ebc


def small():
    b = ebc.batch("float64", (300, 65), ((0, 1), (3, 0)))
    return dict(K=b["K"], pairs=b["pairs"], uvs_a=b["uvs_a"], uvs_b=b["uvs_b"], counts=b["counts"])


def refused(match, **change):
    a = dict(small(), **change)
    with pytest.raises((ValueError, TypeError), match=match):
        ca.find_essential_matrices(a.pop("K"), a.pop("pairs"), a.pop("uvs_a"), a.pop("uvs_b"), a.pop("counts"), **a)


def test_refusals_come_before_the_device():
    s = small()
    refused("K must be", K=s["K"][0])
    refused("pairs must be", pairs=s["pairs"].astype(np.float64))
    refused("pairs must be", pairs=s["pairs"].reshape(-1))
    refused("P == 0", pairs=np.zeros((0, 2), np.int32), counts=np.zeros(0, np.int64))
    refused("outside 0 .. 3", pairs=np.array([(0, 1), (4, 0)]))
    refused("outside 0 .. 3", pairs=np.array([(0, 1), (-1, 0)]))
    refused("a != b", pairs=np.array([(0, 1), (2, 2)]))
    refused("counts must be", counts=np.array([300, -65]))
    refused("counts must be", counts=np.array([365]))
    refused("counts must be", counts=np.array([300.0, 65.0]))
    refused("counts sum to 364", counts=np.array([300, 64]))
    refused("both be float64 or both float32", uvs_b=s["uvs_b"].astype(np.float32))
    refused("both be float64 or both float32", uvs_a=s["uvs_a"].astype(np.int32), uvs_b=s["uvs_b"].astype(np.int32))
    refused("same number", uvs_b=s["uvs_b"][:-1])
    refused(r"\(n, 2\)", uvs_a=np.zeros((365, 3)))
    refused("NumPy array or a torch CUDA tensor", uvs_a=s["uvs_a"].tolist())
    refused("hypotheses", hypotheses=0)
    refused("hypotheses", hypotheses=(1 << 20) + 1)
    refused("hypotheses", hypotheses=2.5)
    refused("threshold", threshold=0)
    refused("threshold", threshold=float("inf"))
    bad = s["uvs_a"].copy()
    bad[301, 1] = np.nan
    refused("finite", uvs_a=bad)
    K = s["K"].copy()
    K[3, 0, 0] = np.inf
    refused("finite", K=K)
    K = s["K"].copy()
    K[0] = 0
    refused("invertible", K=K)
    K = s["K"].copy()
    K[0, :2] *= -1
    K[1, :2] *= -1
    refused("positive mean focal", K=K)
    # a view no pair names may hold anything
    K = s["K"].copy()
    K[2] = np.nan
    with pytest.raises(ValueError, match="hypotheses"):
        ca.find_essential_matrices(K, s["pairs"], s["uvs_a"], s["uvs_b"], s["counts"], hypotheses=0)


def test_tensors_on_the_host_are_refused():
    import torch
    s = small()
    with pytest.raises(ValueError, match="GPU"):
        ca.find_essential_matrices(s["K"], s["pairs"], torch.from_numpy(s["uvs_a"]), torch.from_numpy(s["uvs_b"]), s["counts"])
    with pytest.raises(ValueError, match="GPU"):
        ca.find_essential_matrices(s["K"], s["pairs"], s["uvs_a"], torch.from_numpy(s["uvs_b"]), s["counts"])


def test_two_to_the_31_rows_are_refused_by_their_shape_alone():
    s = small()
    huge = np.broadcast_to(np.zeros((1, 2)), (2 ** 31, 2))  # (no memory behind it: only the shape is read)
    with pytest.raises(ValueError, match="below 2\\^31"):
        ca.find_essential_matrices(s["K"], s["pairs"], huge, huge, np.array([2 ** 31, 0]))


def test_pairs_of_fewer_than_eight_rows_need_no_device():
    b = ebc.batch("float32", (7, 0), ((0, 1), (3, 0)))
    res = ca.find_essential_matrices(b["K"], b["pairs"], b["uvs_a"], b["uvs_b"], b["counts"])
    assert res["status"].tolist() == [2, 2] and not res["E"].any() and res["E"].shape == (2, 3, 3)
    assert res["inliers"].dtype == np.bool_ and res["inliers"].shape == (7,) and not res["inliers"].any()
    assert not res["n_inliers"].any() and not res["refined"].any()


def test_estimate_and_robust_together_are_refused():
    s = small()
    with pytest.raises(ValueError, match="robust or estimate, not both"):
        ca.EssentialMatrixStereo(s["uvs_a"][:300], s["uvs_b"][:300], s["K"][0], s["K"][1], xy1=(1280, 720), xy2=(1280, 720), robust=True,
                                 estimate=dict(E=np.eye(3), status="ok"))


@pytest.mark.parametrize("counts", ebc.table_counts())
def test_score_blocks_cover_every_row_once_and_no_block_touches_two_pairs(counts):
    table = eg.essential_score_blocks(counts)
    assert table.dtype == np.int32 and table.shape[1] == 4
    hits = [np.zeros(n, np.int64) for n in counts]
    for p, g, G, _ in table.tolist():
        assert counts[p] >= 8 and 0 <= g < G == -(-counts[p] // 1024)
        lo, hi = 1024 * g, min(1024 * g + 1024, counts[p])  # the rows the workgroup reads: its 1024, cut at the pair's end
        assert lo < hi
        hits[p][lo:hi] += 1
    for n, h in zip(counts, hits):
        assert (h == (1 if n >= 8 else 0)).all()
    assert table[:, 0].tolist() == sorted(table[:, 0].tolist())  # pairs in order, a pair's blocks together
    assert set(table[:, 0].tolist()) == {p for p, n in enumerate(counts) if n >= 8}


@pytest.mark.parametrize("counts", ebc.table_counts())
def test_moments_tables_cover_every_row_once_in_the_single_calls_shape(counts):
    take = [n >= 8 and p % 3 != 1 for p, n in enumerate(counts)]
    blocks, finals = eg.essential_moments_tables(counts, take)
    assert blocks.dtype == finals.dtype == np.int32 and blocks.shape[1] == finals.shape[1] == 4
    assert finals[:, 0].tolist() == [p for p in range(len(counts)) if take[p]]
    hits = [np.zeros(n, np.int64) for n in counts]
    for p, g, G, _ in blocks.tolist():
        assert take[p] and 0 <= g < G == eg.essential_moments_blocks(counts[p]) == min(max(-(-counts[p] // 256), 1), 1024)
        for t0 in range(256 * g, counts[p], 256 * G):  # thread t adds rows 256 g + t, + 256 G, ...
            hits[p][t0:t0 + 256] += 1
    for p, h in enumerate(hits):
        assert (h == (1 if take[p] else 0)).all()
    for p, first, G, _ in finals.tolist():  # a pair's workgroups follow one another from `first`, g = 0 .. G - 1
        assert blocks[first:first + G, 0].tolist() == [p] * G and blocks[first:first + G, 1].tolist() == list(range(G))
    assert int(finals[:, 2].sum()) == len(blocks)
