"""The shared compaction (csrc/compact.hpp: row count -> exclusive scan -> ordered emit) through every entry point that
uses it, at the sizes where it can go wrong: the edges of a 64-lane wave and of a 256-element chunk in a row (widths),
the carry of the scan between its 256-row iterations (heights), and a capacity below the total (-m gpu).  Expected values
are plain NumPy; every index, coordinate and order is compared with array_equal, and the points of
depth_to_point_cloud -- a matrix product in NumPy -- bit for bit with the exact C oracle (oracle/pointcloud_ref.c)."""
import numpy as np
import pytest
import torch

from calibrating_amd import _native, epipolar_geometry as eg, pointcloud, sparse
from oracle import pointcloud_ref
import sparse_ref

pytestmark = pytest.mark.gpu

# (h, w): widths around the wave and chunk edges at height 3, heights around the scan's 256-row iterations at width 5
SHAPES = [(3, w) for w in (1, 63, 64, 65, 255, 256, 257, 513)] + [(h, 5) for h in (1, 255, 256, 257, 513)]
K = np.array([[420.0, 0, 161.3], [0, 424.0, 118.9], [0, 0, 1]])


def _masks(h, w):
    """name -> (h, w) bool.  The last one is not a mask of single pixels but of whole rows: only the last row of every 256
    is on, so that each iteration of the scan hands a carry to the next and nothing else moves the offsets."""
    yy, xx = np.mgrid[:h, :w]
    return {
        "all off": np.zeros((h, w), bool),
        "all on": np.ones((h, w), bool),
        "last lane of each wave": xx % 64 == 63,
        "first of each 256 chunk": xx % 256 == 0,
        "seeded 30 %": np.random.default_rng(h * 1000 + w).random((h, w)) < 0.3,
        "last row of each 256": yy % 256 == 255,
    }


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("h,w", SHAPES)
def test_masked_rows(h, w):
    rng = np.random.default_rng(w * 7 + h)
    arrs = rng.normal(size=(h, w)), rng.integers(-9, 9, (h, w))  # float64 rows, int64 rows
    for name, mask in _masks(h, w).items():
        for arr in arrs:
            got = sparse.arr2d_to_uvzs(arr, mask)
            want = sparse_ref.rows_of(arr, mask)
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, arr.dtype)


@pytest.mark.parametrize("h,w", SHAPES)
def test_flow_to_matched_uvs(h, w):
    rng = np.random.default_rng(w * 11 + h)
    for flow in (np.float32(rng.normal(0, 3, (h, w, 2))), rng.normal(0, 3, (h, w, 2))):
        for name, mask in _masks(h, w).items():
            ys, xs = np.nonzero(mask)
            want_from = np.stack([xs + 0.5 - 1e-8, ys + 0.5 - 1e-8], 1)
            want_to = np.float64(flow[ys, xs]) + want_from
            got_from, got_to = eg.flow_to_matched_uvs(flow, mask)
            assert got_from.dtype == np.float64 and got_to.dtype == np.float64
            assert np.array_equal(got_from, want_from) and np.array_equal(got_to, want_to), (name, flow.dtype)


@pytest.mark.parametrize("rate", [1, 1.5])  # 1.5: the sampling grid is wider than the depth
@pytest.mark.parametrize("h,w", SHAPES)
def test_depth_to_point_cloud(h, w, rate, oracle):
    z = 1.0 + np.random.default_rng(w * 13 + h).random((h, w))
    for name, mask in _masks(h, w).items():
        depth = np.where(mask, z, 0.0)
        got = pointcloud.depth_to_point_cloud(depth, K, interpolation_rate=rate, return_xyzuv=True)
        want = pointcloud_ref.depth_to_point_cloud(depth, K, interpolation_rate=rate, return_xyzuv=True)
        assert got.shape == want.shape and got.dtype == np.float64, name
        assert np.array_equal(got[:, 3:], want[:, 3:]), name                          # same pixels in the same order
        assert np.allclose(got[:, :3], want[:, :3], rtol=1e-13, atol=1e-13), name     # BLAS vs left-to-right products
        assert got.tobytes() == oracle.depth_to_point_cloud(depth, K, rate, return_xyzuv=True).tobytes(), name


def _matching_np(uvs1, uvs2):
    """matching_uvs_in_one_img at MAX_DISTANCE 1: np.unique of the cell rows twice, np.intersect1d of them."""
    firsts = []
    for uv in (uvs1, uvs2):
        cells, first = np.unique(np.int32(uv.round()), axis=0, return_index=True)  # rows sorted by (u, v)
        firsts.append((cells[:, 0].astype(np.int64) * (1 << 20) + cells[:, 1], first))   # the same order as one key
    _, a, b = np.intersect1d(firsts[0][0], firsts[1][0], assume_unique=True, return_indices=True)
    return firsts[0][1][a], firsts[1][1][b]


@pytest.mark.parametrize("cells_w,cells_h", [(3, 257), (300, 1)])
def test_intersection_window_height(cells_w, cells_h):
    rng = np.random.default_rng(cells_h)
    sets = []
    for _ in range(2):
        cells = np.stack([rng.integers(0, cells_w, 600), rng.integers(0, cells_h, 600)], 1)
        cells[:2] = [[0, 0], [cells_w - 1, cells_h - 1]]  # the window is exactly cells_w x cells_h
        sets.append(cells + rng.uniform(-0.3, 0.3, cells.shape))
    want1, want2 = _matching_np(*sets)
    assert len(want1) >= 100
    got = eg.matching_uvs_in_one_img(sets[0], sets[1])
    assert got["uv_match_idx1"].dtype == np.int64
    assert np.array_equal(got["uv_match_idx1"], want1) and np.array_equal(got["uv_match_idx2"], want2)


@pytest.mark.parametrize("n", [1, 256, 257, 1025])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_filter_overlap_uvs(n, dtype):
    rng = np.random.default_rng(n)
    side = int(np.ceil(np.sqrt(3 * n)))  # about a third of the pixels hit: a good share of the rows collide
    uvs1, uvs2 = (dtype(rng.integers(0, side, (n, 2)) + rng.uniform(-0.3, 0.3, (n, 2))) for _ in range(2))
    keep = np.ones(n, bool)
    for uv in (uvs1, uvs2):
        _, inverse, counts = np.unique(np.int32(uv.round()), axis=0, return_inverse=True, return_counts=True)
        keep &= counts[inverse.reshape(-1)] == 1
    assert n == 1 or 0 < keep.sum() < n
    got1, got2 = eg.filter_overlap_uvs(uvs1, uvs2)
    assert got1.dtype == dtype and got2.dtype == dtype
    assert np.array_equal(got1, uvs1[keep]) and np.array_equal(got2, uvs2[keep])


def test_capacity_below_the_total():
    """The raw C ABI with capacity = total - 1: *count is the full total, the first capacity rows are right and the row
    after them keeps its sentinel."""
    lib, st = _native.lib(), _native.current_stream()
    h, w = 257, 70  # two iterations of the scan; the last row holds the rows that do not fit
    rng = np.random.default_rng(5)
    mask = rng.random((h, w)) < 0.3
    mask[-1, -3:] = True
    total = int(mask.sum())
    m = torch.from_numpy(mask).cuda().view(torch.uint8)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.camd_arr2d_mask_workspace_bytes(h), dtype=torch.uint8, device="cuda")

    arr = rng.normal(size=(h, w))
    a = torch.from_numpy(arr).cuda()
    rows = torch.full((total + 1, 3), -7.0, dtype=torch.float64, device="cuda")
    assert lib.camd_arr2d_to_uvzs_masked(a.data_ptr(), m.data_ptr(), w, h, 0, rows.data_ptr(), total - 1, count.data_ptr(),
                                         ws.data_ptr(), st) == 0
    assert int(count.item()) == total
    assert np.array_equal(_np(rows[:total - 1]), sparse_ref.rows_of(arr, mask)[:total - 1])
    assert (_np(rows[total - 1:]) == -7.0).all()

    flow = rng.normal(0, 3, (h, w, 2))
    f = torch.from_numpy(flow).cuda()
    out = torch.full((2, total + 1, 2), -7.0, dtype=torch.float64, device="cuda")
    count.zero_()
    assert lib.camd_flow_to_matched_uvs(f.data_ptr(), _native.VALUE_F64, m.data_ptr(), w, h, out[0].data_ptr(),
                                        out[1].data_ptr(), total - 1, count.data_ptr(), ws.data_ptr(), st) == 0
    assert int(count.item()) == total
    ys, xs = np.nonzero(mask)
    want_from = np.stack([xs + 0.5 - 1e-8, ys + 0.5 - 1e-8], 1)
    assert np.array_equal(_np(out[0, :total - 1]), want_from[:total - 1])
    assert np.array_equal(_np(out[1, :total - 1]), (flow[ys, xs] + want_from)[:total - 1])
    assert (_np(out[:, total - 1:]) == -7.0).all()
