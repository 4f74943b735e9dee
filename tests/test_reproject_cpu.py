"""The re-projection feature without a GPU: the condition under which the GPU's tie rule may be compared with the
reference's literal (unstable) sort, the input on which the reference disagrees with itself, the restatement against
what the reference's own Python produced, and the errors the Python front ends raise before any device call."""
import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import pointcloud

import reproject_cases as cases
import reproject_ref as ref


@pytest.mark.parametrize("rate", cases.PRECONDITION_RATES)
def test_rotated_rig_has_no_ties_and_both_sort_kinds_agree(rate):
    """Precondition of tests/test_gpu_reproject.py: on the rotated rig no two points share a pixel and a bit-equal z, so
    np.argsort's default (introsort) and a stable sort give the same map, and "the larger index wins" decides nothing."""
    d2, T = cases.depth2(), cases.pose()
    hit, ties = ref.reproject_stats(cases.K1, cases.K2, T, d2, cases.XY1, rate)
    assert ties == 0 and hit > 49000
    default = ref.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, rate)
    stable = ref.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, rate, kind="stable")
    assert default.dtype == np.float32 and default.shape == (2, 240, 320)
    assert np.array_equal(default, stable)
    assert ((default[0] >= 0).sum()) == hit and (default[default < 0] == -1).all()


def test_identity_rotation_at_rate_1_5_makes_the_reference_disagree_with_itself():
    """Why the tie rule exists: with R = I the replicated cells of the nearest-neighbour up-sampling share z bit for
    bit, and the winner of np.argsort(-z) depends on the sort kind."""
    d2, T = cases.depth2(), cases.pose(rotated=False)
    _, ties = ref.reproject_stats(cases.K1, cases.K2, T, d2, cases.XY1, 1.5)
    assert ties > 10000
    default = ref.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, 1.5)
    stable = ref.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, 1.5, kind="stable")
    differ = (default != stable).any(0)
    assert differ.sum() > 1000
    assert np.array_equal(default < 0, stable < 0)  # the hit mask is not in question, only who wins
    # at rate 1 there are no replicated cells and no ties
    assert ref.reproject_stats(cases.K1, cases.K2, T, d2, cases.XY1, 1)[1] == 0


def test_restatement_equals_the_reference_run():
    fx = cases.load_fixture()
    assert fx is not None, "tests/golden/reference_reproject.npz is missing"
    d2, T = cases.depth2(), cases.pose()
    gray, rgb = cases.image(1, cn=1), cases.image(2, cn=3)
    for rate in cases.GOLDEN_RATES:
        maps = ref.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, rate)
        want = fx["remap_rate%s" % rate]
        assert maps.dtype == want.dtype and np.array_equal(maps, want)
        assert np.array_equal(ref.reproject_img(gray, *maps), fx["gray_rate%s" % rate])
        assert np.array_equal(ref.reproject_img(rgb, *maps), fx["rgb_rate%s" % rate])
    cloud, colours = cases.coloured_cloud()
    got = ref.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=colours, bg_value=7)
    assert got.dtype == np.uint8 and np.array_equal(got, fx["coloured"])
    # values=None is the depth image of the oracle
    from oracle import pointcloud_ref
    assert np.array_equal(ref.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1),
                          pointcloud_ref.point_cloud_to_depth(cloud, cases.K1, cases.XY1))


def test_errors_are_raised_before_any_device_call():
    """Shapes, dtypes and devices are checked on the arguments themselves: the same errors with and without a GPU."""
    K, T = cases.K1, cases.pose()
    pts, d2 = np.zeros((4, 3)), np.ones((6, 8))
    bad_arr2d = [
        dict(points=np.zeros((4, 2)), values=np.zeros(4)),                 # points (N, < 3)
        dict(points=np.zeros(12), values=np.zeros(4)),                     # points not 2-D
        dict(points=pts, values=np.zeros(5)),                              # N mismatch
        dict(points=pts, values=np.zeros((4, 2, 2))),                      # values 3-D
        dict(points=pts, values=np.zeros((4, 0))),                         # no channel
        dict(points=pts, values=np.zeros(4, np.int32)),                    # dtype
        dict(points=pts, values=np.zeros(4, np.float16)),
        dict(points=pts, values=np.zeros(4, np.uint8), bg_value=-1),       # background not a uint8
        dict(points=pts, values=np.zeros(4, np.uint8), bg_value=2.5),
        dict(points=pts, values=np.zeros(4), xy=(0, 6)),                   # empty image
    ]
    for kw in bad_arr2d:
        kw.setdefault("xy", (8, 6))
        with pytest.raises(ValueError):
            pointcloud.point_cloud_to_arr2d(K=K, **kw)
    with pytest.raises(TypeError):
        pointcloud.point_cloud_to_arr2d([[0, 0, 1]], K, (8, 6), values=np.zeros(1))
    for bad_depth in (np.ones(8), np.ones((2, 2, 6, 8)), np.ones((6, 8), np.int32), np.ones((0, 8))):
        with pytest.raises(ValueError):
            pointcloud.get_reproject_remap(K, K, T, bad_depth, (8, 6))
    for kw in (dict(xy1=(8, 0)), dict(xy1=(8, 6), interpolation_rate=0), dict(xy1=(8, 6), interpolation_rate=float("nan")),
               dict(xy1=(8, 6), T_2in1=np.eye(3)), dict(xy1=(8, 6), K1=np.eye(2))):
        args = dict(K1=K, K2=K, T_2in1=T, depth2=d2)
        args.update(kw)
        with pytest.raises(ValueError):
            pointcloud.get_reproject_remap(**args)
    for bad_img in (np.zeros((6, 8), np.float32), np.zeros((6, 9), np.uint8), np.zeros((6, 8, 4), np.uint8),
                    np.zeros((2, 6, 8), np.uint8)):
        with pytest.raises(ValueError):
            pointcloud.reproject_img(bad_img, d2, K, T, K, (8, 6))
    with pytest.raises(ValueError):   # a batch of depths needs a batch of images
        pointcloud.reproject_img(np.zeros((6, 8, 3), np.uint8), np.ones((3, 6, 8)), K, T, K, (8, 6))
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="GPU"):   # a CPU tensor is not silently moved
        pointcloud.get_reproject_remap(K, K, T, torch.ones((6, 8), dtype=torch.float64), (8, 6))
    with pytest.raises(ValueError, match="GPU"):
        pointcloud.point_cloud_to_arr2d(torch.zeros((4, 3), dtype=torch.float64), K, (8, 6), values=np.zeros(4))


def test_cam_reproject_img_refuses_what_the_reference_cannot_do_here():
    cam1 = ca.Cam.init_by_K_D(cases.K1, None, cases.XY1)
    cam2 = ca.Cam.init_by_K_D(cases.K2, None, cases.XY2)
    d2, img = cases.depth2(), cases.image(1)
    with pytest.raises(NotImplementedError, match="pass T"):
        cam1.reproject_img(cam2, d2, img)
    bent = ca.Cam.init_by_K_D(cases.K2, [[-0.1, 0.01, 0, 0, 0]], cases.XY2)
    with pytest.raises(AssertionError, match="cam2.D has distort"):
        cam1.reproject_img(bent, d2, img, T=cases.pose())
    with pytest.raises(ValueError):   # the image does not belong to the depth
        cam1.reproject_img(cam2, d2, img[:-1], T=cases.pose())
