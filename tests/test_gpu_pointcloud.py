"""n4: depth post-ops (point cloud <-> depth, camera-to-camera re-projection) against the NumPy oracle, whose matrix
products are NumPy's BLAS (tolerances and shares), and beside each such comparison bit for bit against the exact C oracle
oracle/pointcloud_ref.c (-m gpu)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import pointcloud  # noqa: E402
from oracle import pointcloud_ref as ref  # noqa: E402


def _scene_depth(seed, h, w, holes=0.2):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    z = 1.5 + 0.5 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 0.3 * (xx > w // 2)
    z[rng.random((h, w)) < holes] = 0
    return z


K = np.array([[420.0, 0, 161.3], [0, 424.0, 118.9], [0, 0, 1]])


@pytest.mark.parametrize("rate", [1, 1.5, 2, 0.75, 1.37])
def test_depth_to_point_cloud(rate, oracle):
    depth = _scene_depth(1, 240, 320)
    got = pointcloud.depth_to_point_cloud(depth, K, interpolation_rate=rate, return_xyzuv=True)
    want = ref.depth_to_point_cloud(depth, K, interpolation_rate=rate, return_xyzuv=True)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got[:, 3:], want[:, 3:])                      # same pixels in the same order
    assert np.allclose(got[:, :3], want[:, :3], rtol=1e-13, atol=1e-13)   # BLAS vs left-to-right products
    assert got.tobytes() == oracle.depth_to_point_cloud(depth, K, rate, return_xyzuv=True).tobytes()   # the exact chain
    pts = pointcloud.depth_to_point_cloud(depth, K, interpolation_rate=rate)
    assert np.array_equal(pts, got[:, :3])


def test_depth_to_point_cloud_edge_cases(oracle):
    assert pointcloud.depth_to_point_cloud(np.zeros((7, 9)), K).shape == (0, 3)
    full = np.full((5, 300), 2.0)                                       # rows wider than one workgroup pass
    got = pointcloud.depth_to_point_cloud(full, K)
    assert np.allclose(got, ref.depth_to_point_cloud(full, K), rtol=1e-13)
    assert got.tobytes() == oracle.depth_to_point_cloud(full, K).tobytes()
    mm = (np.arange(12, dtype=np.uint16).reshape(3, 4) * 250)
    assert np.allclose(pointcloud.depth_to_point_cloud(mm, K), ref.depth_to_point_cloud(mm, K), rtol=1e-13)
    assert pointcloud.depth_to_point_cloud(mm, K).tobytes() == oracle.depth_to_point_cloud(mm, K).tobytes()
    t = torch.from_numpy(full).cuda()
    assert pointcloud.depth_to_point_cloud(t, K).is_cuda


def test_apply_T_and_point_cloud_to_depth_roundtrip(oracle):
    depth = _scene_depth(2, 240, 320)
    cloud = ref.depth_to_point_cloud(depth, K)
    T = np.eye(4)
    T[:3, :3] = ca.geometry.rodrigues(np.array([0.02, -0.05, 0.01]))
    T[:3, 3] = [0.06, -0.01, 0.02]
    moved = pointcloud.apply_T_to_point_cloud(T, cloud)
    assert np.allclose(moved, ref.apply_T_to_point_cloud(T, cloud), rtol=1e-13, atol=1e-15)
    assert moved.tobytes() == oracle.apply_T_to_point_cloud(T, cloud).tobytes()
    extra = np.concatenate([cloud, np.arange(len(cloud))[:, None] * 1.0], 1)
    assert np.array_equal(pointcloud.apply_T_to_point_cloud(T, extra)[:, 3], extra[:, 3])
    # identity round trip: depth -> cloud -> depth reproduces the image exactly
    back = pointcloud.point_cloud_to_depth(cloud, K, (320, 240))
    assert np.allclose(back, depth, rtol=1e-12, atol=0)
    assert back.tobytes() == oracle.point_cloud_to_depth(cloud, K, (320, 240)).tobytes()
    # z-buffer against the reference's far-to-near overwrite (moved cloud: many pixels receive several points)
    got = pointcloud.point_cloud_to_depth(ref.apply_T_to_point_cloud(T, cloud), K, (320, 240))
    want = ref.point_cloud_to_depth(ref.apply_T_to_point_cloud(T, cloud), K, (320, 240))
    assert (got != 0).sum() == (want != 0).sum()
    assert np.array_equal(got, want)
    assert got.tobytes() == oracle.point_cloud_to_depth(ref.apply_T_to_point_cloud(T, cloud), K, (320, 240)).tobytes()


def test_point_cloud_to_depth_behind_camera_and_outside(oracle):
    pts = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 1.0], [0.0, 0.0, -3.0],      # same pixel: the negative z "wins"
                    [50.0, 0.0, 1.0], [0.1, 0.1, 0.0], [0.2, -0.1, 4.0]])   # outside / z = 0 / ordinary
    got = pointcloud.point_cloud_to_depth(pts, K, (320, 240), bg_value=-1)
    want = ref.point_cloud_to_depth(pts[[0, 1, 2, 3, 5]], K, (320, 240), bg_value=-1)  # z = 0 divides by zero there
    assert np.array_equal(got, want)
    assert got.tobytes() == oracle.point_cloud_to_depth(pts, K, (320, 240), bg_value=-1).tobytes()   # z = 0 included
    assert pointcloud.point_cloud_to_depth(np.zeros((0, 3)), K, (8, 6)).sum() == 0


@pytest.mark.parametrize("interpolation", [1.5, 1, 0])
def test_project_cam2_depth(interpolation, oracle):
    cam1 = ca.Cam.init_by_K_D(K, None, (320, 240))
    K2 = np.array([[380.0, 0, 150.0], [0, 380.0, 110.0], [0, 0, 1]])
    cam2 = ca.Cam.init_by_K_D(K2, None, (300, 220))
    depth2 = _scene_depth(3, 220, 300)
    T = np.eye(4)
    T[:3, :3] = ca.geometry.rodrigues(np.array([0.01, 0.03, -0.02]))
    T[:3, 3] = [-0.05, 0.0, 0.01]
    got = cam1.project_cam2_depth(cam2, depth2, T=T, interpolation=interpolation)
    want = ref.project_cam2_depth(K, (320, 240), K2, depth2, T, interpolation=interpolation)
    assert got.shape == (240, 320)
    same = np.isclose(got, want, rtol=1e-12, atol=1e-12)
    assert same.mean() > 0.9999, same.mean()       # NumPy's BLAS is the machine's: a share, for this comparison alone
    assert ((got != 0) == (want != 0)).mean() > 0.9999
    rate = pointcloud.get_appropriate_interpolation_rate(cam1, cam2, interpolation)
    assert got.tobytes() == oracle.project_depth(depth2, K2, T, K, (320, 240), rate).tobytes()   # every pixel
    with pytest.raises(NotImplementedError):
        cam1.project_cam2_depth(cam2, depth2)
