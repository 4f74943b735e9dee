"""CPU restatement of the payload half of the depth post-ops -- TEST INFRASTRUCTURE ONLY.

NumPy restatement of the reference's own NumPy code: utils.point_cloud_to_arr2d (utils.py:254-288) with its scatter
uvzs_to_arr2d (:291-317), utils.get_reproject_remap (:332-344), and the cv2.remap(img2, mapx, mapy, cv2.INTER_LINEAR)
that follows it in Cam.vis_reproject_img_alignment (camera.py:322-342; cv2.remap through the oracle's restatement).

``kind`` is the sort np.argsort uses for the far-to-near order: None is the reference's literal call (NumPy's default,
introsort, NOT stable); "stable" defines what happens to points that share a pixel and a bit-equal z -- the later one
wins -- which is the rule the library implements.
"""
import numpy as np

from oracle import pointcloud_ref


def _project(points, K):
    proj = points[:, :3] @ K.T
    proj[:, :2] /= proj[:, 2:]
    return proj


def point_cloud_to_arr2d(points, K, xy, values=None, bg_value=0, kind=None):
    proj = _project(points, K)
    order = np.argsort(-proj[:, 2], kind=kind)
    far_first = proj[order]
    if values is None:
        uv, payload = far_first[:, :2], far_first[:, 2:]
    else:
        uv, payload = far_first, values[order]
    if payload.ndim == 1:
        payload = payload[:, None]
    shape = (xy[1], xy[0]) + ((payload.shape[1],) if payload.shape[1] >= 2 else ())
    img = np.ones(shape, payload.dtype) * bg_value
    xs, ys = np.int32(uv[:, :2].round()).T
    ok = (xs >= 0) & (xs < xy[0]) & (ys >= 0) & (ys < xy[1])
    img[ys[ok], xs[ok]] = payload[ok] if payload.shape[1] >= 2 else payload[ok][:, 0]
    return img


def _cloud_in_cam1(K2, T_2in1, depth2, interpolation_rate):
    xyzuv = pointcloud_ref.depth_to_point_cloud(depth2, K2, interpolation_rate=interpolation_rate, return_xyzuv=True)
    return pointcloud_ref.apply_T_to_point_cloud(T_2in1, xyzuv[:, :3]), np.float32(xyzuv[:, 3:])


def get_reproject_remap(K1, K2, T_2in1, depth2, xy1, interpolation_rate=1, kind=None):
    cloud1, uv = _cloud_in_cam1(K2, T_2in1, depth2, interpolation_rate)
    return point_cloud_to_arr2d(cloud1, K1, xy1, values=uv, bg_value=-1, kind=kind).transpose(2, 0, 1)


def reproject_img(img2, mapx, mapy):
    import oracle
    return oracle.remap_u8(img2, np.ascontiguousarray(mapx), np.ascontiguousarray(mapy), interp=oracle.INTER_LINEAR)


def reproject_stats(K1, K2, T_2in1, depth2, xy1, interpolation_rate=1):
    """(target pixels hit, points that share their pixel AND their bit pattern of z with an earlier point)."""
    cloud1, _ = _cloud_in_cam1(K2, T_2in1, depth2, interpolation_rate)
    proj = _project(cloud1, K1)
    xs, ys = np.int32(proj[:, :2].round()).T
    ok = (xs >= 0) & (xs < xy1[0]) & (ys >= 0) & (ys < xy1[1])
    pix = ys[ok].astype(np.int64) * xy1[0] + xs[ok]
    pairs = np.stack([pix, proj[ok, 2].view(np.int64)], 1)
    return len(np.unique(pix)), len(pairs) - len(np.unique(pairs, axis=0))
