"""A calibrated recording as a NeRF ``transforms.json`` (the reference's calibrating/reconstruction_with_board.py).

``convert_cam_to_nerf_json`` is host bookkeeping over the camera's intrinsics and per-frame poses; the one measurement in
it, a frame's sharpness -- ``cv2.Laplacian(gray, cv2.CV_64F).var()`` -- runs on the GPU (``imgproc.sharpness``;
csrc/sharpness.hip).  DEVIATION: the reference reads every frame's picture from ``d["path"]`` to measure it; images are not
read from paths here, so a frame's ``sharpness`` comes from ``d["img"]`` where the record holds an image and the key is
left out where it does not.
"""
import json
import os

import numpy as np

COORDINATE_TYPES = ("opencv", "nerf")
CV_TO_NERF = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]])  # instant-ngp's colmap2nerf.py


def get_sharpness(image):
    """reconstruction_with_board.py:9-12: the variance of the Laplacian of the picture's gray image, on the GPU"""
    from . import imgproc
    return imgproc.sharpness(image)


def _plain(value):
    if isinstance(value, dict):
        return {k: _plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    if isinstance(value, np.ndarray):
        return value.tolist()
    return value.item() if isinstance(value, np.generic) else value


def convert_cam_to_nerf_json(cam, json_path=None, target_scale=None, aabb_scale=4, sharpness=True, basename=False,
                             rotate_z_as_up=True, coordinate_type="nerf"):
    """reconstruction_with_board.py:15-77: the dictionary instant-ngp reads -- ``fl_x, fl_y, cx, cy, w, h, camera_angle_x,
    camera_angle_y`` (radians), ``coordinate_type``, ``k1, k2, p1, p2`` and ``frames``: for every record with a pose
    ``file_path`` (``d["path"]``, its basename with ``basename``; the record's key where it has no path),
    ``transform_matrix`` = ``d["T_cam_in_world"]`` or the inverse of ``d["T"]`` -- with "nerf" times diag(1, -1, -1, 1) and,
    with ``rotate_z_as_up``, a half turn about x from the left -- and ``sharpness`` where the record holds ``d["img"]``.
    ``target_scale``: the translations are scaled so that their mean norm is that many units (the reference recommends
    1 .. 5, 2 for metres).  ``aabb_scale`` is accepted and, as in the reference, not written.  Returns the dictionary, or
    with ``json_path`` writes it there (matrices as lists, indent 1) and returns the path."""
    from . import geometry
    assert coordinate_type in COORDINATE_TYPES
    nerf_json = dict(fl_x=cam.fx, fl_y=cam.fy, cx=cam.cx, cy=cam.cy, w=cam.xy[0], h=cam.xy[1],
                     camera_angle_x=cam.fovs["fovx"] * np.pi / 180, camera_angle_y=cam.fovs["fovy"] * np.pi / 180,
                     coordinate_type=coordinate_type)
    nerf_json.update(zip("k1 k2 p1 p2".split(), np.asarray(cam.D).reshape(1, -1)[0, :4]))
    nerf_json["frames"] = []
    for key, d in cam.items():
        if "T" not in d:
            continue
        T_cam_in_world = d["T_cam_in_world"] if "T_cam_in_world" in d else np.linalg.inv(d["T"])
        if coordinate_type == "nerf":
            T_cam_in_world = T_cam_in_world @ CV_TO_NERF
            if rotate_z_as_up:
                T_cam_in_world = geometry.R_t_to_T([np.pi, 0, 0]) @ T_cam_in_world
        path = d.get("path", key)
        dic = dict(file_path=os.path.basename(path) if basename and isinstance(path, str) else path,
                   transform_matrix=np.array(T_cam_in_world, np.float64))
        if sharpness and d.get("img") is not None and not isinstance(d["img"], str):
            dic["sharpness"] = get_sharpness(d["img"])
        nerf_json["frames"].append(dic)
    if target_scale is not None:
        mean_t = np.mean([np.linalg.norm(d["transform_matrix"][:3, 3]) for d in nerf_json["frames"]])
        for d in nerf_json["frames"]:
            d["transform_matrix"][:3, 3] *= target_scale / mean_t
    if json_path is None:
        return nerf_json
    with open(json_path, "w") as f:
        json.dump(_plain(nerf_json), f, indent=1)
    return json_path
