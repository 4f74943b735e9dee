#!/usr/bin/env python3
"""Runs the REFERENCE's own Python on the pose bookkeeping around PnP and writes tests/golden/reference_pose.npz.

BUILD CONTAINER ONLY (it needs the reference's checkout, which does not travel to the GPU box; only the .npz does).
    python tests/golden/make_pose_golden.py

What is executed, from where it lies and unmodified, with the stand-in modules of make_reference_golden.py:
    utils.mean_Ts(Ts)                       utils.py:418-432   (the accumulation order of R_acc, R_t_to_T's float32 rounding)
    Cam.valid_keys / valid_keys_intersection / get_T_cam2_in_self    camera.py:148-149, 289-296, 371-372
    utils.convert_points_for_cv2            utils.py:132-136
``cv2.Rodrigues`` is this project's ``geometry.rodrigues`` here (both directions): what the fixture pins is every line of the
reference's own Python around it, not cv2's arithmetic.  The fixture holds only data: the input
poses and points, and the matrices and key lists the reference returned.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_reference_golden as mrg  # noqa: E402
from calibrating_amd import geometry  # noqa: E402

FIXTURE = os.path.join(HERE, "reference_pose.npz")
K = np.array([[1000.0, 0, 640], [0, 1000.0, 360], [0, 0, 1]])
XY = (1280, 720)


def pose_sets():
    """name -> (m, 4, 4) float64: what mean_Ts has to average"""
    rng = np.random.default_rng(20260)
    out = {}
    for name, m, spread in (("one", 1, 0.0), ("tight", 5, 1e-3), ("loose", 7, 0.2), ("pair", 2, 0.05)):
        base = np.eye(4)
        base[:3, :3] = geometry.rodrigues(rng.uniform(-1, 1, 3))
        base[:3, 3] = rng.uniform(-0.5, 0.5, 3)
        Ts = []
        for _ in range(m):
            T = np.eye(4)
            T[:3, :3] = geometry.rodrigues(rng.uniform(-1, 1, 3) * spread) @ base[:3, :3]
            T[:3, 3] = base[:3, 3] + rng.uniform(-1, 1, 3) * spread
            Ts.append(T)
        out[name] = np.stack(Ts)
    return out


def camera_records():
    """Two cameras' frame records: key -> (has image points, pose); some keys in one camera only, one without points"""
    rng = np.random.default_rng(20261)
    rig = np.eye(4)
    rig[:3, :3] = geometry.rodrigues(np.array([0.02, -0.3, 0.01]))
    rig[:3, 3] = [-0.12, 0.003, 0.01]
    keys1, keys2 = ["f00", "f01", "f02", "f03", "f05"], ["f01", "f02", "f03", "f04", "f05"]
    T2 = {}
    for k in sorted(set(keys1 + keys2)):
        T = np.eye(4)
        T[:3, :3] = geometry.rodrigues(rng.uniform(-0.4, 0.4, 3))
        T[:3, 3] = [rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 1.5)]
        T2[k] = T
    noise = lambda: np.concatenate([np.concatenate([geometry.rodrigues(rng.uniform(-1e-3, 1e-3, 3)), rng.uniform(-1e-3, 1e-3, (3, 1))], 1),  # noqa: E731
                                    [[0, 0, 0, 1]]])
    T1 = {k: rig @ noise() @ T2[k] for k in T2}
    return keys1, keys2, T1, T2, "f03"  # f03: no image points in camera 2


def main():
    cal = mrg.import_reference()
    sys.modules["cv2"].Rodrigues = lambda src: (geometry.rodrigues(np.asarray(src, np.float64)), None)
    out = {"reference_version": np.array(cal.__version__)}
    for name, Ts in pose_sets().items():
        out["mean/%s/Ts" % name] = Ts
        out["mean/%s/T" % name] = np.asarray(cal.utils.mean_Ts(list(Ts)), np.float64)
    keys1, keys2, T1, T2, empty = camera_records()
    cam1 = cal.Cam.init_by_K_D(K, np.zeros((1, 5)), XY, name="a")
    cam2 = cal.Cam.init_by_K_D(K, np.zeros((1, 5)), XY, name="b")
    pts = np.array([[10.0, 20.0], [30.0, 40.0]])
    for k in keys1:
        cam1[k] = dict(image_points=pts, T=T1[k])
    for k in keys2:
        cam2[k] = dict(image_points={} if k == empty else {3: pts[:1], 1: pts[1:]}, T=T2[k])
    out["rig/keys1"], out["rig/keys2"], out["rig/empty"] = np.array(keys1), np.array(keys2), np.array(empty)
    out["rig/T1"] = np.stack([T1[k] for k in keys1])
    out["rig/T2"] = np.stack([T2[k] for k in keys2])
    out["rig/valid1"] = np.array(sorted(cam1.valid_keys))
    out["rig/valid2"] = np.array(sorted(cam2.valid_keys))
    out["rig/intersection"] = np.array(cam1.valid_keys_intersection(cam2))
    out["rig/T_cam2_in_cam1"] = np.asarray(cam1.get_T_cam2_in_self(cam2), np.float64)
    joined = {5: np.arange(6.0).reshape(3, 2), 2: np.arange(6.0, 10.0).reshape(2, 2), 11: np.arange(10.0, 12.0).reshape(1, 2)}
    out["join/keys"] = np.array(sorted(joined))
    for k, v in joined.items():
        out["join/in_%d" % k] = v
    out["join/out"] = cal.utils.convert_points_for_cv2(joined)
    np.savez_compressed(FIXTURE, **out)
    print("wrote %s (%d bytes, %d arrays)" % (os.path.relpath(FIXTURE, ROOT), os.path.getsize(FIXTURE), len(out)))


if __name__ == "__main__":
    main()
