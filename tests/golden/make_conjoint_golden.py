#!/usr/bin/env python3
"""Runs the REFERENCE's own ``Stereo.get_conjoint_points`` (stereo_camera.py:55-93) on small detections and writes
tests/golden/reference_conjoint.npz.

BUILD CONTAINER ONLY (it needs the reference, which does not travel to the GPU box; only the .npz does).
    python tests/golden/make_conjoint_golden.py

The reference is imported from where it lies, unmodified, with the stand-ins of make_reference_golden.py for its two
missing dependencies (cv2, boxx); none of them is reached by this method.  Two fixtures: ``arrays`` (checkerboard
detections, (n, 2) arrays per key) and ``markers`` (id -> points dicts per key).  Camera 2 lacks a key, holds a key
camera 1 lacks, holds an empty detection, and -- markers -- misses ids and shares none in one key.  Stored: the inputs and,
per fixture, the three lists the reference returns."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_reference_golden as mrg  # noqa: E402

FIXTURE = os.path.join(HERE, "reference_conjoint.npz")


def detections():
    """name -> (frames of camera 1, frames of camera 2): key -> dict(image_points, object_points)"""
    rng = np.random.default_rng(20251019)
    pts = lambda n, w: rng.uniform(0, 100, (n, w)).round(3)  # noqa: E731
    a1, a2 = {}, {}
    for key, n in (("c", 6), ("a", 4), ("b", 5), ("d", 4)):
        obj = pts(n, 3)
        a1[key] = dict(image_points=pts(n, 2), object_points=obj)
        a2[key] = dict(image_points=pts(n, 2), object_points=obj)
    del a2["b"]                                                                # camera 2 did not take this picture
    a2["e"] = dict(image_points=pts(4, 2), object_points=pts(4, 3))            # camera 1 did not take this one
    a2["d"] = dict(image_points=np.zeros((0, 2)), object_points=pts(4, 3))     # taken, nothing detected
    a1["f"] = dict(path="f.png")                                               # no detection at all
    m1, m2 = {}, {}
    for key, ids in (("k2", (7, 3, 5)), ("k1", (3, 9)), ("k3", (1, 2)), ("k4", (4,))):
        obj = {i: pts(4, 3) for i in ids}
        m1[key] = dict(image_points={i: pts(4, 2) for i in ids}, object_points=obj)
        m2[key] = dict(image_points={i: pts(4, 2) for i in ids[::-1]}, object_points=obj)
    del m2["k2"]["image_points"][3]        # an id camera 2 missed
    m2["k1"]["image_points"][8] = pts(4, 2)  # an id only camera 2 saw
    m2["k3"]["image_points"] = {6: pts(4, 2)}  # no common id: the key drops out
    del m2["k4"]                           # camera 2 did not take this picture
    return dict(arrays=(a1, a2), markers=(m1, m2))


def flatten(out, prefix, frames):
    """store one camera's frames: <prefix>/keys, and per key its points (markers: <key>/ids and one array per id)"""
    out[prefix + "/keys"] = np.array(list(frames))
    for key, d in frames.items():
        for what in ("image_points", "object_points"):
            if what not in d:
                continue
            v = d[what]
            if isinstance(v, dict):
                out["%s/%s/%s/ids" % (prefix, key, what)] = np.array(list(v), np.int64)
                for i, a in v.items():
                    out["%s/%s/%s/%d" % (prefix, key, what, i)] = a
            else:
                out["%s/%s/%s" % (prefix, key, what)] = v


def main():
    cal = mrg.import_reference()
    out = {}
    for name, (f1, f2) in detections().items():
        cam1, cam2 = cal.Cam.__new__(cal.Cam), cal.Cam.__new__(cal.Cam)
        cam1.update(f1), cam2.update(f2)
        st = cal.Stereo()
        st.cam1, st.cam2 = cam1, cam2
        res = st.get_conjoint_points()
        flatten(out, name + "/cam1", f1), flatten(out, name + "/cam2", f2)
        out[name + "/frames"] = np.array(len(res[0]))
        for which, arrays in zip(("image_points1", "image_points2", "object_points"), res):
            for i, a in enumerate(arrays):
                out["%s/out/%s/%d" % (name, which, i)] = np.asarray(a)
        print("%s: %d conjoint frames, %s points" % (name, len(res[0]), [len(a) for a in res[0]]))
    np.savez_compressed(FIXTURE, **out)
    print("wrote %s (%d bytes, %d arrays)" % (os.path.basename(FIXTURE), os.path.getsize(FIXTURE), len(out)))


if __name__ == "__main__":
    main()
