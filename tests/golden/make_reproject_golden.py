#!/usr/bin/env python3
"""Runs the REFERENCE's own ``utils.point_cloud_to_arr2d``, ``utils.get_reproject_remap`` and the ``cv2.remap(img2, mapx,
mapy, cv2.INTER_LINEAR)`` step of ``Cam.vis_reproject_img_alignment`` and writes tests/golden/reference_reproject.npz.

BUILD CONTAINER ONLY (it needs the reference checkout next to this repository; only the .npz travels).
    python tests/golden/make_reproject_golden.py

What is executed.  The reference package is imported from where it lies, unmodified, through
``make_reference_golden.import_reference`` (that file is used as it is, with its oracle-backed stand-ins for cv2 / boxx),
and its own code runs on the inputs of tests/reproject_cases.py:
    utils.get_reproject_remap(K1, K2, T_2in1, depth2, xy1, rate)     utils.py:332-344   rotated rig, rates 1 and 1.5
    cv2.remap(img2, mapx, mapy, cv2.INTER_LINEAR)                    camera.py:341      gray and RGB, on those maps
    utils.point_cloud_to_arr2d(points, K1, xy1, values, bg_value)    utils.py:254-317   a coloured cloud (uint8 x 3, bg 7)

WHAT THIS PINS AND WHAT IT DOES NOT.  It pins the reference's own NumPy: the far-to-near order, the float32 hand-over of
(u, v), np.round's half-to-even, the scatter's last-write-wins, the -1 background and the (2, h, w) layout.  On these
inputs no two points share a pixel and a bit-equal z (tests/test_reproject_cpu.py), so NumPy's unstable default sort
cannot have decided anything.  It does NOT pin cv2's arithmetic: cv2.resize(INTER_NEAREST) and cv2.remap are the
oracle's restatements.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_reference_golden as mrg  # noqa: E402  (imported, not edited)
import reproject_cases as cases  # noqa: E402


def main():
    import oracle
    oracle.build()
    cal = mrg.import_reference()
    cv2 = sys.modules["cv2"]
    u = cal.utils
    out = {"reference_version": np.array(cal.__version__)}
    d2, T = cases.depth2(), cases.pose()
    gray, rgb = cases.image(1, cn=1), cases.image(2, cn=3)
    for rate in cases.GOLDEN_RATES:
        maps = u.get_reproject_remap(cases.K1, cases.K2, T, d2, cases.XY1, interpolation_rate=rate)
        assert maps.dtype == np.float32 and maps.shape == (2,) + cases.XY1[::-1]
        mapx, mapy = maps
        out["remap_rate%s" % rate] = maps
        out["gray_rate%s" % rate] = cv2.remap(gray, mapx, mapy, cv2.INTER_LINEAR)
        out["rgb_rate%s" % rate] = cv2.remap(rgb, mapx, mapy, cv2.INTER_LINEAR)
        print("rate %-4s  %d of %d target pixels hit" % (rate, (mapx >= 0).sum(), mapx.size))
    cloud, colours = cases.coloured_cloud()
    out["coloured"] = u.point_cloud_to_arr2d(cloud, cases.K1, cases.XY1, values=colours, bg_value=7)
    assert out["coloured"].dtype == np.uint8 and out["coloured"].shape == cases.XY1[::-1] + (3,)
    np.savez_compressed(cases.FIXTURE, **out)
    print("wrote %s (%d KB, %d arrays)" % (os.path.relpath(cases.FIXTURE, ROOT), os.path.getsize(cases.FIXTURE) // 1024, len(out)))


if __name__ == "__main__":
    main()
