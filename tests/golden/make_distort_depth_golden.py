#!/usr/bin/env python3
"""Runs the REFERENCE's own ``Stereo.distort_depth`` and ``get_depth(return_distort_depth=True)`` and writes
tests/golden/reference_distort_depth.npz.

BUILD CONTAINER ONLY (it needs the reference checkout next to this repository; only the .npz travels).
    python tests/golden/make_distort_depth_golden.py

What is executed.  The reference package is imported from where it lies, unmodified, through
``make_reference_golden.import_reference`` (that file is used as it is), and its own code runs
    Stereo.load(record)                                         for every rig of tests/distort_depth_cases.RIGS
    Stereo.distort_depth(depth)                 :433-464        float64 and float32 depth images, and an index probe
                                                                (depth[i] = i + 1) from which the source-index table is read
    Stereo.set_stereo_matching(SemiGlobalBlockMatching(cfg), max_depth) ; get_depth(img1, img2, return_distort_depth=True)
                                                :492-533        on the barrel rig

What stands in for cv2.  On top of ``make_reference_golden.install_stand_ins`` three more entry points of the stand-in
``cv2`` module are filled, the three ``distort_depth`` calls: cv2.undistortPoints, cv2.convertPointsToHomogeneous and
cv2.projectPoints, backed by tests/distort_depth_ref.py (a restatement of OpenCV 4.x calib3d).

WHAT THIS PINS AND WHAT IT DOES NOT.  It pins what the reference owns between and after those calls: the row-major pixel
order of its meshgrid, the float32 hand-overs, ``.astype(np.int32)`` truncation, np.unique's first-index-wins and its
fancy-index scatter, zeros where nobody lands, the result's dtype, the IndexError of a rig whose targets leave the
image, and the result keys of ``get_depth(return_distort_depth=True)`` (``distort_img1`` being the argument itself).  It
does NOT pin cv2's arithmetic: behind the three entry points sits the same restatement the other tests use (DESIGN.md
section 2, U21 / U22).
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
import reference_cases as rc  # noqa: E402
import distort_depth_cases as dc  # noqa: E402
import distort_depth_ref as ref  # noqa: E402


def import_reference():
    cal = mrg.import_reference()
    cv2 = sys.modules["cv2"]
    cv2.undistortPoints = ref.undistort_points
    cv2.convertPointsToHomogeneous = ref.convert_points_to_homogeneous
    cv2.projectPoints = ref.project_points
    return cal


def run_rig(cal, name, out):
    st = cal.Stereo().load(dc.rig_record(name, spelled=True))
    K, D, (w, h) = dc.camera(name)
    assert np.array_equal(st.cam1.K, K) and np.array_equal(np.ravel(st.cam1.D), D) and tuple(st.cam1.xy) == (w, h)
    if name == dc.OUT_RIG:
        try:
            st.distort_depth(dc.depth_input(name, np.float64))
            raised = "none"
        except IndexError as e:
            raised = "IndexError: %s" % e
        out[name + "/raised"] = np.array(raised)
        print("%-16s %dx%d  the reference raised %s" % (name, w, h, raised))
        return
    probe = st.distort_depth(dc.index_probe(name))
    assert probe.dtype == np.float64
    out[name + "/src_index"] = (probe - 1).astype(np.int32)  # exact: integers below 2^53
    for dtype in (np.float64, np.float32):
        res = st.distort_depth(dc.depth_input(name, dtype))
        out["%s/distort_depth_%s" % (name, np.dtype(dtype).name)] = res
    holes = float((out[name + "/src_index"] < 0).mean())
    print("%-16s %dx%d  nD=%d  holes %.1f %%" % (name, w, h, len(D), 100 * holes))


def run_get_depth(cal, out):
    g = dc.GET_DEPTH
    st = cal.Stereo().load(dc.rig_record(g["rig"], spelled=True))
    st.set_stereo_matching(cal.SemiGlobalBlockMatching(dict(g["cfg"])), **g["setm"])
    img1, img2 = dc.scene_images()
    arg1 = img1.copy()
    res = st.get_depth(arg1, img2.copy(), return_distort_depth=True)
    out["get_depth/result_keys"] = np.array(sorted(res))
    out["get_depth/distort_img1_is_the_argument"] = np.array(res["distort_img1"] is arg1)
    out["get_depth/img1_sha"], out["get_depth/img2_sha"] = np.array(rc.sha(img1)), np.array(rc.sha(img2))
    out["get_depth/distort_depth"] = res["distort_depth"]
    for k in ("unrectify_depth", "distort_depth"):
        out["get_depth/%s_sha" % k] = np.array(rc.sha(res[k]))
    print("get_depth        keys=%s  distort_depth %s %s, %.1f %% non-zero" % (
        ",".join(sorted(res)), res["distort_depth"].dtype, res["distort_depth"].shape,
        100 * float((res["distort_depth"] != 0).mean())))


def main():
    import oracle
    oracle.build()
    cal = import_reference()
    out = {"reference_version": np.array(cal.__version__)}
    for name in dc.RIGS:
        run_rig(cal, name, out)
    run_get_depth(cal, out)
    np.savez_compressed(dc.FIXTURE, **out)
    print("wrote %s (%d KB, %d arrays)" % (os.path.relpath(dc.FIXTURE, ROOT), os.path.getsize(dc.FIXTURE) // 1024, len(out)))


if __name__ == "__main__":
    main()
