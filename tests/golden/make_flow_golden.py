#!/usr/bin/env python3
"""Runs the REFERENCE's own ``flow_utils.warp_flow`` on the cases of tests/flow_cases.py and writes
tests/golden/reference_flow.npz.

BUILD CONTAINER ONLY (it needs the reference checkout next to this repository; only the .npz travels).
    python tests/golden/make_flow_golden.py

What is executed.  The reference package is imported from where it lies, unmodified, through
``make_reference_golden.import_reference`` (that file is used as it is, with its oracle-backed stand-ins for cv2 / boxx),
and its own code runs:
    flow_utils.warp_flow(flow, img2=img2, interpolation=...)     flow_utils.py:110-112,126-129   backward, incl. boxx.resize
    flow_utils.warp_flow(flow, img1=img1, interpolation=...)     flow_utils.py:110-125           forward

WHAT THIS PINS AND WHAT IT DOES NOT.  It pins the reference's own NumPy: the float64 promotion of
``flow * [[[w]], [[h]]]`` for float32 and float64 flows, the float32 hand-over of the backward maps, np.round's
half-to-even and the int32 cast, the mask (``flow.any(0)``: -0.0 is zero; the four range tests) and the scatter order of
the fancy assignment (the last source in row-major order stays).  It does NOT pin cv2's arithmetic: cv2.remap and the
cv2.resize behind boxx.resize are the oracle's restatements.
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
import flow_cases as cases  # noqa: E402


def main():
    import oracle
    oracle.build()
    cal = mrg.import_reference()
    warp_flow = cal.flow_utils.warp_flow
    out = {"reference_version": np.array(cal.__version__)}
    for name, (flow, img2, interp) in cases.backward_cases().items():
        out[name] = warp_flow(flow.copy(), img2=img2.copy(), interpolation=interp)
        assert out[name].dtype == np.uint8 and out[name].shape == flow.shape[1:] + img2.shape[2:]
    for name, (flow, img1) in cases.forward_inputs().items():
        for tag, interp in cases.FORWARD_INTERPOLATIONS:
            out["%s/%s" % (name, tag)] = warp_flow(flow.copy(), img1=img1.copy(), interpolation=interp)
            assert out["%s/%s" % (name, tag)].shape == flow.shape[1:] + img1.shape[2:]
    # img1 wins when both are given (flow_utils.py:113)
    flow, img1 = cases.forward_inputs()["f_outside"]
    both = warp_flow(flow.copy(), img1=img1.copy(), img2=cases.image(2, cn=3), interpolation=cases.INTER_LINEAR)
    assert np.array_equal(both, out["f_outside/linear"])
    np.savez_compressed(cases.FIXTURE, **out)
    print("wrote %s (%d KB, %d arrays)" % (os.path.relpath(cases.FIXTURE, ROOT), os.path.getsize(cases.FIXTURE) // 1024, len(out)))


if __name__ == "__main__":
    main()
