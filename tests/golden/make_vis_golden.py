#!/usr/bin/env python3
"""Runs the REFERENCE's own ``utils.vis_depth_l1``, ``vis_depth``, ``vis_stereo`` and ``vis_align`` on the cases of
tests/vis_cases.py and writes tests/golden/reference_vis.npz.

BUILD CONTAINER ONLY (it needs the reference checkout next to this repository; only the .npz travels).
    python tests/golden/make_vis_golden.py

The reference package is imported from where it lies, unmodified, through ``make_reference_golden.import_reference``
(used as it is).  On top of its stand-ins this script adds what these four functions touch:
    np.bool8 = np.bool_               the alias NumPy 2 dropped
    boxx.sliceInt[key] -> key         (boxx rounds float slice bounds; the bounds here are integers)
    boxx.norma                        recollection: (a - a.min()) / (a.max() - a.min())
    boxx.uint8                        recollection: (a * 255.999).astype(np.uint8)
    cv2.applyColorMap(idx, id)        lookup in calibrating_amd.vis.colormap_table(id), returned in BGR order
    cv2.COLORMAP_JET / COLORMAP_HSV   cv2's ids 2 / 9

WHAT THIS PINS AND WHAT IT DOES NOT.  vis_depth_l1 and the uint8 paths of vis_stereo / vis_align are the reference's own
NumPy from end to end: mask, colour bar (np.linspace, placement, width), np.partition's rank, the colouring, the line
positions through both rot90s.  vis_depth pins clip / normalise / slice / the 255.9 cast / the zero mask; the colour
tables, boxx.norma and boxx.uint8 are restatements.  float32 cases are fed widened to float64.
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
import vis_cases as cases  # noqa: E402


class _SliceInt:
    def __getitem__(self, key):
        return key


def _norma(a):
    return (a - a.min()) / (a.max() - a.min())


def _apply_color_map(idx, colormap):
    from calibrating_amd import vis
    return vis.colormap_table(int(colormap))[idx][..., ::-1].copy()


def _wide(a):
    return a.astype(np.float64) if isinstance(a, np.ndarray) and a.dtype == np.float32 else a


def main():
    import oracle
    oracle.build()
    cal = mrg.import_reference()
    np.bool8 = np.bool_
    boxx, cv2 = sys.modules["boxx"], sys.modules["cv2"]
    boxx.sliceInt, boxx.norma, boxx.uint8 = _SliceInt(), _norma, lambda a: (a * 255.999).astype(np.uint8)
    cv2.applyColorMap, cv2.COLORMAP_JET, cv2.COLORMAP_HSV = _apply_color_map, 2, 9
    utils = cal.utils
    out = {"reference_version": np.array(cal.__version__)}
    for name, (re, gt, kw) in cases.l1_cases().items():
        out["l1/" + name] = utils.vis_depth_l1(_wide(re).copy(), _wide(gt) if np.ndim(gt) == 0 else _wide(gt).copy(), **kw)
        assert out["l1/" + name].dtype == np.uint8 and out["l1/" + name].shape == re.shape + (3,)
    for name, (d, kw) in cases.depth_cases().items():
        out["depth/" + name] = utils.vis_depth(_wide(d).copy(), **kw)
        assert out["depth/" + name].dtype == np.uint8 and out["depth/" + name].shape == d.shape + (3,)
    for name, (a, b, n_line) in cases.line_cases().items():
        out["stereo/" + name] = utils.vis_stereo(a.copy(), b.copy(), n_line=n_line)
        for t, tile in enumerate(utils.vis_align(a.copy(), b.copy(), n_line=n_line, shows=False)):
            out["align/%s/%d" % (name, t)] = np.ascontiguousarray(tile)
    try:  # the reference's own default call fails: it negates max_l1=None while building the bar
        utils.vis_depth_l1(*cases.depth_pair((37, 53), 1))
        raise SystemExit("the reference's default vis_depth_l1 call was expected to raise TypeError")
    except TypeError:
        pass
    np.savez_compressed(cases.FIXTURE, **out)
    print("wrote %s (%d KB, %d arrays)" % (os.path.relpath(cases.FIXTURE, ROOT), os.path.getsize(cases.FIXTURE) // 1024, len(out)))


if __name__ == "__main__":
    main()
