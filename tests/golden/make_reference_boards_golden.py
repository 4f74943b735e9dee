#!/usr/bin/env python3
"""Runs the REFERENCE's own boards.py and writes tests/golden/reference_boards.npz: ``Chessboard(...).object_points`` and
``Chessboard.build_with_calibration_img(...)`` for the arguments below.

BUILD CONTAINER ONLY, like make_reference_golden.py, whose cv2 / boxx stand-ins it installs: the reference's package is
imported from where it lies, unmodified, and nothing of it is copied here.  Both methods are pure NumPy; no stand-in is
called on their path (a called one raises).
    python tests/golden/make_reference_boards_golden.py
"""
import os

import numpy as np

import make_reference_golden as mrg

FIXTURE = os.path.join(mrg.HERE, "reference_boards.npz")
BOARDS = [((11, 8), 25), ((4, 3), 25), ((9, 6), 30.5), ((7, 7), 10)]   # (checkboard, size_mm)
IMAGES = [((1080, 1920), 15, 300), ((480, 640), 7, 120), ((300, 300), 5, 96), ((2480, 3508), 10, 321.29)]  # (hw, n, ppi)


def main():
    cal = mrg.import_reference()
    from calibrating import boards
    out = {"reference_version": np.array(cal.__version__)}
    for i, (checkboard, size_mm) in enumerate(BOARDS):
        b = boards.Chessboard(checkboard=checkboard, size_mm=size_mm)
        out["board%d/args" % i] = np.array([checkboard[0], checkboard[1], size_mm], np.float64)
        out["board%d/object_points" % i] = b.object_points
    for i, (hw, n, ppi) in enumerate(IMAGES):
        b = boards.Chessboard.build_with_calibration_img(hw=hw, n=n, ppi=ppi)
        out["image%d/args" % i] = np.array([hw[0], hw[1], n, ppi], np.float64)
        out["image%d/checkboard" % i] = np.array(b.checkboard, np.int64)
        out["image%d/object_points" % i] = b.object_points
        out["image%d/name" % i] = np.array(b.calibration_img_name)
        out["image%d/info" % i] = np.array(repr(sorted(b.calibration_img_info.items())))
        out["image%d/img_bits" % i] = np.packbits(b.calibration_img == 255)
        assert set(np.unique(b.calibration_img)) <= {0, 255}
    np.savez_compressed(FIXTURE, **out)
    print("wrote %s (%d KB, %d arrays)" % (os.path.relpath(FIXTURE, mrg.ROOT), os.path.getsize(FIXTURE) // 1024, len(out)))


if __name__ == "__main__":
    main()
