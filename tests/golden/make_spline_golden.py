"""Writes tests/golden/reference_spline.npz: what the reference's ``interpolate_uvzs(uvzs, hw, inter_type="rbf")`` computes
(utils.py:373-388) for a few seeded sample sets -- its own call,

    scipy.interpolate.Rbf(u, v, z, function="thin_plate", smooth=0.5)(xs, ys)   (its ``episilon=5`` is a misspelt keyword
                                                                                 that SciPy stores and never reads)

evaluated at every pixel and laid out as ``uvzs_to_arr2d`` lays it out -- with the inputs, and the distance of the NumPy
restatement (tests/spline_ref.py) from it, the first measured number of the spline.  Needs SciPy; the tests need only the
file.  Run from the repository root:  python tests/golden/make_spline_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spline_ref as ref  # noqa: E402

# name -> (seed, rows, (h, w))
CASES = {"few": (11, 7, (9, 12)), "board": (12, 88, (24, 32)), "scene": (13, 200, (34, 60))}


def scipy_image(uvz, hw):
    from scipy.interpolate import Rbf
    rbf = Rbf(uvz[:, 0], uvz[:, 1], uvz[:, 2], function="thin_plate", smooth=0.5, episilon=5)
    ys, xs = np.mgrid[0:hw[0], 0:hw[1]]
    return rbf(xs.astype(np.float64), ys.astype(np.float64))


def main():
    out = {}
    for name, (seed, n, hw) in CASES.items():
        uvz = ref.samples(seed, n, hw)
        want = scipy_image(uvz, hw)
        got, _, status = ref.image(uvz, hw, 0.5)
        assert status == 0
        rel = float(np.abs(got - want).max() / np.abs(uvz[:, 2]).max())
        print("%s: n = %d, %s: restatement vs SciPy %.3g of max|z|" % (name, n, hw, rel))
        out[name + "/uvz"], out[name + "/hw"], out[name + "/scipy"], out[name + "/restatement_vs_scipy"] = uvz, np.array(hw), want, rel
    np.savez_compressed(os.path.join(HERE, "reference_spline.npz"), **out)


if __name__ == "__main__":
    main()
