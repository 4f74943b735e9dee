"""Inputs of the camera-model tests (tests/test_camera_model_cpu.py and the table tests of tests/test_gpu_pipeline.py).
Only DATA lives here: image sizes and seeded rigs, regenerated from seeds on both sides of a comparison."""
import numpy as np

import fuzzers

# (w, h) on the edges of cv2.undistort's stripe rule, rows per stripe = (1 << 12) / w clamped to [1, h]
STRIPE_SIZES = ((64, 130),    # stripes of 64 rows, the last one partial
                (1, 5000),    # one stripe of 4096 rows, then a second
                (4097, 3),    # (1 << 12) / w == 0, clamped to 1
                (97, 33))     # one stripe covers the image


def stripe_rig(w, h, ndist, seed=0):
    """A camera for a w x h image and a lens of ``ndist`` coefficients with the magnitudes of ``fuzzers._undistort_rig``
    (14: zero tilt; 0: None).  The focal length follows the LONGER side, so that the normalised radius stays below 1 on
    the 1-pixel-wide and 3-pixel-high images too and every map entry stays inside int16, where cv2's encoding is defined."""
    rng = np.random.default_rng([seed, w, h, ndist])
    side = max(w, h)
    K, D = fuzzers._undistort_rig(rng, side, side, min(ndist, 12))
    K[0, 2] += (w - side) / 2
    K[1, 2] += (h - side) / 2
    if ndist == 0:
        return K, None
    return K, np.concatenate([D, np.zeros(ndist - D.size)])
