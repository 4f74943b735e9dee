"""The host side every joint Levenberg-Marquardt solver shares (``calibrate``, ``stereo_calibrate``, ``bundle``): the state's
read-back, the loop around one evaluation, and the solver's status.  The device side is csrc/joint_common.hpp.
"""
import numpy as np

from . import _native

STATUS_OK, STATUS_SINGULAR = 0, 3
STATUS_TEXT = {0: "ok", 3: "singular or not converged at the cap"}


def read_state(state, dev, count, what):
    """The first ``count`` doubles of a solver's device state (``camd_calib_read``: the three states begin alike)."""
    out = np.empty(count)
    _native.call("camd_calib_read", dev, state.data_ptr(), count, out.ctypes.data, what=what)
    return out


def iterate(state, dev, what, step, linearise=None):
    """Evaluations until the device says done.  The only read-back of an evaluation is 16 bytes: done, accept.  A solver
    whose step does not linearise by itself passes ``linearise``, called first and after every step that was taken."""
    if linearise is not None:
        linearise()
    while True:
        step()
        done, accept = read_state(state, dev, 2, what)
        if accept and linearise is not None:
            linearise()
        if done:
            return


def check_status(what, status, evaluations, pivot):
    """``ValueError`` unless the finished solver's status is ``STATUS_OK``."""
    if int(status) != STATUS_OK:
        raise ValueError("%s: status %d (%s) after %d evaluations, smallest pivot %.3g" % (what, status, STATUS_TEXT[3], evaluations, pivot))
