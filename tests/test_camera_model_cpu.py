"""The camera model shared by csrc/tables.hip, distort.hip and points.hip (csrc/camera_model.hpp), held without a GPU.

(a) ``camd_undistort_maps_host`` runs the kernel's own per-pixel functions, so "device maps == host maps" compares one
text compiled twice.  What keeps that meaningful is pinned here: the host maps, pushed through the NumPy model of cv2's
fixed-point remap, give bit for bit what the oracle's own stripe-wise construction (oracle/remap_ref.c) gives.
(b) All six entry points that take (K, dist) refuse the same things with the same status, each under its own name, before
the device is asked for; which coefficient counts an entry point takes stays its own rule.  No GPU."""
import ctypes

import numpy as np
import pytest

from calibrating_amd import _native, imgproc

import np_fixed_remap
import points_cases as pc
from camera_model_cases import STRIPE_SIZES, stripe_rig


@pytest.mark.parametrize("size", STRIPE_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ndist", pc.NDIST)
def test_host_maps_through_the_remap_model_are_the_oracles_undistort(oracle, size, ndist):
    w, h = size
    K, D = stripe_rig(w, h, ndist)
    img = np.random.default_rng(w * 31 + ndist).integers(0, 256, (h, w), dtype=np.uint8)
    mapxy, mapa = imgproc.undistort_maps(K, D, (w, h))
    assert np.abs(mapxy.astype(np.int32)).max() < 32767  # the rig keeps its promise: nothing saturates
    got = np_fixed_remap.remap_fixed_bilinear(img, mapxy, mapa, oracle.bilinear_itab())
    assert np.array_equal(got, oracle.undistort_u8(img, K, D))


# ---- (b) the argument contract through the raw ABI ---------------------------------------------------------------
POINT_CALLS = ("camd_undistort_points", "camd_project_points")
MAP_CALLS = ("camd_init_undistort_rectify_map", "camd_undistort_maps", "camd_undistort_maps_host", "camd_distort_index_map")
W4 = H4 = 4


class Buffers:
    """Output and input buffers of a 4 x 4 call: device memory where there is a device (the call then completes there),
    host memory otherwise (no call gets as far as a launch); the host entry point writes host memory either way."""

    def __init__(self):
        import torch
        self.keep = []
        self.gpu = torch.cuda.is_available()

    def host(self, nbytes):
        a = np.zeros(nbytes, np.uint8)
        self.keep.append(a)
        return a.ctypes.data

    def dev(self, nbytes):
        if not self.gpu:
            return self.host(nbytes)
        import torch
        t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        self.keep.append(t)
        return t.data_ptr()


def call(name, buf, dist, ndist):
    """``name`` on a 4 x 4 image / 4 points with good arguments but for (dist, ndist) -> the status."""
    lib = _native.lib()
    K = np.array([4.0, 0, 2, 0, 4, 2, 0, 0, 1])
    R, t = np.eye(3).reshape(9), np.zeros(3)
    buf.keep += [K, R, t, dist]
    dptr = None if dist is None else ctypes.cast(dist, ctypes.c_void_p)
    n = W4 * H4
    if name == "camd_init_undistort_rectify_map":
        return lib.camd_init_undistort_rectify_map(K.ctypes.data, dptr, ndist, None, K.ctypes.data, W4, H4, buf.dev(4 * n),
                                                   buf.dev(4 * n), buf.dev(n), W4, H4, None)
    if name == "camd_undistort_maps":
        return lib.camd_undistort_maps(K.ctypes.data, dptr, ndist, W4, H4, buf.dev(4 * n), buf.dev(2 * n), None)
    if name == "camd_undistort_maps_host":
        return lib.camd_undistort_maps_host(K.ctypes.data, dptr, ndist, W4, H4, buf.host(4 * n), buf.host(2 * n))
    if name == "camd_distort_index_map":
        return lib.camd_distort_index_map(K.ctypes.data, dptr, ndist, W4, H4, buf.dev(4 * n), buf.dev(4 * 6), None)
    if name == "camd_undistort_points":
        return lib.camd_undistort_points(buf.dev(8 * 2 * 4), _native.VALUE_F64, 4, 2, K.ctypes.data, dptr, ndist, 5,
                                         buf.dev(8 * 2 * 4), _native.VALUE_F64, None)
    assert name == "camd_project_points"
    return lib.camd_project_points(buf.dev(8 * 3 * 4), _native.VALUE_F64, 4, 3, R.ctypes.data, t.ctypes.data, K.ctypes.data,
                                   dptr, ndist, buf.dev(8 * 2 * 4), None)


def doubles(values):
    return (ctypes.c_double * len(values))(*values)


@pytest.mark.parametrize("name", MAP_CALLS + POINT_CALLS)
def test_every_entry_point_refuses_the_same_lenses_under_its_own_name(name):
    buf = Buffers()
    tilted = doubles(list(pc.FULL12) + [0.01, 0.0])  # tauX alone
    assert call(name, buf, tilted, 14) == _native.CAMD_ERR_UNSUPPORTED
    msg = _native.last_error()
    assert "tilted" in msg and name + ":" in msg, msg
    assert call(name, buf, doubles([0.0] * 15), 15) == _native.CAMD_ERR_BAD_ARG
    assert name in _native.last_error()
    for ndist in (1, 4, 14):
        assert call(name, buf, None, ndist) == _native.CAMD_ERR_BAD_ARG, ndist
        assert name in _native.last_error()


@pytest.mark.parametrize("ndist", (1, 3, 7))
def test_which_counts_an_entry_point_takes_is_its_own_rule(ndist):
    """cv2's point calls take 4, 5, 8, 12 or 14 coefficients and nothing else; the table builders take any prefix of the
    14.  Good arguments then get as far as the device -- CAMD_ERR_NO_DEVICE where there is none (CAMD_OK from the host
    call), CAMD_OK where there is one -- and never come back as an argument error."""
    import torch
    buf = Buffers()
    D = doubles(list(pc.FULL12[:ndist]))
    for name in POINT_CALLS:
        assert call(name, buf, D, ndist) == _native.CAMD_ERR_BAD_ARG, name
        assert name in _native.last_error()
    for name in MAP_CALLS:
        rc = call(name, buf, D, ndist)
        assert rc not in (_native.CAMD_ERR_BAD_ARG, _native.CAMD_ERR_UNSUPPORTED), (name, rc, _native.last_error())
        assert rc == (_native.CAMD_OK if buf.gpu or name.endswith("_host") else _native.CAMD_ERR_NO_DEVICE), (name, rc)
    if buf.gpu:
        torch.cuda.synchronize()
