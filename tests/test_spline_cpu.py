"""The thin-plate spline fill without a GPU: the argument checks of calibrating_amd.sparse's spline functions (every refusal
comes before the device is touched), and the NumPy restatement (tests/spline_ref.py) against the reference's own call,
``scipy.interpolate.Rbf(u, v, z, function="thin_plate", smooth=0.5)``, recorded in tests/golden/reference_spline.npz by
tests/golden/make_spline_golden.py."""
import inspect
import os

import numpy as np
import pytest

import calibrating_amd as ca
from calibrating_amd import _native, sparse

import spline_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_spline.npz")
CASES = ("few", "board", "scene")
# The restatement and SciPy solve the same system by two eliminations (this LU; LAPACK's blocked gesv) and add the same terms
# in two orders (row order; BLAS dot): they differ by rounding, amplified by the system's condition.  The recorded distance
# grows with n as that condition does (1.3e-14, 9.5e-12, 7.4e-11 of max|z| at n = 7, 88, 200); anything near 1e-8 would be
# a different formula, not rounding.
RESTATEMENT_VS_SCIPY = 1e-9


def test_surface_without_a_gpu():
    assert sparse.MAX_SPLINE_POINTS == _native.SPLINE_MAX_POINTS == 1024
    assert (sparse.SPLINE_NO_SAMPLE, sparse.SPLINE_SINGULAR, sparse.SPLINE_NON_FINITE) == (1, 2, 4)
    q = inspect.signature(sparse.interpolate_uvzs_rbf).parameters
    assert list(q) == ["uvzs", "hw", "smooth", "counts", "mask", "return_info"]
    assert (q["hw"].default, q["smooth"].default, q["counts"].default, q["mask"].default, q["return_info"].default) == \
        (None, 0.5, None, None, False)
    q = inspect.signature(sparse.interpolate_sparse2d_rbf).parameters
    assert list(q) == ["sparse2d", "smooth", "mask"] and q["smooth"].default == 0.5
    q = inspect.signature(ca.FeatureMatchingAsStereoMatching.__init__).parameters
    assert list(q) == ["self", "feature_matching", "downscale", "inter_type"]
    assert q["downscale"].default == 8 and q["inter_type"].default == "nearest"
    assert ca.FeatureMatchingAsStereoMatching(None, inter_type="rbf").inter_type == "rbf"
    with pytest.raises(ValueError, match="inter_type"):
        ca.FeatureMatchingAsStereoMatching(None, inter_type="lstsq")
    for name in ("camd_spline_assemble", "camd_spline_solve", "camd_spline_eval", "camd_spline_upsize"):
        assert name in _native.SIGNATURES
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "calibrating_amd.h")).read()
    assert "#define CAMD_SPLINE_MAX_POINTS %d " % sparse.MAX_SPLINE_POINTS in header
    # the plain fill keeps refusing the value: the spline has names of its own
    with pytest.raises(NotImplementedError):
        sparse.interpolate_uvzs(np.ones((4, 3)), (4, 4), inter_type="rbf")


def test_refusals_come_before_the_device():
    rbf = sparse.interpolate_uvzs_rbf
    big = np.ones((sparse.MAX_SPLINE_POINTS + 1, 3))
    for call in (lambda: rbf(big, (8, 8)), lambda: rbf(np.ones((2, sparse.MAX_SPLINE_POINTS + 1, 3)), (8, 8)),
                 lambda: rbf(big, (8, 8), counts=[0, sparse.MAX_SPLINE_POINTS + 1]),
                 lambda: sparse.spline_assemble(big), lambda: sparse.spline_eval(big, np.ones(len(big)), (8, 8)),
                 lambda: sparse.spline_solve(np.eye(len(big)), np.ones(len(big))),
                 lambda: sparse.interpolate_sparse2d_rbf(np.ones((40, 40)))):
        with pytest.raises(ValueError, match="MAX_SPLINE_POINTS = 1024.*uvzs_to_arr2d.*coarser grid"):
            call()
    rows = ref.samples(1, 6, (8, 8))
    with pytest.raises(ValueError, match=r"\(n, >= 3\)"):
        rbf(rows[:, :2], (8, 8))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        rbf(np.ones((6, 4)), (8, 8))
    with pytest.raises(ValueError, match=r"\(n, >= 3\)"):
        rbf(np.ones(6), (8, 8))
    with pytest.raises(ValueError, match="counts"):
        rbf(rows, (8, 8), counts=[2, 3])
    with pytest.raises(ValueError, match="counts"):
        rbf(rows, (8, 8), counts=[[6]])
    with pytest.raises(ValueError, match="counts"):
        rbf(rows, (8, 8), counts=[7, -1])
    with pytest.raises(ValueError, match="hw"):
        rbf(rows, (0, 8))
    with pytest.raises(ValueError, match="hw=None"):
        rbf(np.zeros((0, 3)))
    with pytest.raises(ValueError, match="smooth"):
        rbf(rows, (8, 8), smooth=float("nan"))
    for col in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            r = rows.copy()
            r[3, col] = bad
            with pytest.raises(ValueError, match="u, v, z must be finite"):
                rbf(r, (8, 8))
            if col < 2:
                with pytest.raises(ValueError, match="finite"):
                    rbf(r)
    with pytest.raises(ValueError, match="mask"):
        rbf(rows, (8, 8), mask=np.ones((8, 9), np.uint8))
    with pytest.raises(ValueError, match="mask"):
        rbf(rows, (8, 8), mask=np.ones((1, 8, 8), np.uint8))  # (one frame, not a batch)
    with pytest.raises(ValueError, match="mask"):
        rbf(rows, (8, 8), counts=[2, 4], mask=np.ones((3, 8, 8), np.uint8))
    with pytest.raises(TypeError):
        rbf([[1.0, 2.0, 3.0]], (8, 8))
    with pytest.raises(ValueError, match="sparse2d"):
        sparse.interpolate_sparse2d_rbf(np.zeros((4, 4, 3)))
    # the stages
    with pytest.raises(ValueError, match="weights"):
        sparse.spline_eval(rows, np.ones(5), (8, 8))
    with pytest.raises(ValueError, match="weights"):
        sparse.spline_eval(rows, np.ones((2, 3)), (8, 8), counts=[2, 4])
    with pytest.raises(ValueError, match="grid_step"):
        sparse.spline_eval(rows, np.ones(6), (8, 8), grid_step=0)
    with pytest.raises(ValueError, match="A must be"):
        sparse.spline_solve(np.ones((3, 4)), np.ones(3))
    with pytest.raises(ValueError, match="does not go with"):
        sparse.spline_solve(np.eye(3), np.ones(4))
    with pytest.raises(ValueError, match="does not go with"):
        sparse.spline_solve(np.ones((2, 3, 3)), np.ones(5), counts=[1, 3])
    with pytest.raises(ValueError, match="counts"):
        sparse.spline_solve(np.ones((2, 3, 3)), np.ones(3), counts=[3])
    with pytest.raises(ValueError, match="float64"):
        sparse.spline_upsize(np.ones((4, 4), np.float32), (8, 8))


def test_the_library_refuses_bad_arguments_without_a_device():
    lib = _native.lib()
    for name, args in (("camd_spline_assemble", (None, 0, 0, None, 0, 0, 0.0, None, None)),
                       ("camd_spline_solve", (None, 0, 0, None, 0, 0, None, None, None, None)),
                       ("camd_spline_eval", (None, 0, 0, None, 0, 0, None, None, 0, 0, 0, None, None)),
                       ("camd_spline_upsize", (None, 0, 0, 0, None, 0, 0, None))):
        assert getattr(lib, name)(*args) == _native.CAMD_ERR_BAD_ARG, name
        assert _native.last_error().startswith(name + ": bad arguments"), _native.last_error()
    # a capacity beyond the cap
    buf = np.zeros(16)
    start = np.zeros(2, np.int64)
    assert lib.camd_spline_solve(buf.ctypes.data, 1, 0, start.ctypes.data, 1, sparse.MAX_SPLINE_POINTS + 1, buf.ctypes.data,
                                 buf.ctypes.data, start.ctypes.data, None) == _native.CAMD_ERR_BAD_ARG


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_references_own_call(name):
    fx = np.load(GOLDEN)
    uvz, hw, want = fx[name + "/uvz"], tuple(int(v) for v in fx[name + "/hw"]), fx[name + "/scipy"]
    got, w, status = ref.image(uvz, hw, 0.5)
    assert status == 0 and got.dtype == np.float64 and got.shape == want.shape == hw
    rel = float(np.abs(got - want).max() / np.abs(uvz[:, 2]).max())
    print("%s: the restatement lies %.3g of max|z| from SciPy (recorded %.3g)" % (name, rel, float(fx[name + "/restatement_vs_scipy"])))
    assert rel <= RESTATEMENT_VS_SCIPY
    assert float(fx[name + "/restatement_vs_scipy"]) <= RESTATEMENT_VS_SCIPY


def test_restatement_stages():
    uvz = ref.samples(3, 20, (12, 12))
    A = ref.assemble(uvz[:, :2], 0.5)
    assert np.array_equal(A, A.T) and (np.diag(A) == -0.5).all()
    w, status = ref.lu_solve(A, uvz[:, 2])
    assert status == 0 and np.abs(A @ w - uvz[:, 2]).max() < 1e-9
    assert np.abs(w - np.linalg.solve(A, uvz[:, 2])).max() <= 1e-9 * np.abs(w).max()
    # a matrix that needs an exchange at every step, a singular one, a non-finite one, none
    n = 6
    P = np.eye(n)[::-1] * np.arange(1, n + 1) + np.triu(np.ones((n, n)), 1)[::-1] * 0.25
    w, status = ref.lu_solve(P, np.arange(n, dtype=np.float64))
    assert status == 0 and np.abs(P @ w - np.arange(n)).max() < 1e-12
    dup = uvz[[0, 1, 1, 2]]
    assert ref.lu_solve(ref.assemble(dup[:, :2], 0.0), dup[:, 2])[1] == ref.SINGULAR
    assert ref.lu_solve(np.array([[1.0, np.nan], [0.0, 1.0]]), np.ones(2))[1] == ref.NON_FINITE
    assert ref.lu_solve(np.zeros((0, 0)), np.zeros(0))[1] == ref.NO_SAMPLE
    img, scale = ref.evaluate(uvz[:, :2], w[:0], (3, 4))
    assert not img.any() and not scale.any()
    assert ref.ulps(np.array([1.0, -0.0]), np.array([np.nextafter(1.0, 2.0), 0.0])) == 1.0


def test_exact_reference_fixtures_are_well_conditioned():
    """the end-to-end fixtures of tests/test_gpu_spline.py: the restatement's own error stays below 1e-6 of max|z| -- a
    condition on the inputs, checked here where no GPU is needed"""
    for seed, n in ref.EXACT_CASES:
        uvz = ref.samples(seed, n, ref.EXACT_HW)
        err = np.abs(ref.image(uvz, ref.EXACT_HW)[0] - ref.exact_image(uvz, ref.EXACT_HW)).max() / np.abs(uvz[:, 2]).max()
        print("n = %d: the restatement lies %.3g of max|z| from the exact spline" % (n, err))
        assert err < 1e-6
