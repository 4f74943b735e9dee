"""NumPy restatement of ``cv2.undistortPoints(src, K, D)`` (no R, no P) and ``cv2.projectPoints`` (no Jacobians) as
``csrc/points.hip`` defines them.  Test infrastructure only.

Plain elementwise float64 in the stated order of operations -- every product and sum a NumPy ufunc call of its own, so
each is rounded once -- and the input's type only where cv2 hands an array over.  ``distort_depth_ref`` holds the same
two calls for the special case ``Stereo.distort_depth`` needs (no distortion in the first, zero pose and z = 1 in the
second); tests/test_points_cpu.py checks that the general forms reduce to them bit for bit.
"""
import numpy as np

from distort_depth_ref import _coefficients

NDIST = (0, 4, 5, 8, 12, 14)


def _rows(a, width):
    a = np.asarray(a)
    assert a.dtype in (np.float32, np.float64), a.dtype
    if a.ndim == 3:
        a = a[:, 0]
    assert a.ndim == 2 and a.shape[1] == width, a.shape
    return a


def _ndist(D):
    n = 0 if D is None else np.asarray(D).size
    assert n in NDIST, n
    return n


def undistort_trace(uvs, K, D=None, iters=5):
    """(normalised points (n, 2) float64 BEFORE the hand-over, took_exit (n,) bool: the point met icdist < 0)."""
    K = np.asarray(K, np.float64)
    p = _rows(uvs, 2).astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ifx, ify = 1.0 / fx, 1.0 / fy
    xs, ys = (p[:, 0] - cx) * ifx, (p[:, 1] - cy) * ify
    done = np.zeros(len(p), bool)
    if _ndist(D) == 0:
        return np.stack([xs, ys], 1), done
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coefficients(D)
    x, y = xs.copy(), ys.copy()
    with np.errstate(all="ignore"):
        for _ in range(int(iters)):
            r2 = x * x + y * y
            icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
            neg = icdist < 0
            dX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 * r2
            dY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r2 * r2
            xn = np.where(neg, xs, (xs - dX) * icdist)
            yn = np.where(neg, ys, (ys - dY) * icdist)
            x, y = np.where(done, x, xn), np.where(done, y, yn)
            done = done | neg
    return np.stack([x, y], 1), done


def undistort_points(uvs, K, D=None, iters=5):
    """cv2.undistortPoints(uvs, K, D)[:, 0]: (n, 2) normalised points in the input's type."""
    with np.errstate(over="ignore"):
        return undistort_trace(uvs, K, D, iters)[0].astype(_rows(uvs, 2).dtype)


def cam_undistort_points(uvs, K, D=None, iters=5):
    """Cam.undistort_points (the reference's camera.py:286-287): ``normalised * [[fx, fy]] + [cx, cy]`` -> float64."""
    K = np.asarray(K, np.float64)
    with np.errstate(all="ignore"):
        return undistort_points(uvs, K, D, iters) * [[K[0, 0], K[1, 1]]] + [K[:2, 2]]


def project_points(xyzs, R, t, K, D=None):
    """cv2.projectPoints(xyzs, rvec, tvec, K, D)[0][:, 0] with R = the 3x3 matrix of rvec: (n, 2) in the input's type."""
    K, R, t = np.asarray(K, np.float64), np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    _ndist(D)
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coefficients(D)
    rows = _rows(xyzs, 3)
    P = rows.astype(np.float64)
    X0, Y0, Z0 = P[:, 0], P[:, 1], P[:, 2]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    with np.errstate(all="ignore"):
        X = R[0, 0] * X0 + R[0, 1] * Y0 + R[0, 2] * Z0 + t[0]
        Y = R[1, 0] * X0 + R[1, 1] * Y0 + R[1, 2] * Z0 + t[1]
        Z = R[2, 0] * X0 + R[2, 1] * Y0 + R[2, 2] * Z0 + t[2]
        iz = np.where(Z != 0, 1.0 / Z, 1.0)
        x, y = X * iz, Y * iz
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        a1 = 2 * x * y
        a2 = r2 + 2 * x * x
        a3 = r2 + 2 * y * y
        cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6
        icdist2 = 1.0 / (1 + k4 * r2 + k5 * r4 + k6 * r6)
        xd = x * cdist * icdist2 + p1 * a1 + p2 * a2 + s1 * r2 + s2 * r4
        yd = y * cdist * icdist2 + p1 * a3 + p2 * a1 + s3 * r2 + s4 * r4
        return np.stack([xd * fx + cx, yd * fy + cy], 1).astype(rows.dtype)
