"""NumPy restatement of ``Stereo.distort_depth`` (the reference's stereo_camera.py:433-464).  Test infrastructure only.

The reference sends every pixel of the undistorted camera-1 image through three cv2 calls and then lets NumPy decide
who wins a target pixel.  The three calls are restated here from OpenCV 4.x calib3d (``cvUndistortPointsInternal``
without distortion, R or P; ``cvProjectPoints2Internal`` with R = I and t = 0) -- float64 inside, float32 wherever cv2
hands an array over, products and sums in cv2's order.  Like the rest of the cv2-owned arithmetic of this project they
are a restatement, unpinned.  What NumPy does afterwards -- pixel order, truncation,
``np.unique(axis=0, return_index=True)``, the fancy-index scatter, the dtype -- is the reference's own and is pinned by
tests/golden/reference_distort_depth.npz, which its unmodified code produced on top of these stand-ins.

``index_map_unique`` is the literal form (np.unique), ``index_map_minimum_at`` the form the GPU kernel implements
(lowest source index per target); ``target_stats`` says what the product must refuse.
"""
import numpy as np


def _coefficients(D):
    d = np.zeros(14)
    if D is not None:
        v = np.asarray(D, np.float64).reshape(-1)
        d[:v.size] = v
    assert d[12] == 0 and d[13] == 0, "tilted-sensor coefficients are not restated"
    return d[:12]


# ---- the three cv2 calls ---------------------------------------------------------------------------------------
def undistort_points(points, K, D=None):
    """cv2.undistortPoints(points (N, 2) float32, K, None) -> (N, 1, 2) float32: with no distortion, R or P nothing is
    iterated; x = (u - cx) * (1 / fx) in float64, stored as float32."""
    assert D is None, "the path passes no distortion here"
    K = np.asarray(K, np.float64)
    p = np.asarray(points, np.float32).reshape(-1, 2).astype(np.float64)
    ifx, ify = 1.0 / K[0, 0], 1.0 / K[1, 1]
    out = np.empty((len(p), 1, 2), np.float32)
    out[:, 0, 0] = (p[:, 0] - K[0, 2]) * ifx
    out[:, 0, 1] = (p[:, 1] - K[1, 2]) * ify
    return out


def convert_points_to_homogeneous(points):
    """cv2.convertPointsToHomogeneous: (N, 1, 2) float32 -> (N, 1, 3) float32 with a 1 appended."""
    p = np.asarray(points, np.float32).reshape(-1, 1, 2)
    return np.concatenate([p, np.ones((len(p), 1, 1), np.float32)], axis=-1)


def project_points(object_points, rvec, tvec, K, D, image_points=None):
    """cv2.projectPoints((N, 1, 3) float32 with z = 1, rvec = 0, tvec = 0, K, D) -> ((N, 1, 2) float32, None)."""
    assert not np.any(rvec) and not np.any(tvec), "the path passes a zero pose"
    K = np.asarray(K, np.float64)
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coefficients(D)
    P = np.asarray(object_points, np.float32).reshape(-1, 3).astype(np.float64)
    assert (P[:, 2] == 1).all()
    x, y = P[:, 0], P[:, 1]  # R = I exactly, t = 0, z = 1: X / Z is X
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    with np.errstate(all="ignore"):
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
        out = np.empty((len(P), 1, 2), np.float32)
        out[:, 0, 0] = xd * fx + cx
        out[:, 0, 1] = yd * fy + cy
    return out, None


# ---- the reference's own steps ---------------------------------------------------------------------------------
def image_points(K, D, w, h):
    """Steps 1-4: the float32 target (U, V) of every source pixel i = v * w + u, shape (w * h, 2)."""
    u, v = np.meshgrid(np.arange(w, dtype=np.int32), np.arange(h, dtype=np.int32))
    pts = np.stack([u.reshape(-1), v.reshape(-1)], axis=-1).astype(np.float32)
    und = undistort_points(pts, K, None)
    return project_points(convert_points_to_homogeneous(und), np.zeros(3, np.float32), np.zeros(3, np.float32), K, D)[0].reshape(-1, 2)


def target_stats(K, D, w, h):
    """What the product reports for a rig: n_out = source pixels whose truncated target is outside [0, w) x [0, h)
    (non-finite ones included), the range of the finite truncated targets (clamped to +-2^30), n_nonfinite."""
    uv = image_points(K, D, w, h).astype(np.float64)
    finite = np.isfinite(uv).all(axis=1)
    t = np.trunc(np.clip(uv[finite], -2.0 ** 30, 2.0 ** 30)).astype(np.int64)
    inside = (t[:, 0] >= 0) & (t[:, 0] < w) & (t[:, 1] >= 0) & (t[:, 1] < h)
    st = dict(n_out=int((~finite).sum() + (~inside).sum()), n_nonfinite=int((~finite).sum()))
    if len(t):
        st.update(minU=int(t[:, 0].min()), maxU=int(t[:, 0].max()), minV=int(t[:, 1].min()), maxV=int(t[:, 1].max()))
    return st


def _int_points(K, D, w, h):
    with np.errstate(invalid="ignore"):
        return image_points(K, D, w, h).astype(np.int32)  # step 5: truncation toward zero


def index_map_unique(K, D, w, h):
    """Step 6 as the reference writes it: np.unique over the integer points, then a scatter of the first indices.
    -> int32 (h, w), -1 = nobody lands here.  Raises IndexError / wraps negative targets exactly as the reference does."""
    pts, index = np.unique(_int_points(K, D, w, h), axis=0, return_index=True)
    res = np.full((h, w), -1, np.int32)
    res[pts[:, 1], pts[:, 0]] = index
    return res


def index_map_minimum_at(K, D, w, h):
    """The same table as 'the lowest source index per target' (what an atomicMin builds).  Rigs with a target outside
    the image are not its business: assert."""
    assert target_stats(K, D, w, h)["n_out"] == 0
    pts = _int_points(K, D, w, h).astype(np.int64)
    key = np.full(w * h, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(key, pts[:, 1] * w + pts[:, 0], np.arange(w * h, dtype=np.int64))
    key[key == np.iinfo(np.int64).max] = -1
    return key.astype(np.int32).reshape(h, w)


def gather(depth, index_map):
    """out[..., p] = index_map[p] < 0 ? 0 : depth[..., index_map[p]] -- shape and dtype of ``depth``."""
    depth = np.asarray(depth)
    h, w = index_map.shape
    flat = depth.reshape(depth.shape[:-2] + (h * w,))
    idx = index_map.reshape(-1)
    out = np.where(idx >= 0, flat[..., np.maximum(idx, 0)], depth.dtype.type(0))
    return out.reshape(depth.shape).astype(depth.dtype, copy=False)


def distort_depth(depth, K, D, xy):
    """``Stereo.distort_depth(depth)`` for one (h, w) image, steps 1-6 with np.unique and the scatter."""
    w, h = int(xy[0]), int(xy[1])
    depth = np.asarray(depth)
    res = np.zeros((h, w), depth.dtype)
    pts, index = np.unique(_int_points(K, D, w, h), axis=0, return_index=True)
    res[pts[:, 1], pts[:, 0]] = depth.reshape(-1)[index]
    return res
