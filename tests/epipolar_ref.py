"""NumPy restatements of the epipolar helpers, written from their behaviour (tests/test_epipolar_cpu.py shows them equal
to the reference's own output, tests/golden/reference_epipolar.npz, bit for bit; the GPU tests at scale compare with them)
and the exact yardsticks of the float results."""
from fractions import Fraction

import numpy as np

import sparse_ref as sr


def _cells(uvs, d):
    """Signed cell of every row as one sortable int64 key (u major), NumPy's own dtype rules for the quotient."""
    c = np.rint(uvs / d).astype(np.int64)
    return c[:, 0] * (1 << 32) + c[:, 1]


def matching(uvs1, uvs2, d=1, min_matched=10):
    """Per cell shared by both sets the first row of each landing there, cells ascending in (u, v)."""
    k1, i1 = np.unique(_cells(uvs1, d), return_index=True)
    k2, i2 = np.unique(_cells(uvs2, d), return_index=True)
    in2 = np.isin(k1, k2, assume_unique=True)
    in1 = np.isin(k2, k1, assume_unique=True)
    if in2.sum() < min_matched:
        return {}
    return dict(uv_match_idx1=i1[in2].astype(np.int64), uv_match_idx2=i2[in1].astype(np.int64))


def overlap_filter(uvs1, uvs2):
    """Rows whose rounded pixel is hit once in set 1 and once in set 2."""
    keep = np.ones(len(uvs1), bool)
    for uvs in (uvs1, uvs2):
        _, inverse, counts = np.unique(_cells(uvs, 1), return_inverse=True, return_counts=True)
        keep &= counts[inverse.reshape(-1)] <= 1
    return uvs1[keep], uvs2[keep]


def flow_to_uvs(flow_abs, mask):
    h, w = mask.shape
    ys, xs = np.nonzero(mask)  # row-major
    uvs_from = np.stack([xs + 0.5 - 1e-8, ys + 0.5 - 1e-8], 1)
    return uvs_from, uvs_from + flow_abs[ys, xs].astype(np.float64)


def abs_to_normal(flow_abs):
    h, w, _ = flow_abs.shape
    out = np.empty((2, h, w), np.float32)
    out[0], out[1] = flow_abs[..., 0].astype(np.float64) / w, flow_abs[..., 1].astype(np.float64) / h
    return out


def normal_to_abs(flow, hw=None):
    h, w = flow.shape[1:] if hw is None else hw
    return np.stack([flow[0].astype(np.float64) * w, flow[1].astype(np.float64) * h], 2)


def set2ds(viewds, flowds):
    out = {}
    for i, j in sorted({tuple(sorted(k)) for k in flowds}):
        d = {}
        for (a, b), key in (((i, j), "ij"), ((j, i), "ji")):
            f = flowds.get((a, b))
            if f is None or f["common_fov_mask"].sum() <= 10:
                continue
            flow = f.get("flow_abs")
            if flow is None:
                fn = f["flow_normal"]
                flow = normal_to_abs(fn, viewds[b]["mask"].shape if "mask" in viewds[b] else fn.shape[1:])
            d["uvs_%s_%s" % (key, key[0])], d["uvs_%s_%s" % (key, key[1])] = flow_to_uvs(flow, f["common_fov_mask"])
        if d:
            d["uvs_i"] = np.concatenate([d[k] for k in ("uvs_ij_i", "uvs_ji_i") if k in d])
            d["uvs_j"] = np.concatenate([d[k] for k in ("uvs_ij_j", "uvs_ji_j") if k in d])
            out[frozenset((i, j))] = d
    return out


# ---- yardsticks --------------------------------------------------------------------------------------------------------
def E_distance(E, want):
    """max |E -+ want|: an essential matrix is defined up to its sign."""
    return min(np.abs(E - want).max(), np.abs(E + want).max())


def zs_relerr(zs1, zs2, uvs1, uvs2, K1, K2, R, t, rows):
    """Largest relative distance of zs1 / zs2 at ``rows`` from the exact least-squares depths under (R, t, K)."""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, np.asarray(t).reshape(3)
    e1, e2 = sr.triangulate_exact(uvs1[rows], uvs2[rows], K1, K2, T)
    return max(sr.relerr(zs1[rows], e1), sr.relerr(zs2[rows], e2))


def exact_mean(z):
    """(mean, mean of |z|) of float64 values as Fractions."""
    f = [Fraction(float(v)) for v in z]
    return sum(f) / len(f), sum(abs(v) for v in f) / len(f)


def reduction_shape(n):
    """(m, d) of the fixed-order sums as include/calibrating_amd.h documents them: G = clamp(ceil(n / 256), 1, 1024)
    workgroups, a thread adds at most m = ceil(n / (256 G)) terms serially, d = 8 + 2 + 8 tree levels above that."""
    G = min(max(-(-n // 256), 1), 1024)
    return -(-n // (256 * G)), 18


def rectified_v(st, X1, R_true=None, t_true=None):
    """v of scene points (camera 1's frame) in the two rectified cameras of the rig ``st``: camera 1 sees X1 turned by
    R1, camera 2 sees R X1 + t turned by R2.  Without ``R_true, t_true`` camera 2 stands where the RIG says it stands
    (the rig's own R, t: do its rectifying rotations line the rows of its own two cameras up?); with them it stands
    where it truly stood when the matches were taken (what the estimated rig does to real observations)."""
    X1 = np.asarray(X1, np.float64)
    R, t = (st.R, st.t) if R_true is None else (R_true, t_true)
    p1 = X1 @ st.R1.T @ st.K.T
    p2 = (X1 @ np.asarray(R, np.float64).T + np.asarray(t, np.float64).reshape(3)) @ st.R2.T @ st.K.T
    return p1[:, 1] / p1[:, 2], p2[:, 1] / p2[:, 2]
