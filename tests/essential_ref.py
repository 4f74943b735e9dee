"""NumPy restatement of the RANSAC 8-point estimator (csrc/essential.hip, epipolar_geometry.find_essential_matrix), in the
kernels' operation order: float64 products and sums rounded one by one, division and square root correctly rounded on
both sides, so samples, matrices, counts, masks and moments are compared with the device bit for bit.  Everything is
vectorised over the hypotheses (an elementwise NumPy operation rounds each element as the scalar one does).  Test
infrastructure only."""
import numpy as np

from calibrating_amd.boards import _splitmix64

M64 = (1 << 64) - 1
MAX_REDRAWS = 1024    # ESS_MAX_REDRAWS
NULL_PIVOT = 1e-10    # ESS_NULL_PIVOT
SUMS = 46             # ESS_SUMS


def _d(i, j):
    """where entry (i, j), j <= i, of a packed lower triangle lies"""
    return i * (i + 1) // 2 + j


# ---- stage 1 ------------------------------------------------------------------------------------------------------------
def sample(seed, h, n):
    """the 8 distinct rows hypothesis h draws"""
    _, key = _splitmix64(int(seed) & M64)
    _, state = _splitmix64(key ^ h)  # the stream starts at the generator's OUTPUT
    idx = []
    for _ in range(8):
        c, dup, tries = 0, True, 0
        while dup and tries < MAX_REDRAWS:
            state, z = _splitmix64(state)
            c = (z * n) >> 64
            dup, tries = c in idx, tries + 1
        if dup:
            c = min(set(range(9)) - set(idx))
        idx.append(c)
    return idx


def samples(seed, hypotheses, n):
    return np.array([sample(seed, h, n) for h in range(hypotheses)], np.int32)


def rays(uvs, K):
    """(u, v, 1) @ inv(K).T as the kernels round it: (k0 u + k1 v) + k2"""
    k = np.linalg.inv(np.asarray(K, np.float64)[:3, :3]).reshape(9)
    u, v = np.asarray(uvs)[:, 0].astype(np.float64), np.asarray(uvs)[:, 1].astype(np.float64)
    return np.stack([(k[3 * r] * u + k[3 * r + 1] * v) + k[3 * r + 2] for r in range(3)], -1)


def rows(a, b):
    """the rows of the 8-point system: row[3 j + k] = a[k] * b[j]"""
    return np.stack([a[..., k] * b[..., j] for j in range(3) for k in range(3)], -1)


def normal_matrices(r):
    """(H, 45) packed sum of row^T row over the 8 rows of every hypothesis, in the order drawn.  r: (H, 8, 9)"""
    M = np.zeros((r.shape[0], 45))
    for k in range(8):
        for p in range(9):
            for q in range(p + 1):
                M[:, _d(p, q)] = M[:, _d(p, q)] + r[:, k, p] * r[:, k, q]
    return M


def null_vector(M):
    """null_vector<9> of pnp_common.hpp on (H, 45) packed matrices -> (v (H, 9), ok (H,), the Cholesky factor (H, 45), trace)"""
    N, M = 9, M.copy()
    with np.errstate(all="ignore"):
        trace = np.zeros(M.shape[0])
        for q in range(N):
            trace = trace + M[:, _d(q, q)]
        mu = 1e-13 * trace
        for q in range(N):
            M[:, _d(q, q)] = M[:, _d(q, q)] + mu
        v = np.stack([np.full(M.shape[0], 1. + 0.25 * q) for q in range(N)], 1)
        ok = np.ones(M.shape[0], bool)
        for j in range(N):  # cholesky<9>
            d = M[:, _d(j, j)].copy()
            for q in range(j):
                d = d - M[:, _d(j, q)] * M[:, _d(j, q)]
            ok &= (d > 0) & np.isfinite(d)
            root = np.sqrt(d)
            ir = 1. / root
            M[:, _d(j, j)] = root
            for i in range(j + 1, N):
                s = M[:, _d(i, j)].copy()
                for q in range(j):
                    s = s - M[:, _d(i, q)] * M[:, _d(j, q)]
                M[:, _d(i, j)] = s * ir
        for _ in range(6):
            for i in range(N):  # cholesky_solve<9>
                s = v[:, i].copy()
                for q in range(i):
                    s = s - M[:, _d(i, q)] * v[:, q]
                v[:, i] = s / M[:, _d(i, i)]
            for i in range(N - 1, -1, -1):
                s = v[:, i].copy()
                for q in range(i + 1, N):
                    s = s - M[:, _d(q, i)] * v[:, q]
                v[:, i] = s / M[:, _d(i, i)]
            s = np.zeros(M.shape[0])
            for q in range(N):
                s = s + v[:, q] * v[:, q]
            s = 1. / np.sqrt(s)
            v = v * s[:, None]
        ok &= np.isfinite(v).all(1)
    return v, ok, M, trace


def hypotheses(uvs1, uvs2, K1, K2, n_hypotheses, seed):
    """(samples (H, 8) int32, Es (H, 9)): a marked hypothesis is all zero"""
    a, b = rays(uvs1, K1), rays(uvs2, K2)
    idx = samples(seed, n_hypotheses, len(a))
    v, ok, L, trace = null_vector(normal_matrices(rows(a[idx], b[idx])))
    with np.errstate(all="ignore"):
        tiny = sum((L[:, _d(q, q)] * L[:, _d(q, q)] < NULL_PIVOT * trace).astype(int) for q in range(9))
        ok = ok & (tiny <= 1)
        big = v[:, 0].copy()
        for q in range(1, 9):
            big = np.where(np.abs(v[:, q]) > np.abs(big), v[:, q], big)
        v = np.where((big < 0)[:, None], -v, v)
    return idx, np.where(ok[:, None], v, 0.)


# ---- stage 2 ------------------------------------------------------------------------------------------------------------
def inliers(e, a, b, thr2):
    """(..., n) bool: e (..., 9) broadcast against the rays (n, 3)"""
    e = np.asarray(e, np.float64)[..., None, :]
    with np.errstate(all="ignore"):
        p = [(e[..., 3 * r] * a[:, 0] + e[..., 3 * r + 1] * a[:, 1]) + e[..., 3 * r + 2] * a[:, 2] for r in range(3)]
        q = [(e[..., c] * b[:, 0] + e[..., 3 + c] * b[:, 1]) + e[..., 6 + c] * b[:, 2] for c in range(2)]
        num = (b[:, 0] * p[0] + b[:, 1] * p[1]) + b[:, 2] * p[2]
        den = ((p[0] * p[0] + p[1] * p[1]) + q[0] * q[0]) + q[1] * q[1]
        return num * num < thr2 * den


def score(Es, a, b, thr2):
    """(counts (H,) int32, the winner's index): the largest count, ties to the lowest index"""
    counts = np.concatenate([inliers(Es[s:s + 64], a, b, thr2).sum(-1) for s in range(0, len(Es), 64)]).astype(np.int32)
    return counts, int(np.argmax(counts))


# ---- stage 3 ------------------------------------------------------------------------------------------------------------
def moments(e, a, b, thr2):
    """(mask (n,) bool, sums (46,)) in the reduction shape of camd_essential_moments"""
    n = len(a)
    on = inliers(np.asarray(e, np.float64).reshape(9), a, b, thr2)
    r = rows(a, b)
    terms = np.stack([r[:, p] * r[:, q] for p in range(9) for q in range(p + 1)] + [np.ones(n)], 1)
    terms = np.where(on[:, None], terms, 0.)
    G = min(max(-(-n // 256), 1), 1024)
    m = -(-n // (256 * G))
    padded = np.zeros((m * G * 256, SUMS))
    padded[:n] = terms
    padded = padded.reshape(m, G, 256, SUMS)
    s = np.zeros((G, 256, SUMS))
    for k in range(m):  # a thread's rows, in order
        s = s + padded[k]

    def tree(x):  # block_tree: sh[t] += sh[t + o], o = 128 .. 1
        o = 128
        while o:
            x = x[..., :o, :] + x[..., o:2 * o, :]
            o >>= 1
        return x[..., 0, :]

    partials = np.zeros((1024, SUMS))
    partials[:G] = tree(s)
    p = partials.reshape(4, 256, SUMS)
    return on, tree((p[0] + p[1]) + (p[2] + p[3]))


# ---- the whole call --------------------------------------------------------------------------------------------------
def force_rank2(E):
    U, S, Vt = np.linalg.svd(E)
    S[2] = 0
    return np.dot(U, np.dot(np.diag(S), Vt))


def refit(sums):
    """the smallest eigenvector of the moment matrix, its largest entry positive, forced to rank 2"""
    M = np.zeros((9, 9))
    M[np.tril_indices(9)] = sums[:45]
    v = np.linalg.eigh(M, UPLO="L")[1][:, 0]
    v = -v if v[np.argmax(np.abs(v))] < 0 else v
    return force_rank2(v.reshape(3, 3))


def ray_threshold2(K1, K2, threshold):
    K1 = np.asarray(K1, np.float64)
    K2 = K1 if K2 is None else np.asarray(K2, np.float64)
    thr = float(threshold) / ((K1[0, 0] + K1[1, 1] + K2[0, 0] + K2[1, 1]) / 4)
    return thr * thr


def find(uvs1, uvs2, K1, K2=None, threshold=1.0, n_hypotheses=1024, seed=0, refine=True, Es=None):
    """find_essential_matrix(..., return_info=True), plus ``samples, Es, counts``.  ``Es``: matrices to score instead of
    stage 1's own (the device's, when the later stages are compared)."""
    K2 = K1 if K2 is None else K2
    a, b, thr2 = rays(uvs1, K1), rays(uvs2, K2), ray_threshold2(K1, K2, threshold)
    idx, own = hypotheses(uvs1, uvs2, K1, K2, n_hypotheses, seed)
    Es = own if Es is None else np.asarray(Es, np.float64)
    counts, h = score(Es, a, b, thr2)
    count = int(counts[h])
    info = dict(samples=idx, Es=Es, counts=counts, hypothesis=h, hypothesis_inliers=count, refined=False,
                status="ok" if count else "degenerate")
    if not count:
        info.update(E=np.zeros((3, 3)), n_inliers=0, inliers=np.zeros(len(a), bool))
        return info
    E = force_rank2(Es[h].reshape(3, 3))
    mask, sums = moments(Es[h], a, b, thr2)
    info.update(hypothesis_mask=mask, hypothesis_sums=sums)
    if refine:
        E_fit = refit(sums)
        mask_fit, sums_fit = moments(E_fit, a, b, thr2)
        if int(sums_fit[45]) >= count:
            E, mask, count, info["refined"] = E_fit, mask_fit, int(sums_fit[45]), True
    info.update(E=E, n_inliers=count, inliers=mask)
    return info


# ---- yardsticks --------------------------------------------------------------------------------------------------------
def candidates(E):
    """the four (R, t) of an essential matrix (float64 throughout, t of unit length)"""
    U, _, Vt = np.linalg.svd(E)
    W = np.array([[0., -1, 0], [1, 0, 0], [0, 0, 1]])
    out = []
    for Wk in (W, W.T):
        R = U @ Wk @ Vt
        R = -R if np.linalg.det(R) < 0 else R
        out += [(R, U[:, 2]), (R, -U[:, 2])]
    return out


def pose_error(E, R_true, t_true):
    """(rotation angle, angle between the translation directions) in radians of the candidate of E nearest the truth"""
    t_true = np.asarray(t_true, np.float64) / np.linalg.norm(t_true)
    best = None
    for R, t in candidates(E):
        rot = np.arccos(np.clip((np.trace(R @ np.asarray(R_true).T) - 1) / 2, -1, 1))
        tdir = np.arccos(np.clip(t @ t_true, -1, 1))
        if best is None or rot + tdir < sum(best):
            best = (float(rot), float(tdir))
    return best


def true_E(R, t):
    t = np.asarray(t, np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ np.asarray(R, np.float64)


def angle9(u, v):
    """the angle between two 9-vectors, up to sign"""
    u, v = np.asarray(u, np.float64).ravel(), np.asarray(v, np.float64).ravel()
    c = abs(u @ v) / (np.linalg.norm(u) * np.linalg.norm(v))
    s = np.linalg.norm(u / np.linalg.norm(u) - np.sign(u @ v) * v / np.linalg.norm(v))
    return float(s if c > 0.5 else np.arccos(min(c, 1.0)))
