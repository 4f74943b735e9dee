"""A rig's pose from matched points on the GPU -- same names and argument meanings as the reference's
``epipolar_geometry.py`` (``EssentialMatrixStereo``, ``filter_overlap_uvs``, ``matching_uvs_in_one_img``), ``flow_utils``
(``flow_abs_to_normal`` / ``flow_normal_to_abs``) and the flow-to-matches step of
``ReconstructionExtrinsics.build_set2ds_by_flowds`` (reconstruction_epipolar_geometry.py:256-295).  NumPy in -> NumPy out,
torch CUDA tensors in -> tensors out on the same device (csrc/epipolar.hip; DESIGN.md "Epipolar path").

Where the work runs.  Everything that touches every match or every pixel is a kernel: the cell grids and their
intersection, the overlap filter, the depth of every match under all four candidate poses, the gathered means, the flow
compaction and conversions.  The essential matrix itself is an SVD of at most 199 x 9 numbers (the reference subsamples
``[:: n // 100]``) followed by 3 x 3 algebra: init-time work on the host in NumPy float64, fed with the strided subsample
only.  ``find_essential_matrix`` / ``EssentialMatrixStereo(robust=...)`` is the opt-in estimate for matches that hold
wrong pairs: RANSAC over 8-point samples, every hypothesis scored against every match on the device (csrc/essential.hip);
``find_essential_matrices`` is the same estimate for every pair of a batch in one pass, bit for bit.

Arguments are checked before the device is touched.  Deviations from the reference:
``precise=True`` is refused, ``xy1`` / ``xy2`` are required, non-finite coordinates and cell windows beyond 2^28 cells
raise ``ValueError``.
"""
import numpy as np

from . import _native, geometry, hostio
from ._arrays import FLOAT_TYPES, Kinv9, check_array, dtype_name, is_np, mat, to_caller, to_device
from ._native import call
from .sparse import matched_uvs_to_zs  # noqa: F401  (also a re-export)
from .stereo_camera import Stereo

MAX_CELLS = 1 << 28  # the most one cell window may hold: two uint32 grids of it are 2 GiB
# the most cells all grids of one pass of matching_uvs_in_one_img_batch hold together (uint32 each: 512 MiB); beyond it
# the pairs are worked off in several passes
BATCH_MAX_CELLS = 1 << 27


def _float_rows(a, what, other=None):
    """(n, 2) rows as they take part in NumPy's arithmetic: float32 stays, everything else becomes float64."""
    check_array(a, what)
    if len(a.shape) != 2 or a.shape[1] != 2:
        raise ValueError("%s must be (n, 2), got %s" % (what, tuple(a.shape)))
    if int(a.shape[0]) >= 2 ** 32 - 1:
        raise ValueError("%s: %d rows do not fit the 32-bit row index" % (what, a.shape[0]))
    if other is not None and is_np(a) != is_np(other):
        raise TypeError("%s: pass both point sets as ndarrays or both as CUDA tensors" % what)
    return "float32" if dtype_name(a) == "float32" else "float64"


def _min_max(a):
    """[min u, min v, max u, max v] as float64 on the host.  Tensors are reduced on the device and four numbers read back.
    ndarrays are reduced on the host BEFORE they are uploaded: non-finite input and an oversized window are then refused
    without touching the device (one pass over host memory that a device-resident caller does not pay)."""
    if is_np(a):
        return np.concatenate([a.min(0), a.max(0)]).astype(np.float64)
    import torch
    return torch.cat([a.amin(0), a.amax(0)]).to(torch.float64).cpu().numpy()


def _window(bounds, what, hint):
    """(cu0, cv0, cells_w, cells_h) holding the rounded ``bounds`` = rows of [min u, min v, max u, max v] cells."""
    b = np.asarray(bounds, np.float64)
    if not np.isfinite(b).all():
        raise ValueError("%s: u, v must be finite" % what)
    lo, hi = np.rint(b[:, :2]).min(0), np.rint(b[:, 2:]).max(0)
    if lo.min() < -2 ** 31 or hi.max() >= 2 ** 31 - 1:
        raise ValueError("%s: cells leave the int32 range%s" % (what, hint))
    cw, ch = (int(v) for v in hi - lo + 1)
    if cw * ch > MAX_CELLS:
        raise ValueError("%s: the points span %d x %d cells, more than 2^28%s" % (what, cw, ch, hint))
    return int(lo[0]), int(lo[1]), cw, ch


# ---- small helpers -----------------------------------------------------------------------------------------------------
def uvs_to_xyz_noramls(uvs, K):
    """Rays (x, y, 1) of pixels: ``(u, v, 1) @ inv(K).T`` (epipolar_geometry.py:84-85; the spelling is the reference's)."""
    Kinv_T = np.linalg.inv(np.asarray(K)).T
    if is_np(uvs):
        return np.pad(uvs, ((0, 0), (0, 1)), constant_values=1) @ Kinv_T
    import torch
    check_array(uvs, "uvs")
    ones = torch.ones((uvs.shape[0], 1), dtype=uvs.dtype, device=uvs.device)
    return torch.cat([uvs, ones], 1).to(torch.float64) @ torch.from_numpy(np.ascontiguousarray(Kinv_T, np.float64)).to(uvs.device)


uvs_to_xyz_normals = uvs_to_xyz_noramls


def compute_essential_matrix(xyzs1, xyzs2):
    """Eight-point essential matrix of matched rays (:12-43), host NumPy float64: every ``n // 100``-th pair when there
    are more than 100, the null vector of the n x 9 system by SVD, then the smallest singular value forced to 0."""
    xyzs1, xyzs2 = np.asarray(xyzs1), np.asarray(xyzs2)
    if xyzs1.shape != xyzs2.shape:
        raise ValueError("the two point sets must have the same shape, got %s and %s" % (xyzs1.shape, xyzs2.shape))
    n = xyzs1.shape[0]
    if n < 8:
        raise ValueError("at least 8 point pairs are required, got %d" % n)
    if n > 100:
        xyzs1, xyzs2 = xyzs1[:: n // 100], xyzs2[:: n // 100]
    (x1, y1, z1), (x2, y2, z2) = xyzs1.T[:3], xyzs2.T[:3]
    A = np.stack([x1 * x2, x2 * y1, z1 * x2, x1 * y2, y1 * y2, z1 * y2, x1 * z2, y1 * z2, z1 * z2], 1).astype(np.float64)
    return _force_rank2(np.linalg.svd(A)[2][-1].reshape(3, 3))


def _force_rank2(E):
    """``E`` with its smallest singular value set to 0 (:39-43)."""
    U, S, Vt = np.linalg.svd(E)
    S[2] = 0
    return np.dot(U, np.dot(np.diag(S), Vt))


def decompose_essential_matrix(E):
    """The four candidate poses of an essential matrix as 4x4 ``T_1to2`` (:46-62), in the reference's order: (Ra, +u),
    (Rb, -u), (Ra, -u), (Rb, +u) with u the last left singular vector and Ra / Rb = U W Vt / U W^T Vt, each made a proper
    rotation.  Like the reference's ``R_t_to_T`` the rotations are rounded through float32.  (The products keep the
    reference's association, U (W Vt): the candidates are compared with its numbers.)"""
    U, _, Vt = np.linalg.svd(E)
    quarter_turn = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
    rotations = []
    for W in (quarter_turn, quarter_turn.T):
        R = np.dot(U, np.dot(W, Vt))
        rotations.append(-R if np.linalg.det(R) < 0 else R)
    u = U[:, 2]
    order = ((0, u), (1, -u), (0, -u), (1, u))
    return tuple(geometry.R_t_to_T(rotations[k], t) for k, t in order)


def _host_subsample(uvs, n):
    """Every ``n // 100``-th row (all of them up to 100) on the host: the only rows the essential matrix reads."""
    rows = uvs[:: n // 100] if n > 100 else uvs
    return rows if is_np(rows) else rows.cpu().numpy()


def _pose_candidates(uvs1, uvs2, K1, K2, baseline):
    """(E, four T_1to2 with |t| = baseline) from the host subsample of the matches."""
    n = int(uvs1.shape[0])
    E = compute_essential_matrix(uvs_to_xyz_noramls(_host_subsample(uvs1, n), K1),
                                 uvs_to_xyz_noramls(_host_subsample(uvs2, n), K2))
    return E, _scaled_candidates(E, baseline)


def _scaled_candidates(E, baseline):
    """The four ``T_1to2`` of ``E`` with |t| = baseline."""
    Ts = decompose_essential_matrix(E)
    for T in Ts:
        T[:3, 3] *= baseline / np.linalg.norm(T[:3, 3])
    return Ts


def _candidate_means(a, b, K1, K2, Ts):
    """(4, 2) mean zs1 / zs2 of the matches under each candidate: one pass over device-resident (n, 2) float64 rows."""
    import torch
    n = int(a.shape[0])
    Kinv = [Kinv9(K) for K in (K1, K2)]
    T4 = mat(np.stack(Ts), 64)
    partials = torch.empty(_native.lib().camd_epipolar_sums_blocks(n) * 8, dtype=torch.float64, device=a.device)
    sums = torch.empty(8, dtype=torch.float64, device=a.device)
    call("camd_epipolar_sums", a.device, a.data_ptr(), b.data_ptr(), n, Kinv[0].ctypes.data, Kinv[1].ctypes.data, T4.ctypes.data,
         partials.data_ptr(), sums.data_ptr(), what="EssentialMatrixStereo")
    return sums.cpu().numpy().reshape(4, 2) / n


def _mean(z, idx=None, what="mean"):
    """``z.mean()`` / ``z[idx].mean()`` of a float64 vector through the fixed-order reduction (one number read back)."""
    import torch
    zd = to_device(z, dtype="float64", cast=True)
    lib = _native.lib()
    n = int(zd.shape[0]) if idx is None else int(idx.shape[0])
    if n == 0:
        raise ValueError("%s of no elements" % what)
    i = None if idx is None else to_device(idx, dtype="int64", cast=True, device=zd.device)
    partials = torch.empty(lib.camd_vector_sum_blocks(n) * 2, dtype=torch.float64, device=zd.device)
    sums = torch.empty(2, dtype=torch.float64, device=zd.device)
    call("camd_vector_sum", zd.device, zd.data_ptr(), int(zd.shape[0]), None if i is None else i.data_ptr(), n,
         partials.data_ptr(), sums.data_ptr(), what=what)
    total, bad = sums.cpu().numpy()
    if bad:
        raise IndexError("%s: %d indices lie outside the %d depths" % (what, int(bad), int(zd.shape[0])))
    return float(total) / n


# ---- find_essential_matrix: RANSAC over 8-point samples (csrc/essential.hip) ---------------------------------------------
ESSENTIAL_MAX_HYPOTHESES = 1 << 20  # (ESS_MAX_HYPOTHESES)


class _EssentialRows:
    """The matches as the three stages take them: device rows read in place (type, row strides), inv(K1), inv(K2)."""

    def __init__(self, uvs1, uvs2, K1, K2):
        self.was_np = is_np(uvs1)
        self.uv1, self.stride1 = self._in_place(to_device(uvs1) if self.was_np else uvs1)
        self.device = self.uv1.device
        if self.was_np:
            uvs2 = to_device(uvs2, device=self.device)
        elif uvs2.device != self.device:
            raise ValueError("inputs live on different devices: %s and %s" % (uvs2.device, self.device))
        self.uv2, self.stride2 = self._in_place(uvs2)
        self.n, self.type = int(uvs1.shape[0]), FLOAT_TYPES[dtype_name(uvs1)]
        self.k1, self.k2 = Kinv9(K1), Kinv9(K2)

    @staticmethod
    def _in_place(t):
        """(tensor, row stride in elements): a view whose rows are u, v side by side is read where it lies."""
        if t.stride(1) == 1 and 2 <= t.stride(0) < 2 ** 31:
            return t, int(t.stride(0))
        return t.contiguous(), 2

    def args(self):
        return (self.uv1.data_ptr(), self.uv2.data_ptr(), self.type, self.n, self.stride1, self.stride2, self.k1.ctypes.data,
                self.k2.ctypes.data)


def _essential_hypotheses(rows, hypotheses, seed):
    """Stage 1 alone: (samples (H, 8) int32, Es (H, 9) float64) on the device."""
    import torch
    samples = torch.empty((hypotheses, 8), dtype=torch.int32, device=rows.device)
    Es = torch.empty((hypotheses, 9), dtype=torch.float64, device=rows.device)
    call("camd_essential_hypotheses", rows.device, *rows.args(), int(seed) & 0xFFFFFFFFFFFFFFFF, hypotheses, samples.data_ptr(),
         Es.data_ptr(), what="find_essential_matrix")
    return samples, Es


def _essential_score(rows, Es, threshold2):
    """Stage 2 alone: (counts (H,) int32, winner (11,) float64 = the winning e, its index, its count) on the device."""
    import torch
    Es = to_device(Es, dtype="float64", device=rows.device)
    hypotheses = int(Es.shape[0])
    counts = torch.empty(hypotheses, dtype=torch.int32, device=rows.device)
    winner = torch.empty(11, dtype=torch.float64, device=rows.device)
    call("camd_essential_score", rows.device, *rows.args(), Es.data_ptr(), hypotheses, float(threshold2), counts.data_ptr(),
         winner.data_ptr(), what="find_essential_matrix")
    return counts, winner


def _essential_moments(rows, E, threshold2):
    """Stage 3 alone for one ``E`` (9 float64 on the device, or a host array that is uploaded): (mask (n,) uint8, sums (46,)
    float64 = the packed lower triangle of sum a^T a over the inliers, then their number) on the device."""
    import torch
    E = to_device(np.ascontiguousarray(E, np.float64).reshape(9) if is_np(E) else E, dtype="float64", device=rows.device)
    mask = torch.empty(rows.n, dtype=torch.uint8, device=rows.device)
    partials = torch.empty(_native.lib().camd_essential_moments_blocks(rows.n) * 46, dtype=torch.float64, device=rows.device)
    sums = torch.empty(46, dtype=torch.float64, device=rows.device)
    call("camd_essential_moments", rows.device, *rows.args(), E.data_ptr(), float(threshold2), mask.data_ptr(), partials.data_ptr(),
         sums.data_ptr(), what="find_essential_matrix")
    return mask, sums


def _positive_largest(v):
    """``v`` with the sign that makes its entry of the largest magnitude (the first of equals) positive."""
    return -v if v[np.argmax(np.abs(v))] < 0 else v


def _essential_checks(uvs1, uvs2, K1, K2, threshold, hypotheses):
    """Every refusal of find_essential_matrix that needs no device -> (K1, K2, threshold on the rays)."""
    _float_rows(uvs1, "uvs1")
    _float_rows(uvs2, "uvs2", uvs1)
    if dtype_name(uvs1) not in FLOAT_TYPES or dtype_name(uvs2) != dtype_name(uvs1):
        raise ValueError("uvs1, uvs2 must both be float64 or both float32, got %s and %s" % (dtype_name(uvs1), dtype_name(uvs2)))
    n = int(uvs1.shape[0])
    if int(uvs2.shape[0]) != n or not 8 <= n < 2 ** 31:
        raise ValueError("uvs1, uvs2 must hold the same number (8 .. 2^31 - 1) of matches, got %d and %d" % (n, uvs2.shape[0]))
    K1 = np.asarray(K1, np.float64)
    K2 = K1 if K2 is None else np.asarray(K2, np.float64)
    if K1.shape != (3, 3) or K2.shape != (3, 3):
        raise ValueError("K1, K2 must be 3x3")
    if not (np.isfinite(K1).all() and np.isfinite(K2).all()):
        raise ValueError("K1, K2 must be finite")
    focal = (K1[0, 0] + K1[1, 1] + K2[0, 0] + K2[1, 1]) / 4
    if not focal > 0 or min(abs(np.linalg.det(K1)), abs(np.linalg.det(K2))) == 0:
        raise ValueError("K1, K2 must be invertible camera matrices with a positive mean focal length")
    if int(hypotheses) != hypotheses or not 1 <= int(hypotheses) <= ESSENTIAL_MAX_HYPOTHESES:
        raise ValueError("hypotheses must be an integer in 1 .. 2^20, got %r" % (hypotheses,))
    if not (float(threshold) > 0 and np.isfinite(float(threshold))):
        raise ValueError("threshold must be a positive number of pixels, got %r" % (threshold,))
    if is_np(uvs1) and not (np.isfinite(uvs1).all() and np.isfinite(uvs2).all()):
        raise ValueError("find_essential_matrix: u, v must be finite")
    return K1, K2, float(threshold) / focal


def find_essential_matrix(uvs1, uvs2, K1, K2=None, threshold=1.0, hypotheses=1024, seed=0, refine=True, return_info=False):
    """The essential matrix of matched pixels that holds against wrong matches: RANSAC over 8-point samples on the GPU
    (csrc/essential.hip), a contract of this package's own -- ``cv2.findEssentialMat`` is not restated.  ``uvs1, uvs2``:
    (n, 2) pinhole pixels, both float32 or both float64, ndarrays or CUDA tensors (read in place, a view with rows
    ``u, v`` side by side included), n >= 8, finite.  Returns ``E`` (3, 3) host float64 of rank 2 with
    ``ray2 @ E @ ray1 = 0`` on the rays ``(u, v, 1) @ inv(K).T``; with ``return_info=True`` the dict ``E, inliers ((n,)
    bool of the caller's kind), n_inliers, hypothesis (the index of the winning sample), hypothesis_inliers (its count),
    refined, status`` ("ok", or "degenerate" when no sample determined a matrix: ``E`` is then all zero).

    A match is an inlier when its squared Sampson error on the rays is below ``(threshold / f)^2``, ``threshold`` in
    pixels and ``f`` the mean of fx1, fy1, fx2, fy2 (evaluated as ``num^2 < thr^2 den``; include/calibrating_amd.h has the
    order of the operations).

    1  Hypothesis ``h`` of ``hypotheses`` draws 8 distinct matches from ``boards._splitmix64``: ``key`` is the generator's
       output from the state ``seed``; the hypothesis' own stream starts at the state that is the generator's OUTPUT from
       the state ``key ^ h``; a draw is ``(z * n) >> 64`` of the stream's next output ``z`` (multiply-high), made again from
       the same stream while it repeats an earlier draw of the hypothesis.  No state is shared: hypothesis ``h`` draws the
       same matches and gives the same matrix whatever ``hypotheses`` is.  Its matrix is the null vector of the 8 x 9
       system in the reference's row layout; a sample that leaves more than one null direction is marked and scores 0.
    2  Every hypothesis is scored against every match; the largest count wins, ties go to the lowest index.
    3  ``refine=True``: the smallest eigenvector (``np.linalg.eigh``, 9 x 9) of the moment matrix of ALL inliers of the
       winner, forced to rank 2 and scored once more, replaces the winner when it has at least as many inliers;
       otherwise, and with ``refine=False``, the winner's matrix forced to rank 2 is returned.  ``inliers`` belong to the
       matrix that was scored: the refit's, or the winner's before its rank was forced.

    The same input and seed give the same bits on every run.  Every refusal (``ValueError``) comes before a kernel of the
    estimator is queued; for tensors the finite check is one reduction on the device."""
    import torch
    K1, K2, thr = _essential_checks(uvs1, uvs2, K1, K2, threshold, hypotheses)
    if not is_np(uvs1) and not (bool(torch.isfinite(uvs1).all()) and bool(torch.isfinite(uvs2).all())):
        raise ValueError("find_essential_matrix: u, v must be finite")
    rows, thr2 = _EssentialRows(uvs1, uvs2, K1, K2), thr * thr
    _, Es = _essential_hypotheses(rows, int(hypotheses), seed)
    _, winner = _essential_score(rows, Es, thr2)
    won = winner.cpu().numpy()  # synchronises: the one read-back of the search
    E_won, h, count = won[:9].reshape(3, 3), int(won[9]), int(won[10])
    info = dict(hypothesis=h, hypothesis_inliers=count, refined=False, status="ok" if count else "degenerate")
    if not count:
        mask = torch.zeros(rows.n, dtype=torch.bool, device=rows.device)
        info.update(E=np.zeros((3, 3)), n_inliers=0, inliers=to_caller(mask, rows.was_np))
        return info if return_info else info["E"]
    E = _force_rank2(E_won)
    if refine or return_info:
        mask, sums = _essential_moments(rows, winner[:9], thr2)
    if refine:
        M = np.zeros((9, 9))
        M[np.tril_indices(9)] = sums[:45].cpu().numpy()
        E_fit = _force_rank2(_positive_largest(np.linalg.eigh(M, UPLO="L")[1][:, 0]).reshape(3, 3))
        mask_fit, sums_fit = _essential_moments(rows, E_fit, thr2)
        if int(sums_fit[45].item()) >= count:
            E, mask, info["refined"] = E_fit, mask_fit, True
            count = int(sums_fit[45].item())
    if not return_info:
        return E
    info.update(E=E, n_inliers=count, inliers=to_caller(mask != 0, rows.was_np))
    return info


# ---- find_essential_matrices: every pair of a batch in one pass -----------------------------------------------------------
ESSENTIAL_SCORE_ROWS = 1024  # rows a workgroup of the batch's score kernel owns (256 * ESS_SCORE_ROWS)
ESSENTIAL_LDS_SUM = True  # the score kernel adds the four waves' counts in LDS (DESIGN.md has the timing of both)
STATUS_OK, STATUS_DEGENERATE, STATUS_TOO_FEW = 0, 1, 2


def essential_moments_blocks(n):
    """``camd_essential_moments_blocks(n)`` without the library: clamp(ceil(n / 256), 1, 1024)."""
    return min(max(-(-int(n) // 256), 1), 1024)


def essential_score_blocks(counts):
    """The score kernel's block table, counts in, table out: ``(B, 4)`` int32 rows ``(pair, g, G, 0)`` -- workgroup ``g`` of the
    pair's ``G`` owns the pair's rows ``1024 g .. 1024 g + 1023`` -- for the pairs of at least 8 rows, pairs in order.  No
    block names two pairs; every row of such a pair lies in exactly one block."""
    table = []
    for p, n in enumerate(int(c) for c in counts):
        if n >= 8:
            G = -(-n // ESSENTIAL_SCORE_ROWS)
            table += [(p, g, G, 0) for g in range(G)]
    return np.array(table, np.int32).reshape(-1, 4)


def essential_moments_tables(counts, take):
    """The moments launch's two tables for the pairs ``take`` marks: blocks ``(B, 4)`` int32 ``(pair, g, G, 0)`` with ``G =
    essential_moments_blocks(rows of the pair)`` -- thread ``t`` of workgroup ``g`` adds the pair's rows ``256 g + t, + 256 G,
    ...`` -- and finals ``(F, 4)`` ``(pair, the pair's first block, G, 0)``."""
    blocks, finals = [], []
    for p, n in enumerate(int(c) for c in counts):
        if take[p]:
            G = essential_moments_blocks(n)
            finals.append((p, len(blocks), G, 0))
            blocks += [(p, g, G, 0) for g in range(G)]
    return np.array(blocks, np.int32).reshape(-1, 4), np.array(finals, np.int32).reshape(-1, 4)


def _essential_batch_checks(K, pairs, uvs_a, uvs_b, counts, threshold, hypotheses):
    """Every refusal of find_essential_matrices that needs no device -> (pairs (P, 2) int64, counts (P,) int64, the pair
    table's host part (P, 21) float64 without the row columns: inv(K_a), inv(K_b), threshold2 on the rays)."""
    _float_rows(uvs_a, "uvs_a")
    _float_rows(uvs_b, "uvs_b", uvs_a)
    if dtype_name(uvs_a) not in FLOAT_TYPES or dtype_name(uvs_b) != dtype_name(uvs_a):
        raise ValueError("uvs_a, uvs_b must both be float64 or both float32, got %s and %s" % (dtype_name(uvs_a), dtype_name(uvs_b)))
    M = int(uvs_a.shape[0])
    if int(uvs_b.shape[0]) != M or M >= 2 ** 31:
        raise ValueError("uvs_a, uvs_b must hold the same number (below 2^31) of matches, got %d and %d" % (M, uvs_b.shape[0]))
    K = np.asarray(K, np.float64)
    if K.ndim != 3 or K.shape[1:] != (3, 3):
        raise ValueError("K must be (N, 3, 3), got %s" % (K.shape,))
    pairs = np.asarray(pairs)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
        raise ValueError("pairs must be (P, 2) integers, got shape %s dtype %s" % (pairs.shape, pairs.dtype))
    if pairs.shape[0] == 0:
        raise ValueError("find_essential_matrices needs at least one pair (P == 0)")
    pairs = pairs.astype(np.int64)
    if (pairs < 0).any() or (pairs >= K.shape[0]).any():
        raise ValueError("a pair names a view outside 0 .. %d" % (K.shape[0] - 1))
    if (pairs[:, 0] == pairs[:, 1]).any():
        raise ValueError("every pair (a, b) must have a != b")
    counts = np.asarray(counts)
    if counts.shape != (len(pairs),) or counts.dtype.kind not in "iu" or (counts < 0).any():
        raise ValueError("counts must be (P,) non-negative integers, got shape %s dtype %s" % (counts.shape, counts.dtype))
    counts = counts.astype(np.int64)
    if int(counts.sum()) != M:
        raise ValueError("counts sum to %d, uvs_a has %d rows" % (int(counts.sum()), M))
    named = np.unique(pairs)
    if not np.isfinite(K[named]).all():
        raise ValueError("K of every view a pair names must be finite")
    if (np.abs(np.linalg.det(K[named])) == 0).any():
        raise ValueError("K of every view a pair names must be an invertible camera matrix")
    Ka, Kb = K[pairs[:, 0]], K[pairs[:, 1]]
    focal = (Ka[:, 0, 0] + Ka[:, 1, 1] + Kb[:, 0, 0] + Kb[:, 1, 1]) / 4
    if not (focal > 0).all():
        raise ValueError("K1, K2 must be invertible camera matrices with a positive mean focal length")
    if int(hypotheses) != hypotheses or not 1 <= int(hypotheses) <= ESSENTIAL_MAX_HYPOTHESES:
        raise ValueError("hypotheses must be an integer in 1 .. 2^20, got %r" % (hypotheses,))
    if not (float(threshold) > 0 and np.isfinite(float(threshold))):
        raise ValueError("threshold must be a positive number of pixels, got %r" % (threshold,))
    if is_np(uvs_a) and not (np.isfinite(uvs_a).all() and np.isfinite(uvs_b).all()):
        raise ValueError("find_essential_matrices: u, v must be finite")
    inv_of = {int(v): Kinv9(K[v]) for v in named}
    table = np.zeros((len(pairs), 21))
    for p, (a, b) in enumerate(pairs):
        thr = float(threshold) / focal[p]
        table[p, 2:11], table[p, 11:20], table[p, 20] = inv_of[int(a)], inv_of[int(b)], thr * thr
    return pairs, counts, table


def _essential_batch_stages(uvs_a, uvs_b, counts, table, hypotheses, seed, lds_sum=None):
    """The search of every pair: device (samples (P, H, 8), Es (P, H, 9), counts (P, H), winner (P, 11)) and the call's ``batch``
    arguments; one launch per stage, nothing is read back."""
    import torch
    was_np = is_np(uvs_a)
    ua, stride_a = _EssentialRows._in_place(to_device(uvs_a) if was_np else uvs_a)
    dev = ua.device
    if not was_np and uvs_b.device != dev:
        raise ValueError("inputs live on different devices: %s and %s" % (uvs_b.device, dev))
    ub, stride_b = _EssentialRows._in_place(to_device(uvs_b, device=dev) if was_np else uvs_b)
    P, M = len(counts), int(ua.shape[0])
    table[:, 0:2].view(np.int64)[:] = np.stack([np.cumsum(counts) - counts, counts], 1)
    d_table = torch.from_numpy(table).to(dev)
    batch = (ua.data_ptr(), ub.data_ptr(), FLOAT_TYPES[dtype_name(ua)], M, stride_a, stride_b, d_table.data_ptr(), P)
    keep = (ua, ub, d_table)  # (alive while the launches are queued)
    samples = torch.empty((P, hypotheses, 8), dtype=torch.int32, device=dev)
    Es = torch.empty((P, hypotheses, 9), dtype=torch.float64, device=dev)
    call("camd_essential_batch_hypotheses", dev, *batch, int(seed) & 0xFFFFFFFFFFFFFFFF, hypotheses, samples.data_ptr(), Es.data_ptr(),
         what="find_essential_matrices")
    blocks = torch.from_numpy(essential_score_blocks(counts)).to(dev)
    hcounts = torch.empty((P, hypotheses), dtype=torch.int32, device=dev)
    winner = torch.empty((P, 11), dtype=torch.float64, device=dev)
    call("camd_essential_batch_score", dev, *batch, blocks.data_ptr(), int(blocks.shape[0]), Es.data_ptr(), hypotheses,
         int(ESSENTIAL_LDS_SUM if lds_sum is None else lds_sum), hcounts.data_ptr(), winner.data_ptr(), what="find_essential_matrices")
    return samples, Es, hcounts, winner, batch, keep


def _essential_batch_moments(batch, counts, take, E, E_stride):
    """Stage 3 of the pairs ``take`` marks, each with its matrix ``E[pair * E_stride ..]`` (device): (mask (M,) uint8, zero on
    the rows of the other pairs, sums (P, 46) float64) on the device."""
    import torch
    dev = E.device
    P, M = len(counts), batch[3]
    blocks, finals = (torch.from_numpy(t).to(dev) for t in essential_moments_tables(counts, take))
    mask = torch.zeros(M, dtype=torch.uint8, device=dev)
    partials = torch.empty((int(blocks.shape[0]), 46), dtype=torch.float64, device=dev)
    sums = torch.zeros((P, 46), dtype=torch.float64, device=dev)
    call("camd_essential_batch_moments", dev, *batch, blocks.data_ptr(), int(blocks.shape[0]), finals.data_ptr(), int(finals.shape[0]),
         E.data_ptr(), int(E_stride), mask.data_ptr(), partials.data_ptr(), sums.data_ptr(), what="find_essential_matrices")
    return mask, sums


def find_essential_matrices(K, pairs, uvs_a, uvs_b, counts, threshold=1.0, hypotheses=1024, seed=0, refine=True):
    """``find_essential_matrix`` for every pair of a batch in one pass: one launch per stage for all pairs and a constant
    number of read-backs (the winners, the winners' sums, the refits' sums; for tensors the finite check) instead of three
    per pair.  The argument layout is ``bundle_adjust_pairs``' own: ``K`` (N, 3, 3); ``pairs`` (P, 2) integers, ``a != b``
    (either order: ``uvs_a`` shows view ``pairs[p, 0]``); ``uvs_a`` / ``uvs_b`` (M, 2) pinhole pixels, both float32 or both
    float64, ndarrays or CUDA tensors read in place (a view with ``u, v`` side by side included); ``counts`` (P,) rows of
    each pair, the pairs' rows one after the other.

    -> ``dict(E (P, 3, 3) host float64, inliers (M,) bool of the caller's kind, n_inliers, hypothesis, hypothesis_inliers
    (P,) int64, refined (P,) bool, status (P,) int64)``.  ``status``: 0 ok; 1 degenerate (no sample determined a matrix:
    ``E`` zero, no inliers -- ``find_essential_matrix``'s ``"degenerate"``); 2 fewer than 8 rows, the empty pair included
    (``E`` zero, no inliers).  For every pair of status 0 or 1 every field equals, bit for bit, what
    ``find_essential_matrix(uvs_a[rows of p], uvs_b[rows of p], K[a], K[b], threshold, hypotheses, seed, refine,
    return_info=True)`` returns for that pair alone, whatever the other pairs are and wherever it stands: every pair uses
    the same ``seed``, its own ``threshold / f``, sample indices local to its rows, and its moments are summed in the single
    call's order; the rank-2 forcing and the refit's ``eigh`` (one call on the stacked moments) stay on the host.

    ``ValueError`` before the device is touched (for tensors after the one finite reduction): everything
    ``find_essential_matrix`` refuses per argument; ``pairs`` out of range or with ``a == b``; ``counts`` negative or not
    summing to M; ``M >= 2^31``; ``P == 0``; a ``K`` of a view some pair names that is not finite or not invertible."""
    import torch
    pairs, counts, table = _essential_batch_checks(K, pairs, uvs_a, uvs_b, counts, threshold, hypotheses)
    was_np = is_np(uvs_a)
    if not was_np and not bool(torch.isfinite(uvs_a).all() & torch.isfinite(uvs_b).all()):
        raise ValueError("find_essential_matrices: u, v must be finite")
    P, M, H = len(pairs), int(uvs_a.shape[0]), int(hypotheses)
    res = dict(E=np.zeros((P, 3, 3)), n_inliers=np.zeros(P, np.int64), hypothesis=np.zeros(P, np.int64),
               hypothesis_inliers=np.zeros(P, np.int64), refined=np.zeros(P, bool), status=np.where(counts < 8, STATUS_TOO_FEW, STATUS_OK))
    if (counts < 8).all():  # nothing to estimate: no kernel is queued
        if was_np:
            res["inliers"] = np.zeros(M, bool)
        else:
            res["inliers"] = torch.zeros(M, dtype=torch.bool, device=uvs_a.device)
        return res
    _, _, _, winner, batch, keep = _essential_batch_stages(uvs_a, uvs_b, counts, table, H, seed)
    dev = winner.device
    won = winner.cpu().numpy()  # synchronises: the one read-back of the search, all pairs
    live = counts >= 8
    res["hypothesis"][live], res["hypothesis_inliers"][live] = won[live, 9].astype(np.int64), won[live, 10].astype(np.int64)
    res["status"][live & (won[:, 10] == 0)] = STATUS_DEGENERATE
    take = res["status"] == STATUS_OK
    res["n_inliers"][take] = res["hypothesis_inliers"][take]
    mask = torch.zeros(M, dtype=torch.uint8, device=dev)
    if take.any():
        for p in np.flatnonzero(take):
            res["E"][p] = _force_rank2(won[p, :9].reshape(3, 3))
        mask, sums = _essential_batch_moments(batch, counts, take, winner, 11)
        if refine:
            idx = np.flatnonzero(take)
            Ms = np.zeros((len(idx), 9, 9))
            Ms[(slice(None),) + np.tril_indices(9)] = sums.cpu().numpy()[idx, :45]  # synchronises: the winners' sums
            vectors = np.linalg.eigh(Ms, UPLO="L")[1][:, :, 0]  # ONE call on the stacked moments
            E_fit = np.zeros((P, 9))
            for k, p in enumerate(idx):
                E_fit[p] = _force_rank2(_positive_largest(vectors[k]).reshape(3, 3)).reshape(9)
            mask_fit, sums_fit = _essential_batch_moments(batch, counts, take, torch.from_numpy(E_fit).to(dev), 9)
            fit_counts = sums_fit[:, 45].cpu().numpy().astype(np.int64)  # synchronises: the refits' sums
            kept = take & (fit_counts >= res["hypothesis_inliers"])
            res["refined"] = kept
            res["E"][kept], res["n_inliers"][kept] = E_fit[kept].reshape(-1, 3, 3), fit_counts[kept]
            if kept.any():  # rows of the pairs whose refit is kept take its mask, the others the winner's
                rows_kept = torch.repeat_interleave(torch.from_numpy(kept).to(dev), torch.from_numpy(counts).to(dev), output_size=M)
                mask = torch.where(rows_kept, mask_fit, mask)
    del keep
    res["inliers"] = to_caller(mask != 0, was_np)
    return res


# ---- filter_overlap_uvs ------------------------------------------------------------------------------------------------
def filter_overlap_uvs(uvs1, uvs2):
    """The matches whose pixel ``int32(round(u, v))`` is hit by no other match, in image 1 and in image 2 (:205-216):
    ``(uvs1[mask], uvs2[mask])``, order and dtype kept."""
    import torch
    name = _float_rows(uvs1, "uvs1")
    if _float_rows(uvs2, "uvs2", uvs1) != name or dtype_name(uvs1) not in FLOAT_TYPES or dtype_name(uvs2) != dtype_name(uvs1):
        raise ValueError("uvs1, uvs2 must both be float64 or both float32, got %s and %s" % (dtype_name(uvs1), dtype_name(uvs2)))
    n = int(uvs1.shape[0])
    if int(uvs2.shape[0]) != n:
        raise ValueError("uvs1, uvs2 must have the same number of rows, got %d and %d" % (n, uvs2.shape[0]))
    was_np = is_np(uvs1)
    if n == 0:
        return (uvs1.copy(), uvs2.copy()) if was_np else (uvs1.clone(), uvs2.clone())
    cu0, cv0, cw, ch = _window([_min_max(uvs1), _min_max(uvs2)], "filter_overlap_uvs", "")
    a = to_device(uvs1)
    b = to_device(uvs2, device=a.device)
    dev, t, who = a.device, FLOAT_TYPES[name], "filter_overlap_uvs"
    pop = torch.empty((2, cw * ch), dtype=torch.int32, device=dev)
    counters = torch.zeros(3, dtype=torch.int64, device=dev)  # kept rows, rows outside the window of set 1 / 2
    for k, uv in enumerate((a, b)):
        call("camd_cell_population", dev, uv.data_ptr(), t, n, 2, cu0, cv0, cw, ch, pop[k].data_ptr(),
             counters[1 + k:].data_ptr(), what=who)
    blocks = _native.lib().camd_overlap_blocks(n)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    blockcount = torch.empty(blocks, dtype=torch.int32, device=dev)
    call("camd_overlap_keep", dev, a.data_ptr(), b.data_ptr(), t, n, 2, cu0, cv0, cw, ch, pop[0].data_ptr(), pop[1].data_ptr(),
         keep.data_ptr(), blockcount.data_ptr(), what=who)
    start = torch.zeros(blocks + 1, dtype=torch.int64, device=dev)
    torch.cumsum(blockcount, 0, dtype=torch.int64, out=start[1:])  # the exclusive scan between count and emit
    out = torch.empty((2, n, 2), dtype=a.dtype, device=dev)
    call("camd_overlap_emit", dev, a.data_ptr(), b.data_ptr(), t, n, 2, keep.data_ptr(), start.data_ptr(), out[0].data_ptr(),
         out[1].data_ptr(), n, counters.data_ptr(), what=who)
    count, out1, out2 = (int(v) for v in counters.cpu().numpy())  # synchronises: the output length is data dependent
    if out1 or out2:
        raise RuntimeError("filter_overlap_uvs: %d rows fell outside the window sized from the data" % (out1 + out2))
    return to_caller((out[0, :count], out[1, :count]), was_np)


# ---- matching_uvs_in_one_img -------------------------------------------------------------------------------------------
def matching_uvs_in_one_img(uvs1, uvs2, MAX_DISTANCE=1, MIN_MATCHED_PIXELS=10, precise=False):
    """Points of two sets that fall into the same ``MAX_DISTANCE`` cell of one image (:241-271): ``dict(uv_match_idx1,
    uv_match_idx2)`` int64 -- per shared cell the first row of each set landing there, cells in ascending (u, v) order --
    or ``{}`` when fewer than ``MIN_MATCHED_PIXELS`` cells are shared.  ``precise=True`` (SciPy KDTree + argpartition,
    whose choice among equal distances is undefined) is refused."""
    import torch
    if precise:
        raise NotImplementedError("precise=True keeps the k smallest distances through np.argpartition, whose choice among "
                                  "equal distances is undefined: there is nothing to pin -- use precise=False")
    names = [_float_rows(uvs1, "uvs1"), _float_rows(uvs2, "uvs2", uvs1)]
    d = float(MAX_DISTANCE)
    if not (d > 0 and np.isfinite(d)):
        raise ValueError("MAX_DISTANCE must be a positive number, got %r" % (MAX_DISTANCE,))
    n1, n2 = int(uvs1.shape[0]), int(uvs2.shape[0])
    if n1 == 0 or n2 == 0:
        raise ValueError("matching_uvs_in_one_img needs at least one point in each set")
    # the quotient's dtype is NumPy's: float32 rows stay float32 unless MAX_DISTANCE itself is a wider NumPy scalar
    names = [(np.zeros(1, nm) / MAX_DISTANCE).dtype.name for nm in names]
    hint = " -- raise MAX_DISTANCE (%r)" % (MAX_DISTANCE,)
    with np.errstate(over="ignore", invalid="ignore"):
        bounds = [_min_max(uv).astype(nm) / np.dtype(nm).type(d) for uv, nm in zip((uvs1, uvs2), names)]
    cu0, cv0, cw, ch = _window(bounds, "matching_uvs_in_one_img", hint)
    was_np = is_np(uvs1)
    a = to_device(uvs1, dtype=names[0], cast=True)
    b = to_device(uvs2, dtype=names[1], cast=True, device=a.device)
    dev, who = a.device, "matching_uvs_in_one_img"
    first = torch.empty((2, cw * ch), dtype=torch.int32, device=dev)
    counters = torch.zeros(3, dtype=torch.int64, device=dev)  # shared cells, rows outside the window of set 1 / 2
    for k, (uv, nm) in enumerate(zip((a, b), names)):
        call("camd_cell_first_index", dev, uv.data_ptr(), FLOAT_TYPES[nm], int(uv.shape[0]), 2, d, cu0, cv0, cw, ch,
             first[k].data_ptr(), counters[1 + k:].data_ptr(), what=who)
    colcount = torch.empty(cw, dtype=torch.int32, device=dev)
    call("camd_cell_intersect_count", dev, first[0].data_ptr(), first[1].data_ptr(), cw, ch, colcount.data_ptr(), what=who)
    start = torch.zeros(cw + 1, dtype=torch.int64, device=dev)
    torch.cumsum(colcount, 0, dtype=torch.int64, out=start[1:])  # the exclusive scan between count and emit
    cap = min(n1, n2)
    idx = torch.empty((2, cap), dtype=torch.int64, device=dev)
    call("camd_cell_intersect_emit", dev, first[0].data_ptr(), first[1].data_ptr(), cw, ch, start.data_ptr(), idx[0].data_ptr(),
         idx[1].data_ptr(), cap, counters.data_ptr(), what=who)
    count, out1, out2 = (int(v) for v in counters.cpu().numpy())  # synchronises: the output length is data dependent
    if out1 or out2:
        raise RuntimeError("matching_uvs_in_one_img: %d rows fell outside the window sized from the data" % (out1 + out2))
    if count < MIN_MATCHED_PIXELS:
        return {}
    i1, i2 = to_caller((idx[0, :count], idx[1, :count]), was_np)
    return dict(uv_match_idx1=i1, uv_match_idx2=i2)


def _batch_bounds(sets):
    """(len(sets), 4) float64 [min u, min v, max u, max v]: ndarrays on the host, all tensors in one launch and one
    read-back (camd_uv_bounds_batch leaves one row per workgroup; min / max commute, so finishing on the host is exact)."""
    import torch
    out = np.empty((len(sets), 4), np.float64)
    dev = [k for k, s in enumerate(sets) if not is_np(s)]
    for k, s in enumerate(sets):
        if is_np(s):
            out[k] = _min_max(s)
    if dev:
        B = _native.lib().camd_uv_bounds_blocks()
        table = (_native.CellSet * len(dev))()
        for e, k in zip(table, dev):
            e.uv, e.n, e.uv_type = sets[k].data_ptr(), int(sets[k].shape[0]), FLOAT_TYPES[dtype_name(sets[k])]
        device = sets[dev[0]].device
        table_dev = torch.empty(len(dev) * 48, dtype=torch.uint8, device=device)
        parts = torch.empty((len(dev), B, 4), dtype=torch.float64, device=device)
        call("camd_uv_bounds_batch", device, table, len(dev), table_dev.data_ptr(), parts.data_ptr(),
             what="matching_uvs_in_one_img_batch")
        parts = parts.cpu().numpy()  # the one read-back of all bounds
        out[dev, :2], out[dev, 2:] = parts[:, :, :2].min(1), parts[:, :, 2:].max(1)
    return out


def matching_uvs_in_one_img_batch(pairs_of_sets, MAX_DISTANCE=1, MIN_MATCHED_PIXELS=10, max_cells=None):
    """``[matching_uvs_in_one_img(a, b, MAX_DISTANCE, MIN_MATCHED_PIXELS) for a, b in pairs_of_sets]``, bit for bit, without
    a host synchronisation per pair: one read-back of all bounds, one of all counts.  A point set that several pairs name
    (the SAME object) gets its first-occurrence grid once.  Sets that pairs link share one cell window, the union of their
    bounds (the result does not depend on the window as long as it covers the data).  All grids of a pass hold at most
    ``max_cells`` cells (default ``BATCH_MAX_CELLS``); beyond it the pairs are worked off in several passes."""
    import torch
    pairs = list(pairs_of_sets)
    if not pairs:
        return []
    cap_cells = BATCH_MAX_CELLS if max_cells is None else int(max_cells)
    d = float(MAX_DISTANCE)
    if not (d > 0 and np.isfinite(d)):
        raise ValueError("MAX_DISTANCE must be a positive number, got %r" % (MAX_DISTANCE,))
    sets, slot = [], {}  # distinct point sets in order of first appearance
    for a, b in pairs:
        for uv in (a, b):
            if id(uv) not in slot:
                _float_rows(uv, "a point set", pairs[0][0])
                if int(uv.shape[0]) == 0:
                    raise ValueError("matching_uvs_in_one_img needs at least one point in each set")
                slot[id(uv)] = len(sets)
                sets.append(uv)
    was_np = is_np(sets[0])
    names = [(np.zeros(1, _float_rows(s, "a point set")) / MAX_DISTANCE).dtype.name for s in sets]
    devs = [to_device(sets[0], dtype=names[0], cast=True)]
    devs += [to_device(s, dtype=nm, cast=True, device=devs[0].device) for s, nm in zip(sets[1:], names[1:])]
    device = devs[0].device
    raw = _batch_bounds([s if is_np(s) else t for s, t in zip(sets, devs)])
    with np.errstate(over="ignore", invalid="ignore"):
        bounds = [raw[k].astype(nm) / np.dtype(nm).type(d) for k, nm in enumerate(names)]
    # sets that a pair links share a window
    root = list(range(len(sets)))

    def find(k):
        while root[k] != k:
            root[k] = root[root[k]]
            k = root[k]
        return k

    for a, b in pairs:
        root[find(slot[id(b)])] = find(slot[id(a)])
    hint = " -- raise MAX_DISTANCE (%r)" % (MAX_DISTANCE,)
    windows = {r: _window([bounds[k] for k in range(len(sets)) if find(k) == r], "matching_uvs_in_one_img_batch", hint)
               for r in sorted({find(k) for k in range(len(sets))})}
    cells = [windows[find(k)][2] * windows[find(k)][3] for k in range(len(sets))]
    # passes: pairs in the order of their windows, as many as the cell cap lets the grids of their sets in
    order = sorted(range(len(pairs)), key=lambda p: (find(slot[id(pairs[p][0])]), p))
    passes, members, used = [[]], set(), 0
    for p in order:
        need = {slot[id(uv)] for uv in pairs[p]}
        if sum(cells[k] for k in need) > cap_cells:
            raise ValueError("matching_uvs_in_one_img_batch: one pair needs %d cells, more than max_cells = %d%s"
                             % (sum(cells[k] for k in need), cap_cells, hint))
        extra = sum(cells[k] for k in need - members)
        if passes[-1] and used + extra > cap_cells:
            passes.append([])
            members, used, extra = set(), 0, sum(cells[k] for k in need)
        passes[-1].append(p)
        members |= need
        used += extra
    done, keep = [], []  # per pass (pair numbers, idx, counts, outside); host tables stay alive until the read-back
    who = "matching_uvs_in_one_img_batch"
    for chunk in passes:
        mine = sorted({slot[id(uv)] for p in chunk for uv in pairs[p]})
        goff, total = {}, 0
        stable = (_native.CellSet * len(mine))()
        for e, k in zip(stable, mine):
            cu0, cv0, cw, ch = windows[find(k)]
            e.uv, e.n, e.grid_offset, e.uv_type = devs[k].data_ptr(), int(devs[k].shape[0]), total, FLOAT_TYPES[names[k]]
            e.cu0, e.cv0, e.cells_w, e.cells_h = cu0, cv0, cw, ch
            goff[k] = total
            total += cw * ch
        ttable = (_native.CellTriple * len(chunk))()
        ncols = capacity = 0
        for e, p in zip(ttable, chunk):
            k1, k2 = (slot[id(uv)] for uv in pairs[p])
            _, _, cw, ch = windows[find(k1)]
            e.grid_offset1, e.grid_offset2, e.column_offset, e.cells_w, e.cells_h = goff[k1], goff[k2], ncols, cw, ch
            ncols += cw
            capacity += min(int(devs[k1].shape[0]), int(devs[k2].shape[0]), cw * ch)  # a cell is shared at most once
        grids = torch.empty(total, dtype=torch.int32, device=device)
        tables_dev = torch.empty(len(mine) * 48 + len(chunk) * 32, dtype=torch.uint8, device=device)
        sd, td = tables_dev.data_ptr(), tables_dev.data_ptr() + len(mine) * 48
        outside = torch.empty(1, dtype=torch.int64, device=device)
        call("camd_cell_first_index_batch", device, stable, len(mine), sd, d, grids.data_ptr(), total, outside.data_ptr(), what=who)
        colcount = torch.empty(ncols, dtype=torch.int32, device=device)
        call("camd_cell_intersect_count_batch", device, grids.data_ptr(), total, ttable, len(chunk), td, colcount.data_ptr(), ncols,
             what=who)
        start = torch.zeros(ncols + 1, dtype=torch.int64, device=device)
        torch.cumsum(colcount, 0, dtype=torch.int64, out=start[1:])  # ONE exclusive scan over the columns of all triples
        idx = torch.empty((2, capacity), dtype=torch.int64, device=device)
        counts = torch.empty(len(chunk), dtype=torch.int64, device=device)
        call("camd_cell_intersect_emit_batch", device, grids.data_ptr(), total, ttable, len(chunk), td, start.data_ptr(), ncols,
             idx[0].data_ptr(), idx[1].data_ptr(), capacity, counts.data_ptr(), what=who)
        done.append((chunk, idx, counts, outside))
        keep.append((stable, ttable))
    numbers = torch.cat([t for _, _, c, o in done for t in (c, o)]).cpu().numpy()  # synchronises: the one read-back of all counts
    del keep
    results, at = [None] * len(pairs), 0
    for chunk, idx, _, _ in done:
        counts, out = numbers[at:at + len(chunk)], int(numbers[at + len(chunk)])
        at += len(chunk) + 1
        if out:
            raise RuntimeError("matching_uvs_in_one_img_batch: %d rows fell outside the windows sized from the data" % out)
        if was_np:
            idx = hostio.to_host(idx[:, :int(counts.sum())])
        off = 0
        for p, c in zip(chunk, (int(c) for c in counts)):
            if c < MIN_MATCHED_PIXELS:
                results[p] = {}
            elif was_np:
                results[p] = dict(uv_match_idx1=idx[0, off:off + c].copy(), uv_match_idx2=idx[1, off:off + c].copy())
            else:
                results[p] = dict(uv_match_idx1=idx[0, off:off + c], uv_match_idx2=idx[1, off:off + c])
            off += c
    return results


# ---- flow ------------------------------------------------------------------------------------------------------------
def _flow(flow, what, channel_axis):
    check_array(flow, what)
    if len(flow.shape) != 3 or flow.shape[channel_axis] != 2:
        want = "(h, w, 2)" if channel_axis == 2 else "(2, h, w)"
        raise ValueError("%s must be %s, got %s" % (what, want, tuple(flow.shape)))
    name = dtype_name(flow)
    if name not in FLOAT_TYPES:
        raise ValueError("%s must be float32 or float64, got %s" % (what, name))
    hw = [int(s) for i, s in enumerate(flow.shape) if i != channel_axis]
    if min(hw) <= 0:
        raise ValueError("%s is empty: %s" % (what, tuple(flow.shape)))
    return name, hw[0], hw[1]


def flow_abs_to_normal(flow_abs):
    """(h, w, 2) flow in pixels -> float32 (2, h, w) in image widths / heights (flow_utils.py:83-86)."""
    import torch
    name, h, w = _flow(flow_abs, "flow_abs", 2)
    f = to_device(flow_abs)
    out = torch.empty((2, h, w), dtype=torch.float32, device=f.device)
    call("camd_flow_abs_to_normal", f.device, f.data_ptr(), FLOAT_TYPES[name], w, h, out.data_ptr(), what="flow_abs_to_normal")
    return to_caller(out, is_np(flow_abs))


def flow_normal_to_abs(flow, hw=None):
    """(2, h, w) normalised flow -> float64 (h, w, 2) in pixels of an image of ``hw`` (default: the flow's own size)
    (flow_utils.py:89-95; float64 is NumPy's promotion of its ``flow * [[[w]], [[h]]]``)."""
    import torch
    name, h, w = _flow(flow, "flow", 0)
    th, tw = (h, w) if hw is None else hw
    f = to_device(flow)
    out = torch.empty((h, w, 2), dtype=torch.float64, device=f.device)
    call("camd_flow_normal_to_abs", f.device, f.data_ptr(), FLOAT_TYPES[name], w, h, float(tw), float(th), out.data_ptr(),
         what="flow_normal_to_abs")
    return to_caller(out, is_np(flow))


def flow_to_matched_uvs(flow_abs, mask):
    """``(uvs_from, uvs_to)``, float64 (n, 2): the masked pixels' centres ``(x + 0.5 - 1e-8, y + 0.5 - 1e-8)`` in row-major
    order and where the flow takes them -- one direction of ``build_set2ds_by_flowds`` (:276-282)."""
    import torch
    name, h, w = _flow(flow_abs, "flow_abs", 2)
    check_array(mask, "mask")
    if tuple(mask.shape) != (h, w):
        raise ValueError("mask %s does not match flow_abs %s" % (tuple(mask.shape), (h, w)))
    f = to_device(flow_abs)
    m = to_device(np.asarray(mask != 0) if is_np(mask) else (mask != 0), device=f.device).view(torch.uint8)
    rows = torch.empty((2, h * w, 2), dtype=torch.float64, device=f.device)
    count = torch.zeros(1, dtype=torch.int64, device=f.device)
    ws = torch.empty(_native.lib().camd_arr2d_mask_workspace_bytes(h), dtype=torch.uint8, device=f.device)
    call("camd_flow_to_matched_uvs", f.device, f.data_ptr(), FLOAT_TYPES[name], m.data_ptr(), w, h, rows[0].data_ptr(),
         rows[1].data_ptr(), h * w, count.data_ptr(), ws.data_ptr(), what="flow_to_matched_uvs")
    n = int(count.item())  # synchronises: the output length is data dependent
    return to_caller((rows[0, :n], rows[1, :n]), is_np(flow_abs))


def _cat(parts):
    if is_np(parts[0]):
        return np.concatenate(parts)
    import torch
    return torch.cat(parts)


def build_set2ds_by_flowds(viewds, flowds):
    """Matched points of every pair of views from optical flow (reconstruction_epipolar_geometry.py:256-295): ``{frozenset
    ({i, j}): dict(uvs_ij_i, uvs_ij_j, uvs_ji_j, uvs_ji_i, uvs_i, uvs_j)}`` with i < j.  ``flowds[(a, b)]`` holds
    ``common_fov_mask`` and ``flow_abs`` (h, w, 2) or ``flow_normal`` (2, h, w); a direction whose mask has <= 10 pixels is
    skipped.  A ``flow_normal`` is scaled to the target view's ``mask`` shape when ``viewds`` has one, else to its own
    (h, w) (the reference passes the whole 3-tuple there and fails on it)."""
    set2ds = {}
    for set2 in set(map(frozenset, flowds)):
        ij = tuple(sorted(set2))
        set2d = {}
        for xx, name in ((ij, "ij"), (ij[::-1], "ji")):
            if xx not in flowds:
                continue
            mask = flowds[xx]["common_fov_mask"]
            if not int((mask != 0).sum()) > 10:
                continue
            flow_abs = flowds[xx].get("flow_abs")
            if flow_abs is None:
                flow_normal = flowds[xx]["flow_normal"]
                target = viewds[xx[-1]]["mask"].shape if "mask" in viewds[xx[-1]] else tuple(flow_normal.shape)[-2:]
                flow_abs = flow_normal_to_abs(flow_normal, tuple(target)[:2])
            set2d["uvs_%s_%s" % (name, name[0])], set2d["uvs_%s_%s" % (name, name[1])] = flow_to_matched_uvs(flow_abs, mask)
        if set2d:
            set2d["uvs_i"] = _cat([set2d[k] for k in set2d if k in ("uvs_ij_i", "uvs_ji_i")])
            set2d["uvs_j"] = _cat([set2d[k] for k in list(set2d) if k in ("uvs_ij_j", "uvs_ji_j")])
            set2ds[set2] = set2d
    return set2ds


# ---- EssentialMatrixStereo ---------------------------------------------------------------------------------------------
class EssentialMatrixStereo(Stereo):
    """A ``Stereo`` whose pose comes from matched pixels: 8-point essential matrix, four candidate poses, the first whose
    mean depths in both cameras are positive (:100-150).  ``self.epipolar`` holds ``zs1, zs2, uvs1, uvs2`` (arrays of the
    caller's kind), ``E`` (3x3 ndarray) and ``z1, z2`` (the winner's mean depths, floats).

    ``robust=None``: the reference's plain 8-point fit of a subsample, as ever.  ``robust=True`` or a dict of
    ``find_essential_matrix``'s keyword arguments (threshold, hypotheses, seed, refine): ``E`` comes from there, the
    candidate is chosen by the mean depths of the INLIERS, ``zs1`` / ``zs2`` still hold every match, and ``epipolar`` gains
    ``inliers`` ((n,) bool of the caller's kind) and ``n_inliers``; ``self.robust_info`` is the estimator's whole answer.
    ``estimate``: a ``find_essential_matrix(..., return_info=True)`` answer for these very matches, oriented view 1 -> view 2
    (``find_essential_matrices`` gives every pair's in one pass): nothing is estimated, ``E``, ``inliers`` and ``n_inliers``
    come from it and the rest is the ``robust`` branch; giving both is a ``ValueError``."""

    def __init__(self, uvs1=None, uvs2=None, K1=None, K2=None, baseline=1, xy1=None, xy2=None, name1="cam1", name2="cam2",
                 robust=None, estimate=None):
        if uvs1 is None:  # (type(self)() as Stereo.copy makes it)
            super().__init__()
            return
        if K2 is None:
            K2 = K1
        if name1 == name2:
            raise ValueError("the two cameras need different names, got %r twice" % (name1,))
        if xy1 is None or xy2 is None:
            raise ValueError("xy1 and xy2 (width, height of each camera) are required: the reference's fallback reads column 3 "
                             "of a 3x3 K and cannot work")
        _float_rows(uvs1, "uvs1")
        _float_rows(uvs2, "uvs2", uvs1)
        n = int(uvs1.shape[0])
        if int(uvs2.shape[0]) != n or n < 8:
            raise ValueError("uvs1, uvs2 must hold the same number (>= 8) of matches, got %d and %d" % (n, uvs2.shape[0]))
        K1, K2 = np.asarray(K1, np.float64), np.asarray(K2, np.float64)
        if K1.shape != (3, 3) or K2.shape != (3, 3):
            raise ValueError("K1, K2 must be 3x3")
        if robust is not None and estimate is not None:
            raise ValueError("EssentialMatrixStereo: give robust or estimate, not both")
        info = None
        if robust is None and estimate is None:
            E, Ts = _pose_candidates(uvs1, uvs2, K1, K2, baseline)
        else:
            if estimate is not None:
                info = dict(estimate)
            else:
                info = find_essential_matrix(uvs1, uvs2, K1, K2, return_info=True, **({} if robust is True else dict(robust)))
            if info["status"] != "ok":
                raise ValueError("EssentialMatrixStereo: no 8 of the matches determine an essential matrix (%s)" % info["status"])
            E, Ts = info["E"], _scaled_candidates(info["E"], baseline)
        a = to_device(uvs1, dtype="float64", cast=True)
        b = to_device(uvs2, dtype="float64", cast=True, device=a.device)
        if info is None:
            means = _candidate_means(a, b, K1, K2, Ts)
        else:
            keep = to_device(info["inliers"], device=a.device)
            means = _candidate_means(a[keep], b[keep], K1, K2, Ts)
        # the first candidate with both means positive; if none is, the last one, as the reference's loop leaves it
        self.candidate = next((c for c in range(4) if means[c, 0] > 0 and means[c, 1] > 0), 3)
        T = Ts[self.candidate]
        zs = matched_uvs_to_zs(a, b, K1, K2, T)
        zs["zs1"], zs["zs2"] = to_caller((zs["zs1"], zs["zs2"]), is_np(uvs1))
        super().__init__()
        self.load(dict(R=T[:3, :3], t=T[:3, 3], cam1=dict(xy=list(xy1), K=K1, name=str(name1)),
                       cam2=dict(xy=list(xy2), K=K2, name=str(name2))))
        self.epipolar = dict(zs, E=E, uvs1=uvs1, uvs2=uvs2, z1=float(means[self.candidate, 0]), z2=float(means[self.candidate, 1]))
        if info is not None:
            self.epipolar.update(inliers=info["inliers"], n_inliers=info["n_inliers"])
            self.robust_info = info

    @classmethod
    def from_stereo(cls, uvs1, uvs2, stereo, baseline=None, robust=None, estimate=None):
        """The pose re-estimated from matches for an existing rig: everything of ``stereo``'s record is kept (distortion
        included), ``R`` and ``t`` are replaced (:152-166).  ``baseline=None``: the rig's own.  ``robust``, ``estimate``: as
        the constructor's."""
        self = cls(uvs1, uvs2, K1=stereo.cam1.K, K2=stereo.cam2.K, xy1=stereo.cam1.xy, xy2=stereo.cam2.xy,
                   baseline=baseline or stereo.baseline, robust=robust, estimate=estimate)
        rec = stereo.dump(return_dict=True)
        rec["R"], rec["t"] = self.R, self.t
        self.load(rec)
        return self

    def set_scale(self, rate):
        """Scale the translation (hence ``baseline``) and every depth of ``epipolar`` by ``rate`` (:194-202).  The
        rectifying rotations and maps depend on the direction of ``t`` only; ``min_disparity``, which
        ``set_stereo_matching`` derived from the baseline, is brought up to date."""
        rate = float(rate)
        self.t = self.t * rate
        for key in ("z1", "z2", "zs1", "zs2"):
            self.epipolar[key] *= rate
        if hasattr(self, "min_disparity"):
            self.min_disparity = int(self.cam1.K[0, 0] * self.baseline / self.max_depth)
        return self

    def align_scale_with(stereo1, stereo2, matched=None):
        """Bring this rig to the scale of ``stereo2``, which shares exactly one camera (by name) with it (:168-192): the
        ratio of the mean depths, in the shared camera, of the points both rigs matched."""
        mine, other = [stereo1.cam1.name, stereo1.cam2.name], [stereo2.cam1.name, stereo2.cam2.name]
        for pair in (mine, other):
            assert pair[0] != pair[1], "a rig needs two different camera names, got %s" % (pair,)
        shared = [nm for nm in mine if nm in other]
        assert len(shared) != 2, "names1=%s and names2=%s are the same pair of cameras" % (mine, other)
        assert len(shared) != 0, "names1=%s and names2=%s share no camera" % (mine, other)
        s1, s2 = str(mine.index(shared[0]) + 1), str(other.index(shared[0]) + 1)
        if matched is None:
            matched = matching_uvs_in_one_img(stereo1.epipolar["uvs" + s1], stereo2.epipolar["uvs" + s2])
        assert len(matched.get("uv_match_idx1", ())) > 10, "more than 10 points matched by both rigs are needed"
        z_mine = _mean(stereo1.epipolar["zs" + s1], matched["uv_match_idx1"], "align_scale_with")
        z_other = _mean(stereo2.epipolar["zs" + s2], matched["uv_match_idx2"], "align_scale_with")
        return stereo1.set_scale(z_other / z_mine)
