"""The poses of N cameras and per-view sparse depths from matched points or optical flow -- the reference's
``reconstruction_epipolar_geometry.py`` (``ReconstructionExtrinsics``, :31-314): same arguments, same meaning, same results.

Where the work runs.  The bookkeeping -- which view of a triple is its main view, the seed, the propagation path, the
chain of poses -- is host Python that follows the reference statement for statement, so that every tie-break comes out
the same.  Everything that touches every match is a kernel (csrc/epipolar.hip): the matches of ALL
triples in one pass (``epipolar_geometry.matching_uvs_in_one_img_batch``: one read-back of bounds and one of counts instead
of two per triple), the rigs (``EssentialMatrixStereo``), and the per-view rows ``uvzis``, which are packed into one device
buffer, summed in a fixed order and scaled in place without a host concatenation.

Three deviations from the reference, each where it fails or silently loses data: a triple with
two or more empty pairs is skipped instead of ending the loop over triples; the seed's second view gets its pose when a
path entry first needs it instead of ``KeyError: 'T_re'``; views the propagation does not reach raise ``ValueError``.
"""
from itertools import combinations

import numpy as np
from numpy.linalg import inv

from . import _native, epipolar_geometry as eg
from ._arrays import FLOAT_TYPES, dtype_name, is_np, to_caller, to_device
from ._native import call

TRIPLE_STAGES = ("batch", "loop")
TRIPLE_STAGE = "batch"  # how the triples are matched unless cfg["triple_stage"] says otherwise (DESIGN.md 4.3c has the timing)


def view_xy(viewd, key="?"):
    """(width, height) of a view: from ``img`` (only its shape is read), else ``xy``, else ``mask``."""
    if "img" in viewd:
        return tuple(int(v) for v in tuple(viewd["img"].shape)[:2][::-1])
    if "xy" in viewd:
        return tuple(int(v) for v in viewd["xy"])
    if "mask" in viewd:
        return tuple(int(v) for v in tuple(viewd["mask"].shape)[:2][::-1])
    raise ValueError("view %r has no size: one of 'img', 'xy' or 'mask' is required" % (key,))


# ---- planning: counts in, decisions out (no array is read) -------------------------------------------------------------
def plan_triples(view_keys, pair_sizes):
    """The triples worth matching, in the order ``combinations(viewds, 3)`` yields them (:129-144): ``[(set3, idx_sorted,
    not_include_uvsn)]``.  ``pair_sizes[frozenset((i, j))]`` = rows of ``set2ds[{i, j}]["uvs_i"]`` (absent = 0).
    ``idx_sorted[0]`` is the main view: the one whose opposite pair has the fewest matches (stable sort).  A triple with two
    or more empty pairs is skipped (the reference ends the whole loop there)."""
    out = []
    for set3 in combinations(view_keys, 3):
        set3 = frozenset(set3)
        ijk = tuple(sorted(set3))
        not_include_uvsn = {idx: int(pair_sizes.get(set3.difference({idx}), 0)) for idx in ijk}
        if list(not_include_uvsn.values()).count(0) >= 2:
            continue
        out.append((set3, sorted(ijk, key=lambda x: not_include_uvsn[x]), not_include_uvsn))
    return out


def plan_propagation(view_keys, triples, reroot=None):
    """Seed and propagation path from the matched triples (:146-179).  ``triples``: ``[(set3, idx_sorted, not_include_uvsn,
    number of matches)]`` in the order they were made.  ``reroot(set3, idx_sorted)`` is called when the view a triple adds
    is its main view (the triple must then be matched again around a view that is already placed) and returns whether
    it still matches.  -> ``dict(seed, propagate_path, rerooted)``; ``ValueError`` names the views that are not reached."""
    if not triples:
        raise ValueError("no triple of views shares enough matched points")
    info = {t[0]: t for t in triples}
    idx_sorted = {t[0]: list(t[1]) for t in triples}
    set3_sort_matched = sorted(info, key=lambda x: info[x][3])[::-1]
    seed = set3_sort_matched.pop(0)
    propagated = set(seed)
    propagate_path = [(idx_sorted[seed][2], seed)]
    rerooted = []
    while len(set3_sort_matched):
        for set3 in set3_sort_matched[:]:
            diff = set3.difference(propagated)
            if len(diff) == 1:
                idx_new = list(diff)[0]
                set3_sort_matched.remove(set3)
                if idx_new == idx_sorted[set3][0]:
                    if info[set3][2][idx_new] == 0:
                        break  # the two placed views share no matches: the triple is void
                    order = idx_sorted[set3][1:] + idx_sorted[set3][:1]
                    if reroot is not None and not reroot(set3, order):
                        break  # nothing matches around the new main view: void as well
                    idx_sorted[set3] = order
                    rerooted.append(set3)
                propagated = propagated.union(set3)
                propagate_path.append((idx_new, set3))
                break
            if len(diff) == 0:
                set3_sort_matched.remove(set3)
                break
        if len(diff) in [2, 3]:
            break  # no remaining triple touches the placed views
    missing = [k for k in view_keys if k not in propagated]
    if missing:
        raise ValueError("%d views are not reached from the seed %s (more than one connected group): %s"
                         % (len(missing), sorted(seed), missing))
    return dict(seed=seed, propagate_path=propagate_path, rerooted=rerooted)


# ---- the depth rows ----------------------------------------------------------------------------------------------------
def _column_sum(buf, row0, n, column=2):
    """Sum of ``buf[row0 : row0 + n, column]`` through the fixed-order reduction; a device scalar is read back."""
    import torch
    partials = torch.empty(_native.lib().camd_column_sum_blocks(n), dtype=torch.float64, device=buf.device)
    out = torch.empty(1, dtype=torch.float64, device=buf.device)
    call("camd_column_sum", buf.device, buf.data_ptr(), int(buf.shape[0]), int(buf.shape[1]), column, row0, n,
         partials.data_ptr(), out.data_ptr(), what="ReconstructionExtrinsics")
    return float(out.cpu().numpy()[0])


def _column_scale(buf, row0, n, rate, column=2):
    call("camd_column_scale", buf.device, buf.data_ptr(), int(buf.shape[0]), int(buf.shape[1]), column, row0, n, float(rate),
         what="ReconstructionExtrinsics.change_scale")


def _pack(buf, row0, uvs, zs, other):
    name = "float32" if dtype_name(uvs) == "float32" else "float64"
    uv = to_device(uvs, dtype=name, cast=True, device=None if is_np(uvs) else buf.device)
    z = to_device(zs, dtype="float64", cast=True, device=None if is_np(zs) else buf.device)
    call("camd_uvzi_pack", buf.device, uv.data_ptr(), FLOAT_TYPES[name], z.data_ptr(), int(uv.shape[0]), float(other),
         buf.data_ptr(), int(buf.shape[0]), row0, what="ReconstructionExtrinsics")


def _inlier_rows(uvs_a, uvs_b, inliers, total):
    """``(uvs_a[inliers], uvs_b[inliers])`` of device rows, order kept, without a read-back: ``total`` = the number of
    inliers, which the estimator has already reported.  The emit step of the compaction ``filter_overlap_uvs`` uses."""
    import torch
    dev, n = uvs_a.device, int(uvs_a.shape[0])
    a, b = uvs_a.contiguous(), uvs_b.contiguous()
    blocks = _native.lib().camd_overlap_blocks(n)
    keep = torch.zeros(blocks * 256, dtype=torch.uint8, device=dev)
    keep[:n] = inliers
    start = torch.zeros(blocks + 1, dtype=torch.int64, device=dev)
    torch.cumsum(keep.view(blocks, 256).sum(1, dtype=torch.int64), 0, out=start[1:])  # the exclusive scan between count and emit
    out = torch.empty((2, total, 2), dtype=a.dtype, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    call("camd_overlap_emit", dev, a.data_ptr(), b.data_ptr(), FLOAT_TYPES[dtype_name(a)], n, 2, keep.data_ptr(), start.data_ptr(),
         out[0].data_ptr(), out[1].data_ptr(), total, counter.data_ptr(), what="ReconstructionExtrinsics")
    return out[0], out[1]


def robust_set2ds(viewds, set2ds, robust):
    """``cfg["robust"]``: every pair of ``set2ds`` through ONE ``find_essential_matrices`` call (pairs in ``set2ds`` order, the
    lower key first, ``K`` from ``viewds``) -> (the pairs reduced to their inliers, order kept: ``{set2: dict(uvs_i, uvs_j)}``,
    new dicts; the estimator's answer with ``keys``: the pairs' ``(i, j)``).  A pair whose status is not 0 is left with 0
    rows."""
    import torch
    kw = {} if robust is True else dict(robust)
    keys = list(viewds)
    index = {k: n for n, k in enumerate(keys)}
    order = [tuple(sorted(set2)) for set2 in set2ds]
    parts_i, parts_j = [set2ds[frozenset(ij)]["uvs_i"] for ij in order], [set2ds[frozenset(ij)]["uvs_j"] for ij in order]
    was_np = is_np(parts_i[0])
    cat = np.concatenate if was_np else torch.cat
    uvs_i, uvs_j = cat(parts_i), cat(parts_j)
    counts = np.array([int(p.shape[0]) for p in parts_i], np.int64)
    K = np.stack([np.asarray(viewds[k]["K"], np.float64)[:3, :3] for k in keys])
    res = eg.find_essential_matrices(K, np.array([(index[i], index[j]) for i, j in order], np.int64).reshape(-1, 2), uvs_i, uvs_j,
                                     counts, **kw)
    res["keys"] = order
    kept = np.where(res["status"] == 0, res["n_inliers"], 0)
    if not was_np and int(kept.sum()):
        rows_i, rows_j = _inlier_rows(uvs_i, uvs_j, res["inliers"], int(kept.sum()))
    else:
        rows_i, rows_j = uvs_i[:0], uvs_j[:0]
    bounds, at = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum(kept)])
    filtered = {}
    for p, ij in enumerate(order):
        if was_np:
            on = res["inliers"][bounds[p]:bounds[p + 1]]
            filtered[frozenset(ij)] = dict(uvs_i=parts_i[p][on], uvs_j=parts_j[p][on])
        else:
            filtered[frozenset(ij)] = dict(uvs_i=rows_i[at[p]:at[p + 1]], uvs_j=rows_j[at[p]:at[p + 1]])
    return filtered, res


class ReconstructionExtrinsics:
    def __init__(self, viewds, set2ds=None, flowds=None, cfg=None):
        """``viewds[k]``: ``K`` and the view's size (``img`` / ``xy`` / ``mask``); ``set2ds[frozenset((i, j))]``: ``uvs_i``,
        ``uvs_j`` matched points of the pair, i < j -- or ``flowds[(a, b)]``: ``flow_abs`` / ``flow_normal`` and
        ``common_fov_mask``, from which ``set2ds`` is built.  Afterwards every view holds ``T_re`` (4x4 float64 ndarray,
        camera to world) and ``uvzis`` ((m, 4) float64 rows [u, v, z, other view]: ndarray for ndarray matches, CUDA tensor
        for tensor matches); mean depth 1 over all views, view ``0`` at ``z = -its mean depth`` looking down +z.

        ``cfg["robust"]``: ``True`` or a dict of ``find_essential_matrices``' keywords (threshold, hypotheses, seed, refine) for
        matches that hold wrong pairs -- every pair is estimated robustly in one pass and reduced to its inliers before
        anything else (``robust_set2ds``); the rigs then take the pair's ``E`` from there instead of the plain 8-point fit.
        ``self.set2ds`` holds the filtered pairs (``refine()`` bundles inliers only), ``self.set2ds_all`` the caller's, which
        are not mutated, ``self.robust`` the estimator's answer.  Absent or ``None``: the constructor as ever."""
        self.cfg = cfg or {}
        self.viewds = viewds
        stage = self.cfg.get("triple_stage", TRIPLE_STAGE)
        if stage not in TRIPLE_STAGES:
            raise ValueError("cfg['triple_stage'] must be one of %s, got %r" % (TRIPLE_STAGES, stage))
        if len(viewds) < 3:
            raise ValueError("at least 3 views are required, got %d" % len(viewds))
        if 0 not in viewds:
            raise KeyError("viewds needs a view with key 0: the result is placed relative to it")
        xys = {k: view_xy(v, k) for k, v in viewds.items()}
        for k in viewds:
            if "K" not in viewds[k]:
                raise ValueError("view %r has no 'K'" % (k,))
            float(k)  # the key goes into the fourth column of uvzis
        if not set2ds and flowds:
            set2ds = self.build_set2ds_by_flowds(viewds, flowds)
        if not set2ds:
            raise ValueError("set2ds or flowds with at least one pair of views is required")
        self.set2ds_all, self.robust = set2ds, None
        estimates = {}
        if self.cfg.get("robust") is not None:
            set2ds, self.robust = robust_set2ds(viewds, set2ds, self.cfg["robust"])
            for p, ij in enumerate(self.robust["keys"]):
                if self.robust["status"][p] == 0:
                    estimates[ij] = self.robust["E"][p]
        self.set2ds = set2ds
        self.flowds = flowds

        def estimate_of(ii, jj, uvs):
            """the pair's answer oriented ii -> jj for its filtered rows: every row is an inlier"""
            if self.robust is None:
                return None
            import torch
            n = int(uvs.shape[0])
            E = estimates[(ii, jj)] if ii < jj else estimates[(jj, ii)].T
            ones = np.ones(n, bool) if is_np(uvs) else torch.ones(n, dtype=torch.bool, device=uvs.device)
            return dict(E=np.array(E), inliers=ones, n_inliers=n, status="ok")

        def uvsd_of(idx_sorted):
            ii, jj, kk = idx_sorted
            uvsd = {}
            for idx_other in (jj, kk):
                set2 = frozenset([idx_other, ii])
                at = tuple(sorted(set2)).index(ii)
                uvsd[idx_other] = dict(uvs_main=set2ds[set2]["uvs_" + "ij"[at]], uvs_other=set2ds[set2]["uvs_" + "ji"[at]])
            return uvsd

        # build_set3ds: sizes come from shapes, the matches of all triples from one pass
        sizes = {set2: int(d["uvs_i"].shape[0]) for set2, d in set2ds.items()}
        planned = plan_triples(list(viewds), sizes)
        uvsds = [uvsd_of(idx_sorted) for _, idx_sorted, _ in planned]
        pairs = [(u[idx_sorted[1]]["uvs_main"], u[idx_sorted[2]]["uvs_main"]) for u, (_, idx_sorted, _) in zip(uvsds, planned)]
        if stage == "batch":
            matches = eg.matching_uvs_in_one_img_batch(pairs)
        else:
            matches = [eg.matching_uvs_in_one_img(a, b) for a, b in pairs]
        set3ds = {}
        for (set3, idx_sorted, not_include_uvsn), uvsd, matched in zip(planned, uvsds, matches):
            if matched:
                set3ds[set3] = dict(idx_sorted=idx_sorted, uvsd=uvsd, not_include_uvsn=not_include_uvsn, **matched)

        def reroot(set3, idx_sorted):  # rare: the single call
            uvsd = uvsd_of(idx_sorted)
            matched = eg.matching_uvs_in_one_img(uvsd[idx_sorted[1]]["uvs_main"], uvsd[idx_sorted[2]]["uvs_main"])
            if matched:
                set3ds[set3].update(matched, idx_sorted=idx_sorted, uvsd=uvsd)
            return bool(matched)

        plan = plan_propagation(list(viewds), [(s, d["idx_sorted"], d["not_include_uvsn"], int(d["uv_match_idx1"].shape[0]))
                                               for s, d in set3ds.items()], reroot)
        seed, propagate_path = plan["seed"], plan["propagate_path"]

        # propagate_scale
        stereods = {}
        idx_seed_main, idx_seed_2th = set3ds[seed]["idx_sorted"][:2]
        T_re = {idx_seed_main: np.eye(4)}
        propagate_baseline = {}

        def step(idx_new, set3):
            set3d = set3ds[set3]
            assert idx_new != set3d["idx_sorted"][0]
            idx_main, jj, kk = set3d["idx_sorted"]
            idx_propagated = kk if idx_new == jj else jj
            uvsd = set3d["uvsd"]

            def get_stereo(ii, jj):
                if (ii, jj) not in stereods:
                    stereods[(ii, jj)] = eg.EssentialMatrixStereo(
                        uvsd[jj]["uvs_main"], uvsd[jj]["uvs_other"], K1=viewds[ii]["K"], K2=viewds[jj]["K"], xy1=xys[ii],
                        xy2=xys[jj], name1=ii, name2=jj, baseline=propagate_baseline.get(frozenset([ii, jj]), 1),
                        estimate=estimate_of(ii, jj, uvsd[jj]["uvs_main"]))
                return stereods[(ii, jj)]

            stereo_new = get_stereo(idx_main, idx_new)
            stereo_propagated = get_stereo(idx_main, idx_propagated)
            suffix_new, suffix_propagated = "12" if idx_new == jj else "21"
            matched = dict(uv_match_idx1=set3d["uv_match_idx" + suffix_new], uv_match_idx2=set3d["uv_match_idx" + suffix_propagated])
            stereo_new.align_scale_with(stereo_propagated, matched)
            propagate_baseline[frozenset([idx_main, idx_new])] = stereo_new.baseline
            T_re[idx_new] = T_re[idx_main] @ inv(stereo_new.T)

        seed_2th_placed = False
        for idx_new, set3 in propagate_path:
            if set3ds[set3]["idx_sorted"][0] not in T_re:  # only the seed's second view can be placed and still without a pose
                step(idx_seed_2th, seed)
                seed_2th_placed = True
            step(idx_new, set3)
        if not seed_2th_placed:
            step(idx_seed_2th, seed)
        for k in viewds:
            viewds[k]["T_re"] = T_re[k]

        self.set3ds = set3ds
        self.seed = seed
        self.propagate_path = propagate_path
        self.stereods = stereods
        self._depth_rows()

    def _depth_rows(self):
        """uvzis of every view in ONE device buffer, views in the order of ``viewds``; within a view the rigs' blocks in
        the reverse of the order the rigs were made (the reference prepends), then mean depth 1 and view 0 in place."""
        import torch
        viewds, stereods = self.viewds, self.stereods
        blocks = {k: [] for k in viewds}  # per view [(uvs, zs, other view)], in the order the reference prepends them
        for (k1, k2), stereo in stereods.items():
            d = stereo.epipolar
            blocks[k1].insert(0, (d["uvs1"], d["zs1"], k2))
            blocks[k2].insert(0, (d["uvs2"], d["zs2"], k1))
        first = next(iter(stereods.values())).epipolar["uvs1"]
        was_np = is_np(first)
        if was_np:
            _native.require_device()
        device = torch.device("cuda", torch.cuda.current_device()) if was_np else first.device
        rows = {k: sum(int(b[0].shape[0]) for b in blocks[k]) for k in viewds}
        total = sum(rows.values())
        buf = torch.empty((total, 4), dtype=torch.float64, device=device)
        start, at = {}, 0
        for k in viewds:
            start[k] = at
            for uvs, zs, other in blocks[k]:
                _pack(buf, at, uvs, zs, other)
                at += int(uvs.shape[0])
        self._normalise(buf, start, rows, was_np)

    def _normalise(self, buf, start, rows, was_np):
        """The class's normalisation of the packed rows ``buf`` (view k owns rows ``start[k] .. start[k] + rows[k]``) and of
        the poses: mean depth 1 over all rows, view 0 at ``z = -its mean depth``; then every view gets its ``uvzis``."""
        viewds = self.viewds
        total = int(buf.shape[0])
        z_mean = _column_sum(buf, 0, total) / total
        rate = 1 / np.float64(z_mean)
        _column_scale(buf, 0, total, rate)
        for viewd in viewds.values():
            viewd["T_re"][:3, 3] *= rate
        T0_target = np.eye(4)
        T0_target[2, 3] = -(_column_sum(buf, start[0], rows[0]) / rows[0])
        rows_all = to_caller(buf, was_np)
        for k, viewd in viewds.items():
            viewd["uvzis"] = rows_all[start[k]:start[k] + rows[k]]
        self.apply_T(T=T0_target @ inv(viewds[0]["T_re"]))

    def refine(self, threshold=None, fixed_view=0):
        """Refine every view's ``T_re`` and one world point per match of EVERY pair of ``set2ds`` together
        (``bundle.bundle_adjust_pairs``: its gauge, its refusals), write the poses back and rebuild every view's ``uvzis``
        from the refined points: views in the order of ``viewds``, within a view the pairs in the order of ``set2ds``; then
        the class's own normalisation.  Unlike after the constructor, ``uvzis`` then holds rows of every pair of ``set2ds``,
        not only of the rigs the propagation built, and only of the matches the refinement used.  ``fixed_view`` is a key of
        ``viewds``.  The result dict is kept as ``self.refinement``; -> ``self.viewds``."""
        import torch
        from . import bundle
        viewds, set2ds = self.viewds, self.set2ds
        keys = list(viewds)
        if fixed_view not in viewds:
            raise ValueError("fixed_view must be a key of viewds, got %r" % (fixed_view,))
        index = {k: i for i, k in enumerate(keys)}
        order = []  # (a, b, uvs_a, uvs_b) with index[a] < index[b], pairs in set2ds order
        for set2, d in set2ds.items():
            i, j = sorted(set2)
            if int(d["uvs_i"].shape[0]) == 0:
                continue
            flip = index[i] > index[j]
            order.append((j, i, d["uvs_j"], d["uvs_i"]) if flip else (i, j, d["uvs_i"], d["uvs_j"]))
        if not order:
            raise ValueError("set2ds holds no matches")
        was_np = is_np(order[0][2])
        cat = np.concatenate if was_np else torch.cat
        res = bundle.bundle_adjust_pairs(
            np.stack([np.asarray(viewds[k]["K"], np.float64)[:3, :3] for k in keys]), np.stack([viewds[k]["T_re"] for k in keys]),
            np.array([(index[a], index[b]) for a, b, _, _ in order], np.int32), cat([o[2] for o in order]), cat([o[3] for o in order]),
            np.array([int(o[2].shape[0]) for o in order], np.int64), fixed_view=index[fixed_view], threshold=threshold,
            return_rows=True, view_labels=[float(k) for k in keys])
        for k in keys:
            viewds[k]["T_re"] = res["T"][index[k]].copy()
        rows_a, rows_b = (to_device(res[n], dtype="float64") for n in ("rows_a", "rows_b"))
        bounds = np.concatenate([[0], np.cumsum(res["used_counts"])])
        blocks = {k: [] for k in keys}
        for p, (a, b, _, _) in enumerate(order):
            blocks[a].append(rows_a[bounds[p]:bounds[p + 1]])
            blocks[b].append(rows_b[bounds[p]:bounds[p + 1]])
        rows = {k: sum(int(x.shape[0]) for x in blocks[k]) for k in keys}
        start, at = {}, 0
        for k in keys:
            start[k], at = at, at + rows[k]
        buf = torch.cat([x for k in keys for x in blocks[k]])
        self._normalise(buf, start, rows, was_np)
        self.refinement = res
        return self.viewds

    build_set2ds_by_flowds = staticmethod(eg.build_set2ds_by_flowds)

    def change_scale(self, rate=1, T=None):
        """Depths and translations times ``rate`` -- or, with ``T``, every pose ``T @ T_re`` (the scale must agree first:
        ``T`` is a rigid motion).  ``uvzis`` are scaled in place, tensors by the column kernel."""
        for viewd in self.viewds.values():
            if T is None:
                uvzis = viewd["uvzis"]
                if is_np(uvzis):
                    uvzis[:, 2] *= rate
                else:
                    _column_scale(uvzis, 0, int(uvzis.shape[0]), rate)
                viewd["T_re"][:3, 3] *= rate
            else:
                assert rate == 1
                viewd["T_re"] = T @ viewd["T_re"]
        return self.viewds

    def apply_T(self, T):
        return self.change_scale(T=T)
