#!/usr/bin/env python3
"""Times ReconstructionExtrinsics (calibrating_amd.reconstruction_epipolar_geometry) on the GPU and writes
profiles/reconstruction_time.json (README and DESIGN.md section 4.3c quote that file).

    python tools/gpu_reconstruction_time.py [--out profiles/reconstruction_time.json] [--reps 5]

For 4, 8 and 12 views at 480 x 640 from the scene generator of the tests (tests/reconstruction_cases.py), matched points
already on the device as float64 tensors, from ONE run: the whole constructor; the triple stage alone through the batch
(matching_uvs_in_one_img_batch) and through a loop over matching_uvs_in_one_img; and the triple stage through the NumPy
restatement (tests/epipolar_ref.py) on this box's CPU.  Medians of a host clock that ends in a synchronise (every path
reads counts back, so it synchronises itself).  No time is asserted anywhere.  Needs a GPU: without one it fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def timed(call, reps, torch):
    call()
    torch.cuda.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
    return dict(wall_ms_median=float(np.median(wall)), wall_ms_min=float(min(wall)), wall_ms_max=float(max(wall)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruction_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, nargs="+", default=[4, 8, 12])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_reconstruction_time.py measures on the GPU; none is visible")
    import calibrating_amd as ca
    from calibrating_amd import epipolar_geometry as eg, reconstruction_epipolar_geometry as reg
    import epipolar_ref as er
    import reconstruction_cases as rcc
    rows = []
    for views in args.views:
        viewds, flowds, _ = rcc.scene(views, 100 + views, hw=(480, 640))
        host = eg.build_set2ds_by_flowds(viewds, flowds)
        host = {k: {kk: vv for kk, vv in v.items() if kk in ("uvs_i", "uvs_j")} for k, v in host.items()}
        dev = {k: {kk: torch.from_numpy(vv).cuda() for kk, vv in v.items()} for k, v in host.items()}

        def pairs_of(set2ds):
            out = []
            for _, (ii, jj, kk), _ in reg.plan_triples(list(viewds), {k: int(v["uvs_i"].shape[0]) for k, v in set2ds.items()}):
                out.append(tuple(set2ds[frozenset((o, ii))]["uvs_" + "ij"[tuple(sorted((o, ii))).index(ii)]] for o in (jj, kk)))
            return out

        pd, ph = pairs_of(dev), pairs_of(host)
        r = dict(views=views, hw=[480, 640], triples=len(pd), points_per_set_mean=float(np.mean([len(a) for a, _ in ph])))
        for stage in reg.TRIPLE_STAGES:
            r["constructor_%s" % stage] = timed(lambda: ca.ReconstructionExtrinsics(rcc.fresh(viewds), set2ds=dev, cfg=dict(triple_stage=stage)),
                                                args.reps, torch)
        r["triple_stage_batch"] = timed(lambda: eg.matching_uvs_in_one_img_batch(pd), args.reps, torch)
        r["triple_stage_loop"] = timed(lambda: [eg.matching_uvs_in_one_img(a, b) for a, b in pd], args.reps, torch)
        t0 = time.perf_counter()
        for a, b in ph:
            er.matching(a, b)
        r["triple_stage_cpu_numpy_restatement_ms"] = 1e3 * (time.perf_counter() - t0)
        r["host_synchronisations_triple_stage"] = dict(batch=2, loop=2 * len(pd))
        rows.append(r)
        print(json.dumps(r))
    doc = dict(tool="tools/gpu_reconstruction_time.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               default_triple_stage=reg.TRIPLE_STAGE,
               what="matched points resident on the device (float64); a host clock ending in a synchronise; medians over reps "
                    "after one warm-up call; call times (checks, bounds, kernels, cumsum, read-backs), not kernel times",
               points=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
