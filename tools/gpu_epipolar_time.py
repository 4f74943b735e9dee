#!/usr/bin/env python3
"""Times the epipolar path (calibrating_amd.epipolar_geometry) on the GPU and writes profiles/epipolar_time.json (the
README row quotes that file).

    python tools/gpu_epipolar_time.py [--out profiles/epipolar_time.json] [--reps 20]

Per point: the median over ``reps`` calls, after a warm-up of the same shape, of one call with its inputs already on
the device -- events on the current stream around the call, and a host clock that ends in a synchronise (these calls
read their output length back, so they synchronise themselves) -- next to the number of kernels this library launches
in it, and from the SAME run the NumPy restatement (tests/epipolar_ref.py) on this box's CPU.  The constructor of
EssentialMatrixStereo is split into its four parts.  No time is asserted anywhere.  Needs a GPU: without one it fails."""
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

# kernels this library launches per call (torch's own -- min / max, cumsum, copies -- come on top)
LAUNCHES = dict(matching_uvs_in_one_img=6, filter_overlap_uvs=6, flow_to_matched_uvs=3, cheirality=2, zs_of_winner=1)


def timed(call, reps, torch):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        ev.append(a.elapsed_time(b))
    return dict(gpu_events_ms_median=float(np.median(ev)), gpu_events_ms_min=float(min(ev)), gpu_events_ms_max=float(max(ev)),
                wall_ms_median=1e3 * float(np.median(wall)))


def cpu(call):
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epipolar_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_epipolar_time.py measures on the GPU; none is visible")
    from calibrating_amd import epipolar_geometry as eg
    import epipolar_cases as ec
    import epipolar_ref as er
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rows = []

    def add(name, what, launches, call, cpu_call, **extra):
        r = dict(name=name, call=what, library_kernel_launches=launches, **timed(call, args.reps, torch))
        r["cpu_numpy_restatement_ms"] = None if cpu_call is None else cpu(cpu_call)
        r.update(extra)
        rows.append(r)
        print(json.dumps(r))

    for n in (60000, 300000, 2000000):
        rng = np.random.default_rng(n)
        u1 = np.stack([rng.uniform(0, 1920, n), rng.uniform(0, 1080, n)], 1)
        u2 = np.ascontiguousarray(u1[rng.permutation(n)] + rng.normal(0, 0.3, (n, 2)))
        a, b = dev(u1), dev(u2)
        add("matching_1080p_%d" % n, "matching_uvs_in_one_img", LAUNCHES["matching_uvs_in_one_img"],
            lambda: eg.matching_uvs_in_one_img(a, b), lambda: er.matching(u1, u2), points_per_set=n)
        add("overlap_1080p_%d" % n, "filter_overlap_uvs", LAUNCHES["filter_overlap_uvs"],
            lambda: eg.filter_overlap_uvs(a, b), lambda: er.overlap_filter(u1, u2), points_per_set=n)
    for hw in ((1024, 1024), (1080, 1920)):
        flow, mask = ec.flow_abs(hw[0], hw), ec.flow_mask(hw[1], hw, 0.3)
        f, m = dev(flow), dev(mask)
        add("flow_%dx%d" % hw, "flow_to_matched_uvs", LAUNCHES["flow_to_matched_uvs"], lambda: eg.flow_to_matched_uvs(f, m),
            lambda: er.flow_to_uvs(flow, mask), mask_density=0.3)
    base = ec.pose_case("scene_720p_noise")
    K1, K2 = base["K1"], base["K2"]
    for n in (20000, 2000000):
        k = -(-n // len(base["uvs1"]))
        rng = np.random.default_rng(n + 1)
        u1 = np.tile(base["uvs1"], (k, 1))[:n] + rng.normal(0, 0.05, (n, 2))
        u2 = np.tile(base["uvs2"], (k, 1))[:n] + rng.normal(0, 0.05, (n, 2))
        a, b = dev(u1), dev(u2)
        E, Ts = eg._pose_candidates(a, b, K1, K2, 0.3)
        st = eg.EssentialMatrixStereo(a, b, K1, K2, baseline=0.3, xy1=base["xy1"], xy2=base["xy2"])
        rec = st.dump(return_dict=True)

        def tables():
            fresh = type(st)().load(rec)
            fresh._tables("cuda")

        add("ctor_%d_total" % n, "EssentialMatrixStereo(...)", LAUNCHES["cheirality"] + LAUNCHES["zs_of_winner"],
            lambda: eg.EssentialMatrixStereo(a, b, K1, K2, baseline=0.3, xy1=base["xy1"], xy2=base["xy2"]), None, matches=n)
        add("ctor_%d_host_svd" % n, "subsample to host + compute/decompose_essential_matrix", 0,
            lambda: eg._pose_candidates(a, b, K1, K2, 0.3), None, matches=n)
        add("ctor_%d_cheirality" % n, "camd_epipolar_sums (four candidates, one pass) + read-back", LAUNCHES["cheirality"],
            lambda: eg._candidate_means(a, b, K1, K2, Ts), None, matches=n)
        add("ctor_%d_load" % n, "Stereo.load of the record (host geometry)", 0, lambda: type(st)().load(rec), None, matches=n)
        add("ctor_%d_table_build" % n, "load + the rectify maps on the device (first use)", 2, tables, None, matches=n)
    doc = dict(tool="tools/gpu_epipolar_time.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               what="per call, inputs resident on the device: stream events around the call and a host clock ending in a "
                    "synchronise; medians; call times (checks, min/max, kernels, cumsum, read-back), not kernel times",
               points=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
