#!/usr/bin/env python3
"""Times the RANSAC 8-point estimator (epipolar_geometry.find_essential_matrix, csrc/essential.hip) on the GPU and writes
profiles/essential_time.json (the README row quotes that file).

    python tools/gpu_essential_time.py [--out profiles/essential_time.json] [--reps 10]

Per (matches, hypotheses): the median over ``reps`` calls, after a warm-up of the same shape and with the matches already
on the device, of each stage alone (stream events around the launch) and of the whole call (a host clock as well: it
reads the winner and the moments back, so it synchronises itself).  Beside them, from the SAME run and on this box's CPU:
today's host path (the plain 8-point fit of every n // 100-th match) and, at the sizes where it ends in reasonable time,
the NumPy restatement (tests/essential_ref.py).  EXPECTATION, recorded as such and not asserted: scoring is bound by
float64 VALU -- 40 products, sums and compares per (hypothesis, match) as the kernel is written (score_flop) -- not by
memory: every match is read once per pass.  No time is asserted anywhere.  Needs a GPU: without one it fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCORE_OPS = 40  # float64 operations of ess_inlier per (hypothesis, match)
RESTATEMENT_MAX = 5000 * 1024  # hypotheses x matches up to which the NumPy restatement is timed too


def timed(call, reps, torch):
    for _ in range(2):
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
    return dict(gpu_events_ms_median=float(np.median(ev)), gpu_events_ms_min=float(min(ev)), wall_ms_median=1e3 * float(np.median(wall)))


def cpu(call):
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_essential_time.py measures on the GPU; none is visible")
    from calibrating_amd import epipolar_geometry as eg
    import essential_cases as es
    import essential_ref as er
    points = []
    for n in (5000, 200000, 2000000):
        s = es.scene(n=n, noise=0.3, wrong=0.3, seed=4500)
        K1, K2 = s["K1"], s["K2"]
        a, b = (torch.from_numpy(s[k]).cuda() for k in ("uvs1", "uvs2"))
        rows, thr2 = eg._EssentialRows(a, b, K1, K2), er.ray_threshold2(K1, K2, 1.0)
        host_ms = cpu(lambda: eg._pose_candidates(s["uvs1"], s["uvs2"], K1, K2, 0.3))
        for H in (256, 1024, 4096):
            _, Es = eg._essential_hypotheses(rows, H, 0)
            _, winner = eg._essential_score(rows, Es, thr2)
            r = dict(matches=n, hypotheses=H, score_flop=SCORE_OPS * H * n, todays_host_path_ms=host_ms,
                     hypotheses_stage=timed(lambda: eg._essential_hypotheses(rows, H, 0), args.reps, torch),
                     score_stage=timed(lambda: eg._essential_score(rows, Es, thr2), args.reps, torch),
                     moments_stage=timed(lambda: eg._essential_moments(rows, winner[:9], thr2), args.reps, torch),
                     whole_call=timed(lambda: eg.find_essential_matrix(a, b, K1, K2, hypotheses=H), args.reps, torch))
            r["score_gflops_by_events"] = r["score_flop"] / r["score_stage"]["gpu_events_ms_median"] / 1e6
            r["cpu_numpy_restatement_ms"] = (cpu(lambda: er.find(s["uvs1"], s["uvs2"], K1, K2, 1.0, H, 0))
                                             if n * H <= RESTATEMENT_MAX else None)
            points.append(r)
            print(json.dumps(r))
    doc = dict(tool="tools/gpu_essential_time.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               what="per call, matches resident on the device (30 % wrong pairs, 0.3 px noise): stream events around the call and "
                    "a host clock ending in a synchronise; medians; call times (allocation, launches, read-backs), not kernel times",
               expectation="scoring bound by float64 VALU at score_flop = 40 H n operations, not by memory (not asserted)",
               points=points)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
