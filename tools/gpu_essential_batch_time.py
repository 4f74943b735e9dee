#!/usr/bin/env python3
"""Times find_essential_matrices (every pair of a batch in one pass, csrc/essential.hip) against a loop of
find_essential_matrix over the same pairs and writes profiles/essential_batch_time.json (the README row and DESIGN.md quote
that file).

    python tools/gpu_essential_batch_time.py [--out profiles/essential_batch_time.json] [--reps 10]

Per (pairs, matches a pair) in {3, 28, 120} x {300, 5 000, 200 000}, at 1024 hypotheses, matches resident on the device (30 %
wrong pairs, 0.3 px noise; pair p holds the scene's matches rotated by 997 p rows, so every pair draws other samples): the
median over ``reps`` calls, after two warm-up calls of the same shape, of the batched call and of the loop -- both read their
results back, so a host clock ending in a synchronise is the measure -- and, by stream events around the launches, of the
batch's score stage alone (clear, score, winners) with the four waves' counts summed in LDS and with one atomic per wave.
No time is asserted anywhere.  Needs a GPU: without one it fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HYPOTHESES = 1024


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
    return dict(gpu_events_ms_median=float(np.median(ev)), gpu_events_ms_min=float(min(ev)), wall_ms_median=1e3 * float(np.median(wall)),
                wall_ms_min=1e3 * float(min(wall)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_batch_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_essential_batch_time.py measures on the GPU; none is visible")
    from calibrating_amd import epipolar_geometry as eg
    import essential_cases as es
    points = []
    for n in (300, 5000, 200000):
        s = es.scene(n=n, noise=0.3, wrong=0.3, seed=4500)
        K = np.stack([s["K1"], s["K2"]])
        one_a, one_b = (torch.from_numpy(s[k]).cuda() for k in ("uvs1", "uvs2"))
        for P in (3, 28, 120):
            uvs_a = torch.cat([torch.roll(one_a, 997 * p, 0) for p in range(P)])
            uvs_b = torch.cat([torch.roll(one_b, 997 * p, 0) for p in range(P)])
            parts = [(uvs_a[p * n:(p + 1) * n], uvs_b[p * n:(p + 1) * n]) for p in range(P)]
            pairs, counts = np.array([(0, 1)] * P, np.int32), np.full(P, n, np.int64)

            def batch():
                return eg.find_essential_matrices(K, pairs, uvs_a, uvs_b, counts, hypotheses=HYPOTHESES)

            def loop():
                return [eg.find_essential_matrix(a, b, K[0], K[1], hypotheses=HYPOTHESES, return_info=True) for a, b in parts]

            got, want = batch(), loop()
            assert all(got["E"][p].tobytes() == want[p]["E"].tobytes() for p in range(P)), "the batch and the loop disagree"
            _, _, table = eg._essential_batch_checks(K, pairs, uvs_a, uvs_b, counts, 1.0, HYPOTHESES)
            _, Es, hcounts, winner, args_batch, keep = eg._essential_batch_stages(uvs_a, uvs_b, counts, table, HYPOTHESES, 0)
            blocks = torch.from_numpy(eg.essential_score_blocks(counts)).cuda()

            def score(lds_sum):
                eg.call("camd_essential_batch_score", Es.device, *args_batch, blocks.data_ptr(), int(blocks.shape[0]), Es.data_ptr(),
                        HYPOTHESES, lds_sum, hcounts.data_ptr(), winner.data_ptr(), what="gpu_essential_batch_time")

            r = dict(pairs=P, matches_per_pair=n, hypotheses=HYPOTHESES, score_workgroups=int(blocks.shape[0]),
                     batched_call=timed(batch, args.reps, torch), loop_of_single_calls=timed(loop, args.reps, torch),
                     score_stage_lds_sum=timed(lambda: score(1), args.reps, torch),
                     score_stage_atomic_per_wave=timed(lambda: score(0), args.reps, torch))
            r["loop_over_batch"] = r["loop_of_single_calls"]["wall_ms_median"] / r["batched_call"]["wall_ms_median"]
            r["lds_sum_over_per_wave"] = r["score_stage_lds_sum"]["gpu_events_ms_median"] / r["score_stage_atomic_per_wave"]["gpu_events_ms_median"]
            points.append(r)
            print(json.dumps(r), flush=True)
            del keep, parts, uvs_a, uvs_b
    doc = dict(tool="tools/gpu_essential_batch_time.py", device=torch.cuda.get_device_name(0), reps=args.reps,
               what="matches resident on the device; whole calls by a host clock ending in a synchronise (they read their results "
                    "back), the score stage by stream events; medians after two warm-up calls; call times (allocation, launches, "
                    "read-backs), not kernel times", points=points)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
