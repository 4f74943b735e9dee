#!/usr/bin/env python3
"""Times ``bundle_adjust_pairs`` (csrc/bundle.hip) on the GPU -- wall time around a synchronised call after warm-up, the
matches resident in HBM as float32 tensors, the median of the repetitions -- and prints one JSON line:
    python tools/gpu_bundle_time.py [--out profiles/bundle_time.json] [--sizes 5000,200000,2000000] [--views 3,8]
Every pair of 3 and of 8 views with 5 000 / 200 000 / 2 000 000 matches a pair: random world points in front of a ring
of cameras, 0.3 px of noise at f = 1000 px, start poses off the truth by 0.005 rad and 0.005 units.  Per size: the call, the
evaluations it took, the time per evaluation, and from one profiled call the share of the kernels of stage 2
(k_bundle_linearise), of stage 4 (k_bundle_evaluate) and of the solve (k_bundle_solve) in the GPU time of all bundle
kernels, with the bytes per point and pass against the HBM rate.  In the same run, on this machine's CPU: the NumPy
restatement tests/bundle_ref.py at the smallest size.  Wall time, not event time: a call synchronises once per evaluation."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F, W, H = 1000.0, 1280, 960


def wall_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def problem(views, per_pair, seed, dev):
    """(K, T_true, T0, pairs, uvs_a, uvs_b float32 tensors on dev, counts): cameras on a ring of radius 1 looking at points
    in the box |x|, |y| < 1, 4 < z < 6"""
    import torch
    from reconstruction_cases import _rodrigues
    rng = np.random.default_rng(seed)
    K = np.array([[F, 0, W / 2], [0, F, H / 2], [0, 0, 1.0]])
    Ts, T0 = [], []
    for v in range(views):
        a = 2 * np.pi * v / views
        T = np.eye(4)
        T[:3, :3] = _rodrigues([0.1 * np.sin(a), -0.1 * np.cos(a), 0.05 * v])
        T[:3, 3] = [np.cos(a), np.sin(a), 0.1 * v]
        P = np.eye(4)
        P[:3, :3] = _rodrigues(rng.normal(size=3) * 0.003)
        P[:3, 3] = rng.uniform(-0.005, 0.005, 3)
        Ts.append(T), T0.append(T @ P)
    pairs = [(a, b) for a in range(views) for b in range(a + 1, views)]
    gen = torch.Generator(device=dev).manual_seed(seed)
    Kt = torch.from_numpy(K).to(dev)
    uas, ubs = [], []
    for a, b in pairs:
        X = torch.rand((per_pair, 3), generator=gen, device=dev, dtype=torch.float64) * torch.tensor([2.0, 2.0, 2.0], device=dev, dtype=torch.float64) + \
            torch.tensor([-1.0, -1.0, 4.0], device=dev, dtype=torch.float64)
        for v, out in ((a, uas), (b, ubs)):
            Tv = torch.from_numpy(np.linalg.inv(Ts[v])).to(dev)
            p = (X @ Tv[:3, :3].T + Tv[:3, 3]) @ Kt.T
            uv = p[:, :2] / p[:, 2:] + 0.3 * torch.randn((per_pair, 2), generator=gen, device=dev, dtype=torch.float64)
            out.append(uv.to(torch.float32))
    return np.array([K] * views), np.array(Ts), np.array(T0), np.array(pairs, np.int32), torch.cat(uas), torch.cat(ubs), \
        np.array([per_pair] * len(pairs), np.int64)


def kernel_shares(fn):
    """GPU time of the bundle kernels of one call by stage, from the profiler's kernel records"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
    total, by = 0.0, dict(linearise=0.0, evaluate=0.0, solve=0.0, pair_sum=0.0, other=0.0)
    for e in prof.key_averages():
        name = e.key
        t = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
        if "k_bundle" not in name and "BundleUsed" not in name:
            continue
        total += t
        for k in ("linearise", "evaluate", "solve", "pair_sum"):
            if "k_bundle_" + k in name:
                by[k] += t
                break
        else:
            by["other"] += t
    return dict(gpu_ms=total / 1e3, share={k: (v / total if total else None) for k, v in by.items()}, ms={k: v / 1e3 for k, v in by.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="5000,200000,2000000")
    ap.add_argument("--views", default="3,8")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    import calibrating_amd as ca
    import bundle_ref as ref
    dev = torch.device("cuda", 0)
    sizes, views = [int(s) for s in args.sizes.split(",")], [int(v) for v in args.views.split(",")]
    res = dict(device=torch.cuda.get_device_name(0), focal_px=F, sigma_px=0.3, rows=[],
               note="wall time per bundle_adjust_pairs call on float32 CUDA tensors, return_points=True, the median of the repetitions: "
                    "the host's checks, the start and status kernel, one read-back of the segment scan, the chunk table, then per "
                    "evaluation camd_bundle_step (six launches) and one 16-byte read-back; the CPU figure is single-threaded NumPy")
    for n in views:
        for m in sizes:
            K, Ts, T0, pairs, ua, ub, counts = problem(n, m, 7, dev)
            out = {}

            def run():
                out["r"] = ca.bundle_adjust_pairs(K, T0, pairs, ua, ub, counts)
            reps = 5 if m * len(pairs) <= 2_000_000 else 2
            med, lo, hi = wall_ms(run, 1, reps)
            r = out["r"]
            used = int((r["status"] == 0).sum())
            row = dict(views=n, pairs=len(pairs), matches_per_pair=m, used=used, evaluations=r["evaluations"], iterations=r["iterations"],
                       retval_px=r["retval"], call_ms=med, call_ms_min=lo, call_ms_max=hi, per_evaluation_ms=med / r["evaluations"],
                       pose_error_start=ref.pose_errors(T0, Ts), pose_error_result=ref.pose_errors(r["T"], Ts))
            try:
                k = kernel_shares(run)
                row["kernels"] = k
                ev = r["evaluations"]
                # float32 pixels 16 B + the point 24 B per pass; stage 4 also writes the candidate 24 B; partials are 104 x 8 B / 256
                if k["ms"]["linearise"] > 0:
                    row["linearise_GBps"] = used * (16 + 24 + 104 * 8 / 256) * (ev + 1) / (k["ms"]["linearise"] * 1e-3) / 1e9
                if k["ms"]["evaluate"] > 0:
                    row["evaluate_GBps"] = used * (16 + 24 + 24) * ev / (k["ms"]["evaluate"] * 1e-3) / 1e9
            except Exception as e:  # the profiler is optional: the wall times stand without it
                row["kernels"] = "not measured: %s" % (e,)
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del ua, ub, r, out
            torch.cuda.empty_cache()
    # the restatement on this machine's CPU at the smallest size
    n, m = views[0], sizes[0]
    K, Ts, T0, pairs, ua, ub, counts = problem(n, m, 7, dev)
    a, b = ua.cpu().numpy(), ub.cpu().numpy()
    t0 = time.perf_counter()
    want = ref.solve(K, T0, pairs, a, b, counts)
    res["numpy_restatement"] = dict(views=n, matches_per_pair=m, ms=(time.perf_counter() - t0) * 1e3, evaluations=want["evaluations"],
                                    cpu_threads=torch.get_num_threads())
    got = ca.bundle_adjust_pairs(K, T0, pairs, ua, ub, counts)
    res["numpy_restatement"]["largest_T_difference"] = float(np.abs(got["T"] - want["T"]).max())
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
