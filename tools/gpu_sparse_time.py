#!/usr/bin/env python3
"""Times the nearest fill of calibrating_amd.sparse.interpolate_uvzs on the GPU and writes
profiles/sparse_interp_time.json (the README row is filled from that file).

    python tools/gpu_sparse_time.py [--out profiles/sparse_interp_time.json] [--reps 200]

Points: the reference's 480x640 // 8 grid with 5 000 matches; 1920x1080 at full resolution with 5 000, 200 000 and
2 000 000 samples; the fused upsizing (1080p // 8 grid written at 1920x1080).  Per point: the time of one call with the
samples already on the device -- a host clock around ``reps`` calls that ends in a device synchronise, after a warm-up of
the same shape -- next to its output-write floor (4 bytes per pixel at the HBM peak) and, from the SAME run, the
reference's own way on this box's CPU: SciPy ``KDTree(...).query`` when SciPy imports, else the brute-force NumPy
restatement (tests/sparse_ref.py; only where it is affordable).  A call includes the non-finite check (one flag read
back), the binning kernels, torch's cumsum between them and the fill; it is a call time, not a kernel time.
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

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak, for the output-write floor

POINTS = [
    dict(name="ref_grid_60x80_5k", grid=(60, 80), out=None, n=5000),
    dict(name="1080p_full_5k", grid=(1080, 1920), out=None, n=5000),
    dict(name="1080p_full_200k", grid=(1080, 1920), out=None, n=200000),
    dict(name="1080p_full_2M", grid=(1080, 1920), out=None, n=2000000),
    dict(name="1080p_div8_fused_upsize_5k", grid=(135, 240), out=(1080, 1920), n=5000),
]


def cpu_way(uvzs, grid, budget_s=120.0):
    """(seconds, how) of the reference's fill on the CPU: KDTree build + query of every grid pixel."""
    ys, xs = np.mgrid[:grid[0], :grid[1]]
    q = np.float32(np.stack([xs.ravel(), ys.ravel()], 1))
    try:
        from scipy.spatial import KDTree
    except ImportError:
        if grid[0] * grid[1] * len(uvzs) > 5e9:
            return None, "not measured (no SciPy on this box; brute force not affordable at this size)"
        import sparse_ref
        t0 = time.perf_counter()
        sparse_ref.nearest_brute(uvzs, grid, 2)
        return time.perf_counter() - t0, "NumPy brute-force restatement (no SciPy on this box)"
    t0 = time.perf_counter()
    d, i = KDTree(uvzs[:, :2]).query(q)
    out = np.zeros(len(q), np.float32)
    out[d < 2] = uvzs[i[d < 2], 2]
    return time.perf_counter() - t0, "scipy.spatial.KDTree build + query, 1 thread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_interp_time.json"))
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_sparse_time.py measures on the GPU; none is visible")
    from calibrating_amd import sparse
    import sparse_cases as sc
    rows = []
    for p in POINTS:
        uvzs = sc.samples(1000 + p["n"] % 997, p["n"], p["grid"], np.float64, margin=4.0)
        dev = torch.from_numpy(uvzs).cuda()
        call = lambda: sparse.interpolate_uvzs(dev, p["grid"], inter_type="nearest", resize_hw=p["out"])  # noqa: E731
        for _ in range(10):
            res = call()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):  # five windows: the spread says how much to trust the median
            t0 = time.perf_counter()
            for _ in range(args.reps):
                res = call()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / args.reps)
        oh, ow = tuple(res.shape)
        floor = oh * ow * 4 / HBM_PEAK_BYTES_PER_S
        cpu_s, how = cpu_way(uvzs, p["grid"])
        rows.append(dict(name=p["name"], grid_hw=list(p["grid"]), out_hw=[oh, ow], samples=p["n"],
                         gpu_call_ms_median=1e3 * float(np.median(times)), gpu_call_ms_min=1e3 * min(times),
                         gpu_call_ms_max=1e3 * max(times), output_write_floor_ms=1e3 * floor,
                         times_floor=float(np.median(times)) / floor,
                         cpu_reference_way_ms=None if cpu_s is None else 1e3 * cpu_s, cpu_reference_way=how,
                         cpu_grid_note="the CPU figure fills the GRID (%dx%d); the reference then resizes" % p["grid"]
                         if p["out"] else None))
        print(json.dumps(rows[-1]))
    doc = dict(tool="tools/gpu_sparse_time.py", device=torch.cuda.get_device_name(0), reps_per_window=args.reps, windows=5,
               what="host clock around reps calls of sparse.interpolate_uvzs(nearest) ending in a device synchronise; "
                    "samples resident on the device; call time (checks, binning, cumsum, fill), not kernel time",
               hbm_peak_bytes_per_s=HBM_PEAK_BYTES_PER_S, points=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
