#!/usr/bin/env python3
"""Times ``imgproc.undistort_points`` / ``imgproc.project_points`` (csrc/points.hip) on the GPU -- HIP events after
warm-up, points resident in HBM -- and prints one JSON line:
    python tools/gpu_points_time.py [--out profiles/points_time.json]
5 000, 200 000 and 2 000 000 points (a sparse matcher, a dense one, every pixel of a 1080p flow), float32 and float64,
5 and 12 distortion coefficients, cv2's 5 iterations.  Beside each time: the byte floor of the call (one input row + one
output row per point) and what share of the HBM peak it would be, whether the GPU result is bit-identical to the NumPy
restatement (tests/points_ref.py), and that restatement's time on this machine's CPU.  The event time is that of the
Python binding: one output allocation from torch's pool + one launch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, as bench.py
SIZES = (5000, 200000, 2000000)


def gpu_ms(fn, warmup=5, reps=50):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(3):  # three windows: the spread says how much the number can be trusted
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return min(times), max(times)


def cpu_s(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    from calibrating_amd import imgproc
    import points_cases as pc
    import points_ref as ref

    res = dict(device=torch.cuda.get_device_name(0), hbm_peak_GBs=HBM_PEAK_GBS, iters=5,
               note="event time per call of the Python binding (one output allocation from torch's pool + one launch); "
                    "floor_bytes = one input row + one output row per point; hbm_frac = floor_bytes / ms_min over the HBM "
                    "peak -- sets of a few MB stay in the last-level cache between calls, so it is a rate, not HBM traffic; "
                    "cpu_restatement_s = tests/points_ref.py, single-threaded NumPy on this machine")
    rows = []
    eye, zero = np.eye(3), np.zeros(3)
    for n in (int(s) for s in args.sizes.split(",")):
        for dtype in (np.float32, np.float64):
            uv, xyz = pc.pixels(n, 1, dtype), pc.points3d(n, 2, dtype)
            tuv, txyz = torch.from_numpy(uv).cuda(), torch.from_numpy(xyz).cuda()
            eb = np.dtype(dtype).itemsize
            for ndist in (5, 12):
                D = pc.lens(ndist)
                calls = (("undistort_points", lambda: imgproc.undistort_points(tuv, pc.K, D), lambda: ref.undistort_points(uv, pc.K, D),
                          (2 + 2) * eb * n),
                         ("project_points", lambda: imgproc.project_points(txyz, eye, zero, pc.K, D),
                          lambda: ref.project_points(xyz, eye, zero, pc.K, D), (3 + 2) * eb * n))
                for name, gpu, cpu, floor_bytes in calls:
                    lo, hi = gpu_ms(gpu, reps=200 if n <= 200000 else 50)
                    secs, want = cpu_s(cpu)
                    rows.append(dict(call=name, n=n, dtype=np.dtype(dtype).name, ndist=ndist, ms_min=lo, ms_max=hi,
                                     floor_bytes=floor_bytes, hbm_frac=floor_bytes / (lo * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                     cpu_restatement_s=secs,
                                     bit_identical_to_restatement=bool(np.array_equal(gpu().cpu().numpy(), want, equal_nan=True))))
            del tuv, txyz
    res["rows"] = rows
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
