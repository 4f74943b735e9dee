#!/usr/bin/env python3
"""Times ``Stereo.distort_depth`` on the GPU (HIP events after warm-up) and prints one JSON line:
    python tools/gpu_distort_depth_time.py [--out profiles/distort_depth_time.json]
  * the per-call gather (camd_distort_depth) at 1920x1080 float64, batch 1 and batch 64, and float32 for comparison,
    the batch of 64 as a fraction of its own HBM floor: one value read + one written + 4 B of index per pixel and image
    (the index is charged once per image here although a workgroup shares it between up to 16 images);
  * camd_unrectify_depth on the same shapes -- the same shape of kernel (8 B read + 8 B written + 8 B of maps);
  * the one-time table build (camd_distort_index_map + the read of its counters);
  * for context, the NumPy restatement on this machine's CPU (np.unique alone, and the whole function)."""
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


def gpu_ms(fn, warmup=5, reps=30):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    import calibrating_amd as ca
    from calibrating_amd import imgproc, synthetic
    import distort_depth_ref as ref

    w, h = (int(v) for v in args.size.split("x"))
    rec = synthetic.rig(w, h)
    st = ca.Stereo.load(rec)
    K, D = st.cam1.K, st.cam1.D
    res = dict(size=[w, h], device=torch.cuda.get_device_name(0), hbm_peak_GBs=HBM_PEAK_GBS)

    lo, hi = gpu_ms(lambda: imgproc.distort_index_map(K, D, (w, h)), warmup=2, reps=5)
    res["table_build_ms"] = dict(min=lo, max=hi, note="two kernels + the read of the counters (one synchronisation)")
    idx = st._distort_table("cuda")
    mx, my = st._unrectify_tables("cuda")
    M = (st.R1.T @ np.linalg.inv(st.K))[2]
    n = w * h
    rows = []
    for dtype, batch in ((torch.float64, 1), (torch.float64, 64), (torch.float32, 1), (torch.float32, 64)):
        z = torch.rand((batch, h, w), dtype=dtype, device="cuda")
        eb = z.element_size()
        lo, hi = gpu_ms(lambda: imgproc.distort_depth(z, idx), reps=200 if batch == 1 else 20)
        floor_bytes = (2 * eb + 4) * n * batch
        # a fraction of the HBM floor only where the working set leaves the 256 MB last-level cache (batch 64: GBs);
        # a batch-1 call is launch-bound and its 40 MB stay cached between calls: no HBM figure is claimed for it
        frac = (lambda fb, ms: fb / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS if batch > 1 else None)
        row = dict(kernel="camd_distort_depth", dtype=str(dtype).replace("torch.", ""), batch=batch, ms_min=lo, ms_max=hi,
                   floor_bytes=floor_bytes, hbm_frac=frac(floor_bytes, lo))
        if batch > 1:  # the timed shape is also a checked shape: every image against a torch gather through the table
            flat = idx.reshape(-1).long()
            want = torch.where(flat >= 0, z.reshape(batch, -1)[:, flat.clamp(min=0)], torch.zeros((), dtype=dtype, device="cuda"))
            row["bit_identical_to_torch_gather"] = bool(torch.equal(imgproc.distort_depth(z, idx).reshape(batch, -1), want))
            del want
        rows.append(row)
        if dtype == torch.float64:
            lo, hi = gpu_ms(lambda: imgproc.unrectify_depth(z, M, mx, my), reps=200 if batch == 1 else 20)
            fb = (8 + 8 + 8) * n * batch
            rows.append(dict(kernel="camd_unrectify_depth", dtype="float64", batch=batch, ms_min=lo, ms_max=hi, floor_bytes=fb,
                             hbm_frac=frac(fb, lo)))
        del z
    res["per_call"] = rows
    res["per_call_note"] = ("event time per call of the Python binding (one output allocation from torch's pool + one launch); at "
                            "batch 1 that is launch-bound host time as much as kernel time")

    # CPU context: the restatement on this machine
    t0 = time.perf_counter()
    pts = ref._int_points(K, D, w, h)
    t1 = time.perf_counter()
    np.unique(pts, axis=0, return_index=True)
    t2 = time.perf_counter()
    z = np.random.default_rng(0).random((h, w))
    t3 = time.perf_counter()
    want = ref.distort_depth(z, K, D, (w, h))
    t4 = time.perf_counter()
    res["cpu_restatement_s"] = dict(points=t1 - t0, np_unique=t2 - t1, whole_function=t4 - t3, note="single-threaded NumPy")
    got = st.distort_depth(z)
    res["bit_identical_to_restatement"] = bool(np.array_equal(got, want))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
