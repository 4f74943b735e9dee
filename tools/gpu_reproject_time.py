#!/usr/bin/env python3
"""Times ``pointcloud.get_reproject_remap`` on the GPU (HIP events after warm-up) and prints one JSON line:
    python tools/gpu_reproject_time.py [--out profiles/reproject_time.json]
  * camd_reproject_remap at 1920x1080 -> 1920x1080, interpolation rates 1 and 1.5, batch 1 and batch 64, each next to
    the bytes its passes must move at the least (below), that count as a fraction of the 8 TB/s HBM peak and of the
    6.29 TB/s measured copy ceiling;
  * camd_project_depth on the same inputs -- the same shape of kernel without the owner pass and with one float64
    plane out -- as the yardstick, one call per image (it takes no batch);
  * the map -> picture step (camd_remap_u8, INTER_LINEAR, RGB) for one image;
  * for context, the NumPy restatement (tests/reproject_ref.py) per frame on this machine's CPU.

Least bytes per image, s = source pixels, t = target pixels (sampling-grid cells beyond the source pixels re-read a
depth value that is already in cache and are not charged):
    clear     12 t   keys (8) and owner (4) written
    pass 1     8 s + 16 t   depth read; every key read and written by its atomicMin at least once
    pass 2     8 s + 8 t + 8 t   depth read again; keys read; owner read and written by its atomicMax
    pass 3     4 t + 8 t   owner read, two float32 planes written
    = 16 s + 56 t;   camd_project_depth: 8 t + (8 s + 16 t) + (8 t + 8 t) = 8 s + 40 t"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak, as bench.py
COPY_CEILING_GBS = 6290.0  # measured copy ceiling of the part


def gpu_ms(fn, warmup=3, reps=30):
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
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    from calibrating_amd import imgproc, pointcloud
    import reproject_cases as cases
    import reproject_ref as ref

    w, h = (int(v) for v in args.size.split("x"))
    xy = (w, h)
    K1 = np.array([[1400.0, 0, w / 2 + 1.3], [0, 1404.0, h / 2 - 1.1], [0, 0, 1]])
    K2 = np.array([[1350.0, 0, w / 2 - 10.0], [0, 1350.0, h / 2 + 5.0], [0, 0, 1]])
    T = cases.pose()
    n = w * h
    depth = cases.scene_depth(11, h, w)
    res = dict(size=[w, h], device=torch.cuda.get_device_name(0), hbm_peak_GBs=HBM_PEAK_GBS, copy_ceiling_GBs=COPY_CEILING_GBS,
               bytes_per_image=dict(reproject_remap="16 s + 56 t", project_depth="8 s + 40 t", s=n, t=n))

    def fracs(nbytes, ms):
        gbs = nbytes / (ms * 1e-3) / 1e9
        return dict(least_bytes=nbytes, GBs=gbs, frac_of_hbm_peak=gbs / HBM_PEAK_GBS, frac_of_copy_ceiling=gbs / COPY_CEILING_GBS)

    rows = []
    d1 = torch.from_numpy(depth).cuda()
    for rate in (1, 1.5):
        for batch in (1, args.batch):
            d = d1 if batch == 1 else torch.stack([torch.roll(d1, 5 * i, dims=1) for i in range(batch)])
            reps = 100 if batch == 1 else 10
            lo, hi = gpu_ms(lambda: pointcloud.get_reproject_remap(K1, K2, T, d, xy, interpolation_rate=rate), reps=reps)
            row = dict(kernel="camd_reproject_remap", rate=rate, batch=batch, ms_min=lo, ms_max=hi, **fracs((16 + 56) * n * batch, lo))
            if batch > 1:  # the timed shape is a checked shape: image 0 of the batch against the single call
                many = pointcloud.get_reproject_remap(K1, K2, T, d, xy, interpolation_rate=rate)
                one = pointcloud.get_reproject_remap(K1, K2, T, d1, xy, interpolation_rate=rate)
                row["image0_bit_identical_to_single_call"] = bool(torch.equal(many[0], one))
                del many
            rows.append(row)

            def yardstick():
                for i in range(batch):
                    pointcloud.project_depth(d[i] if batch > 1 else d, K2, T, K1, xy, interpolation_rate=rate)
            lo, hi = gpu_ms(yardstick, reps=reps)
            rows.append(dict(kernel="camd_project_depth", rate=rate, batch=batch, calls=batch, ms_min=lo, ms_max=hi,
                             **fracs((8 + 40) * n * batch, lo)))
            del d
        maps = pointcloud.get_reproject_remap(K1, K2, T, d1, xy, interpolation_rate=rate)
        img = torch.from_numpy(cases.image(2, xy, cn=3)).cuda()
        lo, hi = gpu_ms(lambda: imgproc.remap(img, maps[0], maps[1], imgproc.INTER_LINEAR), reps=100)
        rows.append(dict(kernel="camd_remap_u8 INTER_LINEAR RGB", rate=rate, batch=1, ms_min=lo, ms_max=hi))
    res["per_call"] = rows
    res["per_call_note"] = ("event time per call of the Python binding (output and workspace allocations from torch's pool + the "
                            "launches); a batch-1 call is launch-bound and its working set stays in the last-level cache: its "
                            "bandwidth figures say how far it is from mattering, not how well it uses HBM")

    cpu = {}
    for rate in (1, 1.5):
        t0 = time.perf_counter()
        want = ref.get_reproject_remap(K1, K2, T, depth, xy, rate, kind="stable")
        cpu["rate_%s_s" % rate] = time.perf_counter() - t0
        got = pointcloud.get_reproject_remap(K1, K2, T, depth, xy, interpolation_rate=rate)
        cpu["rate_%s_share_of_pixels_bit_equal" % rate] = float((got == want).all(0).mean())
    cpu["note"] = "tests/reproject_ref.get_reproject_remap(kind='stable'), single-threaded NumPy, per frame"
    res["cpu_restatement"] = cpu
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
