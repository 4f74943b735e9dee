#!/usr/bin/env python3
"""Times ``imgproc.corner_sub_pix`` and ``imgproc.cvt_gray`` (csrc/subpix.hip) on the GPU -- HIP events after warm-up,
images and corners resident in HBM -- and writes one JSON record:
    python tools/gpu_subpix_time.py [--out profiles/subpix_time.json]
An 11 x 8 board (88 corners per frame) at 1920 x 1080, the reference's arguments (window (4, 4), criteria (30, 0.01)),
seeds up to 2 px from the corners; 1, 100 and 1 000 frames; the refinement alone on gray frames and with the gray
conversion on colour frames.  In the same run, on this machine's CPU: the NumPy restatement tests/subpix_ref.py per frame.
The event time is that of the Python binding: the allocations and the launches (the mask is made on the host and uploaded
once per window and device, in the warm-up).  Every frame is a copy of one rendered image with one set of seeds: all
waves run the same rounds and the pixels stay in cache, a best case."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES = (1, 100, 1000)
W, H, COLS, ROWS = 1920, 1080, 11, 8


def gpu_ms(fn, warmup=2, reps=5):
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
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    from calibrating_amd import imgproc
    import subpix_cases as sc
    import subpix_ref as ref

    K = np.array([[1400.0, 0, 959.5], [0, 1400.0, 539.5], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = sc.rodrigues((0.2, -0.25, 0.05)), (0.01, -0.005, 0.5)
    Hm = K @ np.stack([T[:3, 0], T[:3, 1], T[:3, 3]], 1)
    xy = np.mgrid[:COLS, :ROWS].T.reshape(-1, 2) * sc.SQUARE
    p = np.concatenate([xy - xy.mean(0), np.ones((len(xy), 1))], 1) @ Hm.T
    truth = p[:, :2] / p[:, 2:]
    img = sc.render(Hm, H, W, COLS, ROWS, ss=2)
    seeds = (truth + np.random.default_rng(0).uniform(-2, 2, truth.shape)).astype(np.float32)

    t0 = time.perf_counter()
    want = ref.corner_sub_pix(img, seeds, order="wave")
    cpu_restatement_s = time.perf_counter() - t0
    got = imgproc.corner_sub_pix(img, seeds, return_info=True)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), "the kernel and the restatement disagree"
    end = np.linalg.norm(got[0] - truth, axis=1)

    rec = dict(board=[COLS, ROWS], size=[W, H], corners_per_frame=len(seeds), window=[4, 4], criteria=[30, 0.01],
               iterations_mean=float(got[1].mean()), iterations_max=int(got[1].max()), error_px_max=float(end.max()),
               cpu_numpy_restatement_ms_per_frame=1e3 * cpu_restatement_s, device=torch.cuda.get_device_name(0), runs=[])
    g1, c1 = torch.from_numpy(img).cuda(), torch.from_numpy(sc.colour(img)).cuda()
    s1 = torch.from_numpy(seeds).cuda()
    for f in FRAMES:
        gray, rgb, s = g1[None].repeat(f, 1, 1), c1[None].repeat(f, 1, 1, 1), s1[None].repeat(f, 1, 1)
        lo, hi = gpu_ms(lambda: imgproc.corner_sub_pix(gray, s))
        glo, ghi = gpu_ms(lambda: imgproc.cvt_gray(rgb))
        blo, bhi = gpu_ms(lambda: imgproc.corner_sub_pix(rgb, s))
        rec["runs"].append(dict(frames=f, refine_ms=[lo, hi], gray_ms=[glo, ghi], gray_and_refine_ms=[blo, bhi],
                                refine_us_per_corner=1e3 * lo / (f * len(seeds)),
                                gray_GBps=4.0 * W * H * f / (glo * 1e-3) / 1e9))
        del gray, rgb, s
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
