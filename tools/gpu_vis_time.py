#!/usr/bin/env python3
"""Times the pictures of ``calibrating_amd.vis`` (csrc/vis.hip) on the GPU -- HIP events after warm-up, everything resident
in HBM -- and prints one JSON line:
    python tools/gpu_vis_time.py [--out profiles/vis_time.json]
1920x1080 float64 depths, batch 1 and batch 64: ``vis_depth_l1`` with the default top-5 % limit and with a fixed
``max_l1``, ``vis_depth`` with ``fix_range``, ``vis_align`` of two RGB pictures.  Beside each time: the byte floor of
DESIGN.md and its share of the 6.29 TB/s copy ceiling; in the same run a torch composition that gives the same bytes
(``torch.kthvalue`` for the limit) and the NumPy restatement (tests/vis_ref.py) on this box's CPU, one image."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_CEILING_GBS = 6290.0  # measured copy ceiling of the part
H, W = 1080, 1920
SELECT_PASSES = 8


def gpu_ms(fn, warmup, reps):
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


def cpu_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,64")
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    import calibrating_amd as ca
    from calibrating_amd import vis
    import vis_ref

    dev = torch.device("cuda", 0)
    jet = torch.from_numpy(vis.colormap_table(vis.COLORMAP_JET).copy()).to(dev)

    def l1_composition(re, gt, max_l1):
        """vis_depth_l1(re, gt, max_l1, colorbar=None) with torch operations, image by image for the limit."""
        mask = (re != 0) & (gt != 0)
        l1 = (re - gt) * mask
        a = l1.abs()
        if max_l1 > 0:
            m = torch.full((len(re), 1, 1), max_l1, dtype=torch.float64, device=dev)
        else:
            ms = []
            for i in range(len(re)):
                v = a[i][mask[i]]
                k = int(-max_l1 * v.numel())  # (a host read of valid_num per image)
                ms.append(torch.kthvalue(v, v.numel() - k).values)
            m = torch.stack(ms).view(-1, 1, 1)
        pos, neg = l1 > 0, l1 < 0
        planes = torch.stack([l1 * pos, -l1 * neg, l1 * 0], -1)
        norm = torch.minimum(planes.clamp(min=0), m[..., None]) / m[..., None]
        out = ((norm * (1 - 0.1) + 0.1) * mask[..., None] * 255).to(torch.uint8)
        over = a > m
        out[..., 1] = torch.where(over & pos, 255, out[..., 1])
        out[..., 2] = torch.where(over & pos, 0, out[..., 2])
        out[..., 0] = torch.where(over & neg, 230, out[..., 0])
        out[..., 2] = torch.where(over & neg, 230, out[..., 2])
        return out

    def depth_composition(d, hi):
        n = (d.clamp(0, hi) - 0.0) / (hi - 0.0)
        out = jet[(n * 255.9).to(torch.uint8).long()]
        out[d == 0] = 0
        return out

    res = dict(device=torch.cuda.get_device_name(0), copy_ceiling_GBs=COPY_CEILING_GBS, shape=[H, W], dtype="float64",
               note="event time per call of the Python binding (allocations from torch's pool, the launches and, for "
                    "vis_depth_l1, the one flag read); floor_bytes as in DESIGN.md 4.3f; ceiling_frac = floor_bytes / ms_min "
                    "over the copy ceiling; *_composition = torch operations giving the same bytes; numpy_ms = "
                    "tests/vis_ref.py on this box's CPU, one image")
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                            indexing="ij")
    for n in (int(s) for s in args.batches.split(",")):
        phase = torch.rand((n, 1, 1), device=dev, generator=g, dtype=torch.float64) * 6
        gt = 2.5 + 1.5 * torch.sin(xs / 170 + phase) * torch.cos(ys / 110)
        re = gt + 0.04 * torch.randn((n, H, W), device=dev, generator=g, dtype=torch.float64)
        re = re * (torch.rand((n, H, W), device=dev, generator=g) > 0.05)
        gt = gt * (torch.rand((n, H, W), device=dev, generator=g) > 0.05)
        img1 = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
        img2 = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
        px = n * H * W
        reps = 50 if n == 1 else 5
        error, colour, select = 16 + 9, 9 + 3, SELECT_PASSES * 9  # bytes per pixel: DESIGN.md 4.3f
        calls = (("vis_depth_l1_top5", lambda: ca.vis_depth_l1(re, gt, colorbar=None), px * (error + select + colour)),
                 ("vis_depth_l1_top5_composition", lambda: l1_composition(re, gt, -0.05), None),
                 ("vis_depth_l1_fixed", lambda: ca.vis_depth_l1(re, gt, max_l1=0.05, colorbar=None), px * (error + colour)),
                 ("vis_depth_l1_fixed_composition", lambda: l1_composition(re, gt, 0.05), None),
                 ("vis_depth_fix_range", lambda: ca.vis_depth(re, fix_range=5.0), px * (8 + 3)),
                 ("vis_depth_fix_range_composition", lambda: depth_composition(re, 5.0), None),
                 ("vis_align", lambda: ca.vis_align(img1, img2), px * (4 * 3 + 4 * 3)))
        last = None
        for name, fn, floor_bytes in calls:
            lo, hi = gpu_ms(fn, warmup=2, reps=reps)
            row = dict(call=name, batch=n, ms_min=lo, ms_max=hi)
            if floor_bytes is not None:
                row.update(floor_bytes=floor_bytes, ceiling_frac=floor_bytes / (lo * 1e-3) / 1e9 / COPY_CEILING_GBS)
                last = fn()
            else:
                row["bytes_equal_kernel"] = bool(torch.equal(fn(), last))
            rows.append(row)
        if n == 1:
            r, t, a, b = (x[0].cpu().numpy() for x in (re, gt, img1, img2))
            for name, fn in (("vis_depth_l1_top5", lambda: vis_ref.vis_depth_l1(r, t, colorbar=None)),
                             ("vis_depth_l1_fixed", lambda: vis_ref.vis_depth_l1(r, t, max_l1=0.05, colorbar=None)),
                             ("vis_depth_fix_range", lambda: vis_ref.vis_depth(r, fix_range=5.0)),
                             ("vis_align", lambda: vis_ref.vis_align(a, b))):
                rows.append(dict(call=name + "_numpy", batch=1, numpy_ms=min(cpu_ms(fn) for _ in range(2))))
        del re, gt, img1, img2, last
        torch.cuda.empty_cache()
    res["rows"] = rows
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
