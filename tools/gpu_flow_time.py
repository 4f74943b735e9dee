#!/usr/bin/env python3
"""Times ``warp_flow`` (csrc/flow.hip) on the GPU -- HIP events after warm-up, everything resident in HBM -- and prints
one JSON line:
    python tools/gpu_flow_time.py [--out profiles/flow_time.json]
1920x1080 RGB with a float32 flow of a few pixels, batch 1 and batch 64, both branches, INTER_LINEAR.  Beside each time:
the byte floor of DESIGN.md (backward: 8 B of flow + 3 B read + 3 B written per pixel; forward: 4 B memset + 8 B of flow
+ 4 B atomic, then 4 + 3 + 3) and its share of the 6.29 TB/s copy ceiling.  For the backward branch the same run times
the composition a user had to write before: the float64 map built with torch operations, rounded to float32, then one
``imgproc.remap`` per image -- and says whether its bytes equal the fused kernel's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_GBS = 6290.0  # measured copy ceiling of the part
H, W, CN = 1080, 1920, 3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,64")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    import calibrating_amd as ca
    from calibrating_amd import imgproc
    from calibrating_amd._native import INTER_LINEAR

    dev = torch.device("cuda", 0)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                            indexing="ij")

    def composition(flow, imgs):
        mx = (xs + flow[:, 0].double() * W).float()
        my = (ys + flow[:, 1].double() * H).float()
        return torch.stack([imgproc.remap(imgs[i], mx[i], my[i], INTER_LINEAR) for i in range(len(imgs))])

    res = dict(device=torch.cuda.get_device_name(0), copy_ceiling_GBs=COPY_CEILING_GBS, shape=[H, W, CN], flow_dtype="float32",
               interpolation="INTER_LINEAR",
               note="event time per call of the Python binding (allocations from torch's pool + the launches); floor_bytes "
                    "as in DESIGN.md; ceiling_frac = floor_bytes / ms_min over the copy ceiling; composition = float64 map "
                    "with torch operations -> float32 -> one imgproc.remap per image + torch.stack")
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for n in (int(s) for s in args.batches.split(",")):
        imgs = torch.randint(0, 256, (n, H, W, CN), dtype=torch.uint8, device=dev, generator=g)
        phase = torch.rand((n, 1, 1), device=dev, generator=g, dtype=torch.float64) * 6
        flow = torch.stack([(3.7 * torch.sin(ys / 110 + phase) + 2.3 * torch.cos(xs / 70) + 1.1) / W,
                            (2.9 * torch.cos(xs / 130 + phase) - 1.7 * torch.sin(ys / 50) - 0.6) / H], 1).float().contiguous()
        px = n * H * W
        reps = 200 if n == 1 else 10
        calls = (("backward", lambda: ca.warp_flow(flow, img2=imgs), px * (8 + CN + CN)),
                 ("forward", lambda: ca.warp_flow(flow, img1=imgs), px * (4 + 8 + 4 + 4 + CN + CN)),
                 ("backward_composition", lambda: composition(flow, imgs), None))
        fused = None
        for name, fn, floor_bytes in calls:
            lo, hi = gpu_ms(fn, warmup=3, reps=reps)
            row = dict(call=name, batch=n, ms_min=lo, ms_max=hi)
            if floor_bytes is not None:
                row.update(floor_bytes=floor_bytes, ceiling_frac=floor_bytes / (lo * 1e-3) / 1e9 / COPY_CEILING_GBS)
            if name == "backward":
                fused = fn()
            if name == "backward_composition":
                row["bytes_equal_fused"] = bool(torch.equal(fn(), fused))
            rows.append(row)
        del imgs, flow, fused
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
