#!/usr/bin/env python3
"""Times the plane fill inside the samples' convex hull (csrc/hull.hip) and the board depth built on it -- HIP events after
warm-up, everything resident in HBM -- and prints one JSON line:
    python tools/gpu_hull_time.py [--out profiles/hull_time.json] [--frames 1,64,1000]
An 88-point board (11 x 8 inner corners) at 1920 x 1080, with 1, 64 and 1000 frames: stage A (``camd_hull_fit``), the
fill (``camd_hull_fill``, reciprocal), and ``Cam.get_calibration_board_depth_batch`` end to end from gray images.  Beside
each: the 4 B per pixel write floor and its share of the 6.29 TB/s copy ceiling; and, in the same run,
``sparse.interpolate_uvzs(inter_type="lstsq")`` called once per frame -- today's nearest equivalent, which writes the same
bytes without a mask."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_CEILING_GBS = 6290.0  # measured copy ceiling of the part
H, W = 1080, 1920
PATTERN = (11, 8)
SQUARE = 0.025


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


def render_frames(K, poses):
    """gray (len(poses), H, W) uint8 boards, rendered as tests/subpix_cases.py renders them (2 x 2 samples per pixel)"""
    import numpy as np
    import subpix_cases as sc
    out = []
    for rvec, t in poses:
        R = sc.rodrigues(rvec)
        out.append(sc.render(K @ np.stack([R[:, 0], R[:, 1], np.asarray(t, np.float64)], 1), H, W, PATTERN[0], PATTERN[1], ss=2))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", default="1,64,1000")
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    import calibrating_amd as ca
    from calibrating_amd import _native, sparse

    dev = torch.device("cuda", 0)
    K = np.array([[1500.0, 0, 959.5], [0, 1500.0, 539.5], [0, 0, 1]])
    cam = ca.Cam(K, np.zeros((1, 5)), (W, H))
    board = ca.Chessboard(PATTERN, size_mm=SQUARE * 1000, detector="chess")
    poses = [((0.0, 0.0, 0.05), (0.01, -0.01, 1.0)), ((0.3, -0.1, -0.08), (-0.02, 0.02, 1.1)),
             ((-0.15, 0.35, 0.12), (0.02, 0.01, 1.2)), ((-0.3, -0.25, -0.04), (0.0, -0.02, 1.1))]
    rendered = torch.from_numpy(render_frames(K, poses)).to(dev)
    floor_per_frame = H * W * 4
    result = dict(hw=[H, W], points=PATTERN[0] * PATTERN[1], copy_ceiling_GBs=COPY_CEILING_GBS, cases=[])
    for f in [int(v) for v in args.frames.split(",")]:
        images = rendered[torch.arange(f, device=dev) % len(poses)].contiguous()
        res = cam.get_calibration_board_depth_batch(images, board=board)
        found = int(res["found"].sum().item())
        rows = cam._board_rows(res["T"], torch.from_numpy(board.object_points).to(dev))
        samples = torch.stack([torch.round(rows[..., 0]), torch.round(rows[..., 1]), 1 / rows[..., 2]], -1).contiguous()
        flat, lengths = samples.reshape(-1, 3), np.full(f, samples.shape[1], np.int64)
        rec = sparse._hull_fit(flat, lengths, (H, W), True, False)
        out = torch.empty((f, H, W), dtype=torch.float32, device=dev)
        reps = 20 if f <= 64 else 3

        def fill():
            _native.call("camd_hull_fill", dev, rec["vertices"].data_ptr(), rec["hull_counts"].data_ptr(), rec["abc"].data_ptr(),
                         rec["capacity"], f, W, H, 1, None, out.data_ptr())

        def per_frame_lstsq():
            for i in range(f):
                sparse.interpolate_uvzs(samples[i], (H, W), inter_type="lstsq")

        floor_ms = f * floor_per_frame / (COPY_CEILING_GBS * 1e9) * 1e3
        case = dict(frames=f, found=found, write_floor_bytes=f * floor_per_frame, write_floor_ms=floor_ms)
        for name, fn in (("stage_a", lambda: sparse._hull_fit(flat, lengths, (H, W), True, False)), ("fill", fill),
                         ("fit_and_fill", lambda: sparse.interpolate_uvzs_in_hull(samples, (H, W), reciprocal=True, keep_last_per_pixel=True)),
                         ("board_depth_batch", lambda: cam.get_calibration_board_depth_batch(images, board=board)),
                         ("interpolate_uvzs_lstsq_per_frame", per_frame_lstsq)):
            lo, hi = gpu_ms(fn, 2, reps if name != "interpolate_uvzs_lstsq_per_frame" or f <= 64 else 1)
            case[name + "_ms"] = [lo, hi]
        case["fill_share_of_ceiling"] = floor_ms / case["fill_ms"][0]
        result["cases"].append(case)
        del images, res, rows, samples, out
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
