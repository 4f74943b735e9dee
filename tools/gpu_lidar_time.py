#!/usr/bin/env python3
"""Times the LiDAR path (csrc/lidar.hip, calibrating_amd/lidar.py) -- HIP events after warm-up, everything resident in HBM --
and prints one JSON line:
    python tools/gpu_lidar_time.py [--out profiles/lidar_time.json] [--points 100000,1000000,10000000] [--rates 0.5,1]
The example's 1624 x 900 camera, a synthetic sweep of n points in front of it.  Per (n, rate): each stage (the rows;
the hull record; bins and the fill inside the hull; the resize) and the whole call; in the same run
``sparse.interpolate_uvzs("nearest")`` on the same rows and grid (the search without the hull: the fill inside the hull skips
the pixels outside, so it should cost no more); and the reference's route, SciPy's KDTree over the rows queried at every
pixel, on this machine's CPU.  Each case runs in a child process of its own under a time limit; the first that fails ends
the run."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1624, 900
K = [[803.5323604817661, 0.0, 821.5502789828007], [0.0, 803.8263591371266, 468.6433131586491], [0.0, 0.0, 1.0]]
CASE_SECONDS = 240


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
    return [min(times), max(times)]


def sweep(n, seed=0):
    """(n, 3) float32 points in front of the camera, a fifth of them beside the image or behind it"""
    import numpy as np
    rng = np.random.default_rng(seed)
    z = rng.uniform(2.0, 60.0, n)
    x = rng.uniform(-1.15, 1.15, n) * z
    y = rng.uniform(-0.65, 0.65, n) * z
    z[rng.random(n) < 0.05] *= -1
    return np.stack([x, y, z], 1).astype(np.float32)


def run_case(n, rate):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    import calibrating_amd as ca
    from calibrating_amd import sparse
    from calibrating_amd.resize import resize

    cam = ca.Cam(np.array(K), xy=(W, H))
    cloud = torch.from_numpy(sweep(n)).cuda()
    grid = (int(round(H * rate)), int(round(W * rate)))
    depth, info = ca.xyzs_to_dense_depth(cloud, cam, rate=rate, return_info=True)
    kept = info["rows"]
    reps = 20 if n <= 10 ** 6 else 5
    case = dict(points=n, rate=rate, grid_hw=list(grid), rows=kept, hull_counts=info["hull_counts"])

    # stages, on rows made once
    from calibrating_amd import _native
    from calibrating_amd._arrays import K9
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(8, _native.lib().camd_cloud_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    rows = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    K9_ = K9(cam.K)

    def stage_rows():
        _native.call("camd_cloud_to_uvzs", cloud.device, cloud.data_ptr(), _native.VALUE_F32, n, 3, None, K9_.ctypes.data, W, H, rate, 3,
                     rows.data_ptr(), n, counters.data_ptr(), ws.data_ptr())

    stage_rows()
    r = rows[:kept]
    filled, _ = sparse._nearest_in_hull(r, kept, grid, 2.0, "float64", rows_range=(0, grid[0] + 1))
    uvz = r.contiguous()
    case["rows_ms"] = gpu_ms(stage_rows, 2, reps)
    case["hull_record_ms"] = gpu_ms(lambda: sparse._cloud_hull_record(r, 3, kept, (0, grid[0] + 1)), 2, reps)
    case["hull_and_fill_ms"] = gpu_ms(lambda: sparse._nearest_in_hull(r, kept, grid, 2.0, "float64", rows_range=(0, grid[0] + 1)), 2, reps)
    case["resize_ms"] = gpu_ms(lambda: resize(filled, (H, W)), 2, reps) if grid != (H, W) else [0.0, 0.0]
    case["call_ms"] = gpu_ms(lambda: ca.xyzs_to_dense_depth(cloud, cam, rate=rate), 2, reps)
    case["call_sparse_ms"] = gpu_ms(lambda: ca.xyzs_to_dense_depth(cloud, cam, rate=rate, sparse=True), 2, reps)
    case["interpolate_uvzs_nearest_ms"] = gpu_ms(lambda: sparse.interpolate_uvzs(uvz, grid, None, "nearest", 2), 2, reps)
    # the reference's route on the CPU: KDTree over the rows, one query per pixel
    try:
        from scipy.spatial import KDTree
        host = uvz.cpu().numpy()
        t0 = time.perf_counter()
        ys, xs = np.mgrid[:grid[0], :grid[1]]
        d, i = KDTree(host[:, :2]).query(np.stack([xs.ravel(), ys.ravel()], 1), workers=1)
        np.where(d < 2, host[i, 2], 0).astype(np.float32)
        case["scipy_kdtree_cpu_ms"] = (time.perf_counter() - t0) * 1e3
    except ImportError:
        case["scipy_kdtree_cpu_ms"] = None
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", default="100000,1000000,10000000")
    ap.add_argument("--rates", default="0.5,1")
    ap.add_argument("--case", default=None, help="n,rate: run this one case in this process and print its JSON")
    args = ap.parse_args()
    if args.case:
        n, rate = args.case.split(",")
        print(json.dumps(run_case(int(n), float(rate))))
        return 0
    result = dict(wh=[W, H], distance=2, cases=[])
    for n in [int(v) for v in args.points.split(",")]:
        for rate in [float(v) for v in args.rates.split(",")]:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", "%d,%r" % (n, rate)], stdout=subprocess.PIPE,
                                   timeout=CASE_SECONDS)
            except subprocess.TimeoutExpired:
                result["stopped"] = "case %d, %r ran into its %d s limit" % (n, rate, CASE_SECONDS)
                break
            if p.returncode != 0:
                result["stopped"] = "case %d, %r ended with status %d" % (n, rate, p.returncode)
                break
            result["cases"].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        if "stopped" in result:
            break
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 1 if "stopped" in result else 0


if __name__ == "__main__":
    sys.exit(main())
