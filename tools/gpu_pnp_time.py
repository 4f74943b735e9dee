#!/usr/bin/env python3
"""Times ``pnp.solve_pnp_batch`` (csrc/pnp.hip) on the GPU -- HIP events after warm-up, points resident in HBM -- and
prints one JSON line:
    python tools/gpu_pnp_time.py [--out profiles/pnp_time.json]
1, 1 000 and 10 000 frames of a 70-point board (5 coefficients, 0.3 px noise), float64, without a start pose (both
kernels) and with one (the refinement alone).  In the same run, on this machine's CPU: the NumPy restatement
tests/pnp_ref.py per frame and, where SciPy is present, ``scipy.optimize.least_squares`` per frame from the same start.
The event time is that of the Python binding: the host's planarity SVD of the object points, the allocations, the
launches."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES = (1, 1000, 10000)
POINTS = 70


def gpu_ms(fn, warmup=3, reps=20):
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
    from calibrating_amd import pnp
    import pnp_cases as pc
    import pnp_ref as ref

    base = pc.case("board", POINTS, 8, 5, sigma=pc.NOISE_SIGMA, seed=1)
    K, D, obj = base["K"], base["D"], base["obj"]
    planar, plane = ref.plane_of(obj)
    t0 = time.perf_counter()
    starts = np.stack([ref.init_pose(obj, uv, K, D, planar, plane) for uv in base["uv"]])
    wants = [ref.refine(obj, uv, K, D, s) for uv, s in zip(base["uv"], starts)]
    cpu_restatement_s = (time.perf_counter() - t0) / len(starts)
    cpu_scipy_s = None
    try:
        from scipy import optimize
        t0 = time.perf_counter()
        for uv, s in zip(base["uv"], starts):
            fun = lambda d: ref.residuals(ref.rotate_left(d[:3], s[:3, :3]), s[:3, 3] + d[3:], obj, uv, K, D).reshape(-1)  # noqa: E731
            optimize.least_squares(fun, np.zeros(6), method="lm")
        cpu_scipy_s = (time.perf_counter() - t0) / len(starts)
    except ImportError:
        pass
    res = dict(device=torch.cuda.get_device_name(0), points=POINTS, ndist=5, sigma_px=pc.NOISE_SIGMA,
               cpu_restatement_s_per_frame=cpu_restatement_s, cpu_scipy_s_per_frame=cpu_scipy_s,
               note="event time per call of the Python binding, points resident: the host's planarity test, allocations, one "
                    "launch of camd_pnp_init (unless a start pose is given) and one of camd_pnp_refine; the CPU figures are "
                    "single-threaded NumPy / SciPy on this machine, one frame per call")
    rows = []
    tobj = torch.from_numpy(obj).cuda()
    for frames in FRAMES:
        pick = np.arange(frames) % len(base["uv"])
        tuv = torch.from_numpy(base["uv"][pick]).cuda()
        T0 = starts[pick]
        for name, fn in (("init + refine", lambda: pnp.solve_pnp_batch(tobj, tuv, K, D)),
                         ("refine from T0", lambda: pnp.solve_pnp_batch(tobj, tuv, K, D, T0=T0))):
            lo, hi = gpu_ms(fn)
            r = fn()
            rows.append(dict(call=name, frames=frames, ms_min=lo, ms_max=hi, us_per_frame=lo * 1e3 / frames,
                             all_ok=bool((r["status"] == 0).all().item()), max_iterations=int(r["iterations"].max().item()),
                             max_abs_T_minus_restatement=float(max(np.abs(r["T"][i].cpu().numpy() - wants[pick[i]]["T"]).max()
                                                                   for i in range(min(frames, 8))))))
    res["rows"] = rows
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
