#!/usr/bin/env python3
"""Times the three stages of the thin-plate spline fill (csrc/spline.hip) separately -- HIP events after warm-up, everything
resident in HBM -- and prints one JSON line:
    python tools/gpu_spline_time.py [--out profiles/spline_time.json] [--points 88,512,1024] [--batches 1,64] [--no-scipy]
n = 88 (a board), 512 and 1024 (the cap) samples per frame; the 1080p // 8 grid (135 x 240) and 1920 x 1080; 1 and 64 frames.
Assembly and solve depend on (n, frames) only, the evaluation on the grid as well.  Beside the evaluation: the phi
evaluations (one float64 sqrt and one float64 log each) per second it reaches, what the part's float64 vector peak leaves per
evaluation at that rate, and its 8 B per pixel written against the copy ceiling -- the stage is expected to be bound by the
float64 log, not by bytes.  In the same run ``scipy.interpolate.Rbf`` (the reference's call) on the box's CPU where it fits:
every n on the coarse grid, n = 88 at 1080p in strips of rows (SciPy forms an n x pixels matrix)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_CEILING_GBS = 6290.0  # measured copy ceiling of the part
FP64_VECTOR_TFLOPS = 78.6  # the part's float64 vector peak (AMD's MI355X data sheet)
FRAME = (1080, 1920)
GRIDS = {"1080p//8": ((135, 240), 8), "1080p": ((1080, 1920), 1)}


def gpu_ms(fn, budget_ms=300.0, max_reps=50):
    """(min, max) ms per call over three windows (the spread says how much the number can be trusted), each of as many
    calls as fit ``budget_ms`` by a first timed call, after one warm-up call"""
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    reps = int(max(1, min(max_reps, budget_ms / max(a.elapsed_time(b), 1e-3))))
    times = []
    for _ in range(3):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return [min(times), max(times)], reps


def scipy_s(uvz, hw, step, strip):
    import numpy as np
    from scipy.interpolate import Rbf
    t = time.perf_counter()
    rbf = Rbf(uvz[:, 0], uvz[:, 1], uvz[:, 2], function="thin_plate", smooth=0.5)
    t_fit = time.perf_counter() - t
    xs = np.arange(hw[1], dtype=np.float64) * step
    t = time.perf_counter()
    for y0 in range(0, hw[0], strip):
        ys = np.arange(y0, min(hw[0], y0 + strip), dtype=np.float64) * step
        rbf(*np.meshgrid(xs, ys))
    return t_fit, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", default="88,512,1024")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    from calibrating_amd import _native, sparse
    import spline_ref as ref

    dev = torch.device("cuda", 0)
    result = dict(frame=list(FRAME), copy_ceiling_GBs=COPY_CEILING_GBS, fp64_vector_TFLOPs=FP64_VECTOR_TFLOPS, cases=[], scipy=[])
    for n in [int(v) for v in args.points.split(",")]:
        for frames in [int(v) for v in args.batches.split(",")]:
            uvz = np.concatenate([ref.samples(1000 * n + f, n, FRAME) for f in range(frames)])
            rows = torch.from_numpy(uvz).to(dev)
            lengths = np.full(frames, n, np.int64)
            start = sparse._spline_start(lengths, dev)
            A = torch.empty((frames, n, n), dtype=torch.float64, device=dev)
            weights = torch.zeros((frames, n), dtype=torch.float64, device=dev)
            status = torch.empty(frames, dtype=torch.int32, device=dev)

            def assemble():
                _native.call("camd_spline_assemble", dev, rows.data_ptr(), 3, n * frames, start.data_ptr(), frames, n, 0.5, A.data_ptr())

            def solve():  # (factors A in place: every call is given a fresh matrix, whose assembly is timed beside it)
                assemble()
                _native.call("camd_spline_solve", dev, rows.data_ptr() + 16, 3, n * frames, start.data_ptr(), frames, n, A.data_ptr(),
                             weights.data_ptr(), status.data_ptr())

            case = dict(points=n, frames=frames)
            case["assemble_ms"], _ = gpu_ms(assemble)
            both, _ = gpu_ms(solve)
            case["assemble_and_solve_ms"] = both
            case["solve_ms"] = [both[0] - case["assemble_ms"][0], both[1] - case["assemble_ms"][0]]
            assert int(status.abs().max().item()) == 0, status
            for name, (hw, step) in GRIDS.items():
                out = torch.empty((frames,) + hw, dtype=torch.float64, device=dev)

                def evaluate():
                    _native.call("camd_spline_eval", dev, rows.data_ptr(), 3, n * frames, start.data_ptr(), frames, n, weights.data_ptr(),
                                 None, hw[1], hw[0], step, out.data_ptr())

                ms, reps = gpu_ms(evaluate)
                phis = frames * hw[0] * hw[1] * n
                written = frames * hw[0] * hw[1] * 8
                case["eval_" + name] = dict(ms=ms, reps=reps, phi_evaluations=phis, phi_per_s=phis / (ms[0] * 1e-3),
                                            fp64_flops_per_phi_at_peak=FP64_VECTOR_TFLOPS * 1e12 / (phis / (ms[0] * 1e-3)),
                                            bytes_written=written, write_floor_ms=written / (COPY_CEILING_GBS * 1e9) * 1e3,
                                            share_of_write_floor=written / (COPY_CEILING_GBS * 1e9) * 1e3 / ms[0])
                del out
            case["share_of_solve_in_one_1080p_fill"] = case["solve_ms"][0] / (case["assemble_and_solve_ms"][0] + case["eval_1080p"]["ms"][0])
            result["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
            del A, weights, rows
            torch.cuda.empty_cache()
        if not args.no_scipy:
            one = ref.samples(1000 * n, n, FRAME)
            for name, (hw, step) in GRIDS.items():
                if name == "1080p" and n > 88:
                    result["scipy"].append(dict(points=n, grid=name, measured=False, why="an n x pixels float64 matrix per strip: minutes"))
                    continue
                fit_s, eval_s = scipy_s(one, hw, step, 8 if name == "1080p" else hw[0])
                result["scipy"].append(dict(points=n, grid=name, measured=True, fit_s=fit_s, eval_s=eval_s, cpus=os.cpu_count()))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
