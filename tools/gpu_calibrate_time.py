#!/usr/bin/env python3
"""Times ``calibrate.calibrate_camera`` (csrc/calibrate.hip) on the GPU -- wall time around a synchronised call after
warm-up, points resident in HBM, the median of many repetitions -- and prints one JSON line:
    python tools/gpu_calibrate_time.py [--out profiles/calibrate_time.json]
30, 1 000 and 10 000 frames of a 70-point board (5 coefficients, 0.3 px noise), float64.  With every size: the number of
evaluations and of host read-backs (one of 16 bytes per evaluation; besides them the homographies, the frames' status
words and the final state, once each).  In the same run, on this machine's CPU: the NumPy restatement
tests/calibrate_ref.py and, where SciPy is present, ``scipy.optimize.least_squares`` (sparse Jacobian, trust-region
reflective) from the same start, at the sizes up to ``--cpu-frames`` (30: SciPy needs minutes at 1 000 frames).  Wall time, not event time: a call
synchronises once per evaluation, so the host's share is part of what a caller waits for."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES = (30, 1000, 10000)
POINTS = 70
BASE = 30  # distinct frames; the larger batches repeat them with fresh noise


def wall_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def scipy_calibrate(ref, objs, uvs, xy):
    """least_squares over the same residual from the same start: 9 + 6 f unknowns, the arrow-shaped sparsity given"""
    from scipy import optimize, sparse
    k0, status, poses0, _ = ref.start(objs, uvs, xy)
    f = len(objs)

    def unpack(x):
        return x[:9], [(ref.pnp_ref.rotate_left(x[9 + 6 * i:12 + 6 * i], R), t + x[12 + 6 * i:15 + 6 * i]) for i, (R, t) in enumerate(poses0)]

    def fun(x):
        k, poses = unpack(x)
        K, D = ref.camera_of(k)
        return np.concatenate([(ref.points_ref.project_points(o, R, t, K, D) - u).reshape(-1) for (R, t), o, u in zip(poses, objs, uvs)])
    rows = sum(2 * len(o) for o in objs)
    S = sparse.lil_matrix((rows, 9 + 6 * f), dtype=np.int8)
    S[:, :9] = 1
    at = 0
    for i, o in enumerate(objs):
        S[at:at + 2 * len(o), 9 + 6 * i:15 + 6 * i] = 1
        at += 2 * len(o)
    r = optimize.least_squares(fun, np.concatenate([k0, np.zeros(6 * f)]), jac_sparsity=S.tocsr(), x_scale="jac", method="trf",
                                max_nfev=50)  # SciPy's default tolerances (1e-8): at 1e-12 it does not end within minutes
    return r.x[:9], r.nfev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu-frames", type=int, default=30, help="largest size the CPU solvers are run at (SciPy needs minutes at 1 000 frames)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    from calibrating_amd import calibrate
    import calibrate_cases as cc
    import calibrate_ref as ref
    import pnp_cases as pc

    K, D = cc.true_camera("lens", 1)
    board = pc.centred(pc.board_points(POINTS))
    Ts = cc.poses(BASE, seed=1)
    xy = (cc.W, cc.H)
    res = dict(device=torch.cuda.get_device_name(0), points=POINTS, sigma_px=cc.NOISE_SIGMA,
               note="wall time per calibrate_camera call, points resident, the median of the repetitions: the host's planarity "
                    "test, the homographies and their read-back, camd_pnp_init + camd_pnp_refine, then per evaluation "
                    "camd_calib_step (three launches), one 16-byte read-back and, after an accepted step, "
                    "camd_calib_linearise; the CPU figures are single-threaded NumPy / SciPy on this machine")
    rows = []
    tobj = torch.from_numpy(board).cuda()
    for frames in FRAMES:
        uv = np.stack([pc.observe(board, Ts[i % BASE], K, D, cc.NOISE_SIGMA, seed=i) for i in range(frames)])
        tuv = torch.from_numpy(uv).cuda()
        fn = lambda: calibrate.calibrate_camera(tobj, tuv, xy)  # noqa: E731
        med, lo, hi = wall_ms(fn, warmup=2, reps=15 if frames <= 1000 else 7)
        r = fn()
        row = dict(frames=frames, ms_median=med, ms_min=lo, ms_max=hi, evaluations=r["evaluations"], iterations=r["iterations"],
                   readbacks_in_loop=r["evaluations"], readbacks_outside_loop=3, retval=r["retval"],
                   all_frames_used=bool((r["status"] == 0).all().item()))
        if frames <= args.cpu_frames:
            objs, uvs = [board] * frames, list(uv)
            t0 = time.perf_counter()
            w = ref.calibrate(objs, uvs, xy)
            row.update(cpu_restatement_s=time.perf_counter() - t0, cpu_restatement_evaluations=w["evaluations"],
                       max_abs_K_minus_restatement=float(np.abs(r["K"] - w["K"]).max()))
            try:
                t0 = time.perf_counter()
                k, nfev = scipy_calibrate(ref, objs, uvs, xy)
                row.update(cpu_scipy_s=time.perf_counter() - t0, cpu_scipy_nfev=int(nfev),
                           max_abs_K_minus_scipy=float(np.abs(r["K"] - ref.camera_of(k)[0]).max()))
            except ImportError:
                row.update(cpu_scipy_s=None)
        rows.append(row)
        res["rows"] = rows
        line = json.dumps(res)
        if args.out:  # after every size: a run that is cut short leaves what it has measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
