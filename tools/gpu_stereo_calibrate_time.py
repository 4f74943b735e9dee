#!/usr/bin/env python3
"""Times ``stereo_calibrate`` (csrc/stereo_calibrate.hip) on the GPU -- wall time around a synchronised call after
warm-up, points resident in HBM, the median of many repetitions -- and prints one JSON line:
    python tools/gpu_stereo_calibrate_time.py [--out profiles/stereo_calibrate_time.json]
30, 1 000 and 10 000 frames of a 70-point board seen by two cameras (5 coefficients each, 0.3 px noise), float64.  With
every size: the number of evaluations and of host read-backs (one of 16 bytes per evaluation; besides them the two status
arrays, the start poses for the median and the final state, once each).  For information, ``calibrate_camera`` on camera
1's rows at the same frame counts.  In the same run, on this machine's CPU at 30 frames: the NumPy restatement
tests/stereo_calibrate_ref.py and, where SciPy is present, ``scipy.optimize.least_squares`` (sparse Jacobian, trust-region
reflective) from the same start.  Wall time, not event time: a call synchronises once per evaluation, so the host's share
is part of what a caller waits for."""
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


def scipy_stereo(ref, objs, uv1s, uv2s, cams):
    """least_squares over the same residual from the same start: 6 + 6 f unknowns, the arrow-shaped sparsity given"""
    from scipy import optimize, sparse
    from pnp_ref import rotate_left
    _, T1s, T2s = ref.start(objs, uv1s, uv2s, cams)
    R0, t0 = ref.rig_start(T1s, T2s)
    f = len(objs)

    def fun(x):
        R, t = rotate_left(x[:3], R0), t0 + x[3:6]
        return np.concatenate([ref.residuals(rotate_left(x[6 + 6 * i:9 + 6 * i], T[:3, :3]), T[:3, 3] + x[9 + 6 * i:12 + 6 * i], R, t, o, a, b, cams)
                               for i, (T, o, a, b) in enumerate(zip(T1s, objs, uv1s, uv2s))])
    rows = sum(4 * len(o) for o in objs)
    S = sparse.lil_matrix((rows, 6 + 6 * f), dtype=np.int8)
    S[:, :6] = 1
    at = 0
    for i, o in enumerate(objs):
        S[at:at + 4 * len(o), 6 + 6 * i:12 + 6 * i] = 1
        at += 4 * len(o)
    r = optimize.least_squares(fun, np.zeros(6 + 6 * f), jac_sparsity=S.tocsr(), x_scale="jac", method="trf", max_nfev=50)
    return rotate_left(r.x[:3], R0), t0 + r.x[3:6], r.nfev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu-frames", type=int, default=30, help="largest size the CPU solvers are run at")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    import calibrating_amd as ca
    import pnp_cases as pc
    import stereo_calibrate_cases as sc
    import stereo_calibrate_ref as ref

    cams = sc.cameras((5, 5), 1)
    K1, D1, K2, D2 = cams
    R, t = sc.true_rig(1)
    T12 = np.eye(4)
    T12[:3, :3], T12[:3, 3] = R, t
    board = pc.centred(pc.board_points(POINTS))
    Ts = sc.poses(BASE, board, cams, (R, t), seed=1)
    res = dict(device=torch.cuda.get_device_name(0), points=POINTS, sigma_px=sc.NOISE_SIGMA,
               note="wall time per stereo_calibrate call, points resident, the median of the repetitions: the host's planarity "
                    "test, camd_pnp_init + camd_pnp_refine per camera, the read-back of the status words and start poses, the "
                    "median on the host, then per evaluation camd_stereo_step (four launches), one 16-byte read-back and, after "
                    "an accepted step, camd_stereo_linearise; the CPU figures are single-threaded NumPy / SciPy on this machine")
    rows = []
    tobj = torch.from_numpy(board).cuda()
    for frames in FRAMES:
        uv1 = np.stack([pc.observe(board, Ts[i % BASE], K1, D1, sc.NOISE_SIGMA, seed=2 * i) for i in range(frames)])
        uv2 = np.stack([pc.observe(board, T12 @ Ts[i % BASE], K2, D2, sc.NOISE_SIGMA, seed=2 * i + 1) for i in range(frames)])
        t1, t2 = torch.from_numpy(uv1).cuda(), torch.from_numpy(uv2).cuda()
        fn = lambda: ca.stereo_calibrate(tobj, t1, t2, K1, D1, K2, D2)  # noqa: E731
        reps = 15 if frames <= 1000 else 7
        med, lo, hi = wall_ms(fn, warmup=2, reps=reps)
        r = fn()
        row = dict(frames=frames, ms_median=med, ms_min=lo, ms_max=hi, evaluations=r["evaluations"], iterations=r["iterations"],
                   readbacks_in_loop=r["evaluations"], readbacks_outside_loop=5, retval=r["retval"],
                   all_frames_used=bool((r["status"] == 0).all().item()),
                   max_abs_R_minus_truth=float(np.abs(r["R"] - R).max()), max_abs_t_minus_truth=float(np.abs(r["t"].ravel() - t).max()))
        cal = lambda: ca.calibrate_camera(tobj, t1, (sc.W, sc.H))  # noqa: E731
        cmed, clo, chi = wall_ms(cal, warmup=1, reps=5 if frames <= 1000 else 3)
        row.update(calibrate_camera_ms_median=cmed, calibrate_camera_evaluations=cal()["evaluations"])
        if frames <= args.cpu_frames:
            objs, u1, u2 = [board] * frames, list(uv1), list(uv2)
            t0 = time.perf_counter()
            w = ref.stereo_calibrate(objs, u1, u2, K1, D1, K2, D2)
            row.update(cpu_restatement_s=time.perf_counter() - t0, cpu_restatement_evaluations=w["evaluations"],
                       max_abs_R_minus_restatement=float(np.abs(r["R"] - w["R"]).max()),
                       max_abs_t_minus_restatement=float(np.abs(r["t"] - w["t"]).max()))
            try:
                t0 = time.perf_counter()
                Rs, ts, nfev = scipy_stereo(ref, objs, u1, u2, cams)
                row.update(cpu_scipy_s=time.perf_counter() - t0, cpu_scipy_nfev=int(nfev),
                           max_abs_R_minus_scipy=float(np.abs(r["R"] - Rs).max()), max_abs_t_minus_scipy=float(np.abs(r["t"].ravel() - ts).max()))
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
