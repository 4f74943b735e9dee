#!/usr/bin/env python3
"""Times the chessboard detector (csrc/chessboard.hip) on the GPU -- HIP events after warm-up, gray frames resident in HBM
-- and writes one JSON record:
    python tools/gpu_chessboard_time.py [--out profiles/chessboard_time.json]
An 11 x 8 board (88 corners) at 1920 x 1080 with sigma = 4 grey levels of noise; 1, 100 and 1 000 frames; each stage
(``chess_response``, ``chess_peaks``, the lattice as the rest of ``find_chessboard_corners``) and the whole call.  The
response kernel moves 3 B per pixel (1 read, 2 written) and is set against the 6.29 TB/s a copy reaches on this chip.  In
the same run, on this machine's CPU: the NumPy restatement tests/chessboard_ref.py per frame, stage by stage.  The event
time is that of the Python binding: the allocations and the launches.  Every frame is a copy of one image: a best case for
the caches, and every wave of the lattice does the same work."""
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
COPY_CEILING_TBPS = 6.29


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
    import chessboard_ref as ref
    import subpix_cases as sc

    K = np.array([[1400.0, 0, 959.5], [0, 1400.0, 539.5], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = sc.rodrigues((0.2, -0.25, 0.05)), (0.01, -0.005, 0.5)
    Hm = K @ np.stack([T[:3, 0], T[:3, 1], T[:3, 3]], 1)
    xy = np.mgrid[:COLS, :ROWS].T.reshape(-1, 2) * sc.SQUARE
    p = np.concatenate([xy - xy.mean(0), np.ones((len(xy), 1))], 1) @ Hm.T
    truth = p[:, :2] / p[:, 2:]
    img = sc.render(Hm, H, W, COLS, ROWS, ss=2).astype(np.float64) + np.random.default_rng(0).normal(0, 4, (H, W))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)

    t0 = time.perf_counter()
    r, rmax = ref.response(img[None])
    t1 = time.perf_counter()
    cand, counts = ref.peaks(r, rmax)
    t2 = time.perf_counter()
    corners, status = ref.lattice(cand, counts, W, (COLS, ROWS))
    t3 = time.perf_counter()
    got = imgproc.find_chessboard_corners(img, (COLS, ROWS), return_info=True)
    assert got[0] and status[0] == 0 and np.array_equal(got[1], corners[0]) and got[3] == counts[0], \
        "the kernels and the restatement disagree"
    same_board = min(np.abs(corners[0] - truth).max(), np.abs(corners[0] - truth[::-1]).max())

    rec = dict(board=[COLS, ROWS], size=[W, H], noise_sigma=4, candidates=int(counts[0]), response_max=int(rmax[0]),
               offset_px_max=float(same_board), copy_ceiling_TBps=COPY_CEILING_TBPS,
               cpu_numpy_restatement_ms_per_frame=dict(response=1e3 * (t1 - t0), peaks=1e3 * (t2 - t1), lattice=1e3 * (t3 - t2),
                                                       whole=1e3 * (t3 - t0)),
               device=torch.cuda.get_device_name(0), runs=[])
    g1 = torch.from_numpy(img).cuda()
    for f in FRAMES:
        gray = g1[None].repeat(f, 1, 1)
        resp, top = imgproc.chess_response(gray)
        rlo, rhi = gpu_ms(lambda: imgproc.chess_response(gray))
        plo, phi = gpu_ms(lambda: imgproc.chess_peaks(resp, top))
        wlo, whi = gpu_ms(lambda: imgproc.find_chessboard_corners(gray, (COLS, ROWS)))
        found = imgproc.find_chessboard_corners(gray, (COLS, ROWS))[0]
        assert bool(found.all())
        tbps = 3.0 * W * H * f / (rlo * 1e-3) / 1e12
        rec["runs"].append(dict(frames=f, response_ms=[rlo, rhi], peaks_ms=[plo, phi], whole_ms=[wlo, whi],
                                lattice_and_rest_ms=wlo - rlo - plo, response_TBps=tbps,
                                response_share_of_copy_ceiling=tbps / COPY_CEILING_TBPS, whole_us_per_frame=1e3 * wlo / f))
        del gray, resp, top
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
