#!/usr/bin/env python3
"""Times the ChArUco detector (csrc/charuco.hip) on the GPU -- HIP events after warm-up, gray frames resident in HBM --
and writes one JSON record:
    python tools/gpu_charuco_time.py [--out profiles/charuco_time.json]
A 9 x 5 board (32 inner corners, 22 markers of 4 x 4 bits, half a square wide) at 1920 x 1080 with sigma = 4 grey levels of
noise; 1, 100 and 1 000 frames; the stages it shares with the chessboard detector (``chess_response``, ``chess_peaks``),
the new stages as the rest of ``find_charuco_corners``, and the whole call.  Beside it in the same run:
``find_chessboard_corners`` on a plain 8 x 4-corner board of the same pose, and on this machine's CPU the NumPy restatement
tests/charuco_ref.py per frame.  The event time is that of the Python binding: the allocations and the launches.  Every
frame is a copy of one image: a best case for the caches, and every wave of the new stages does the same work."""
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
W, H = 1920, 1080


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
    from calibrating_amd import boards, imgproc
    import charuco_cases as cc
    import charuco_ref as ref
    import chessboard_ref as cref
    import subpix_cases as sc

    setup = cc.Setup((9, 5), 4, (1, 2), (H, W), 0.5, seed=0)
    setup.K = np.array([[1400.0, 0, 959.5], [0, 1400.0, 539.5], [0, 0, 1]])
    Hm = cc.homography_of_pose(setup, sc.rodrigues((0.2, -0.25, 0.05)), np.array([0.01, -0.005, 0.5]))
    noise = np.random.default_rng(0).normal(0, 4, (H, W))
    old_ss, cc.SS = cc.SS, 2
    img = np.clip(np.rint(cc.render(setup, Hm).astype(np.float64) + noise), 0, 255).astype(np.uint8)
    plain = np.clip(np.rint(cc.render(setup, Hm, markers=False).astype(np.float64) + noise), 0, 255).astype(np.uint8)
    cc.SS = old_ss
    truth = cc.truth(setup, Hm)

    t0 = time.perf_counter()
    r, rmax = cref.response(img[None])
    t1 = time.perf_counter()
    cand, counts = cref.peaks(r, rmax)
    t2 = time.perf_counter()
    corners, marker_ids, status = ref.detect_one(cand[0, :counts[0]], img, setup.squares, ref.words(setup.dictionary), setup.bits,
                                                 setup.ratio, setup.first_id)
    t3 = time.perf_counter()
    call = lambda x: imgproc.find_charuco_corners(x, setup.squares, setup.dictionary, setup.ratio, setup.first_id, return_info=True)  # noqa: E731
    got = call(img)
    assert got[0] and status == 0 and np.array_equal(got[1], corners, equal_nan=True) and np.array_equal(got[2], marker_ids), \
        "the kernel and the restatement disagree"
    seen = ~np.isnan(corners[:, 0])

    rec = dict(board=list(setup.squares), bits=setup.bits, marker_ratio=list(setup.ratio), size=[W, H], noise_sigma=4,
               candidates=int(counts[0]), corners_seen=int(seen.sum()), markers_decoded=int((marker_ids >= 0).sum()),
               offset_px_max=float(np.abs(corners[seen] - truth[seen]).max()),
               cpu_numpy_restatement_ms_per_frame=dict(response=1e3 * (t1 - t0), peaks=1e3 * (t2 - t1), new_stages=1e3 * (t3 - t2),
                                                       whole=1e3 * (t3 - t0)),
               device=torch.cuda.get_device_name(0), runs=[])
    g1, p1 = torch.from_numpy(img).cuda(), torch.from_numpy(plain).cuda()
    for f in FRAMES:
        gray, chess = g1[None].repeat(f, 1, 1), p1[None].repeat(f, 1, 1)
        resp, top = imgproc.chess_response(gray)
        rlo, rhi = gpu_ms(lambda: imgproc.chess_response(gray))
        plo, phi = gpu_ms(lambda: imgproc.chess_peaks(resp, top))
        wlo, whi = gpu_ms(lambda: call(gray))
        clo, chi = gpu_ms(lambda: imgproc.find_chessboard_corners(chess, (8, 4)))
        assert bool(call(gray)[0].all()) and bool(imgproc.find_chessboard_corners(chess, (8, 4))[0].all())
        rec["runs"].append(dict(frames=f, response_ms=[rlo, rhi], peaks_ms=[plo, phi], whole_ms=[wlo, whi],
                                new_stages_and_rest_ms=wlo - rlo - plo, whole_us_per_frame=1e3 * wlo / f,
                                chessboard_whole_ms=[clo, chi]))
        del gray, chess, resp, top
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
