#!/usr/bin/env python3
"""Times the one-pass detector of several ChArUco boards (csrc/charuco.hip, k_charuco_multi) on the GPU -- HIP events after
warm-up, gray frames resident in HBM -- and writes one JSON record:
    python tools/gpu_multiboard_time.py [--out profiles/multiboard_time.json]
Five boards of 5 x 4 squares (4 x 4 bits, 2/3 of a square) cut from one dictionary, side by side at 1920 x 1080 with sigma =
4 grey levels of noise; 1, 100 and 1 000 frames.  ``find_charuco_boards`` (one pass) against five ``find_charuco_corners``
calls (one per board) on the same frames in the same run, with the stages both share (``chess_response``, ``chess_peaks``),
and how many of the five boards each way finds: the single-board detector scans the 32 seeds nearest the centroid of all
peaks and does not reach the outer boards.  The worst case beside it: a texture frame at the 1 024-peak capacity with a
set of 8 boards, where the scan limits (32 B seeds, 4 B lattices) are the only bound on a wave's time.  The event time is
that of the Python binding: the allocations and the launches.  Every frame is a copy of one image: a best case for the
caches, and every wave of the new stage does the same work."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES = (1, 100, 1000)
W, H = 1920, 1080
BOARDS = 5


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
    import multiboard_cases as mc
    import subpix_cases as sc

    dictionary = boards.make_marker_dictionary(BOARDS * 11 + 1, mc.BITS, 1)
    first_ids = [1 + 11 * k for k in range(BOARDS)]
    frame = mc.Setup(0, (H, W), dictionary)
    frame.K = np.array([[1400.0, 0, (W - 1) / 2], [0, 1400.0, (H - 1) / 2], [0, 0, 1]])
    old_ss, cc.SS = cc.SS, 2
    parts = []
    for k, first in enumerate(first_ids):  # squares of about 70 px, 370 px from board to board
        R, t = sc.rodrigues((0.1 * (k - 2), 0.08 * (2 - k), 0.03 * k)), np.array([0.16 * (k - 2), 0.02 * (k % 2) - 0.01, 0.6])
        parts.append((first, cc.homography_of_pose(frame, R, t), {}))
    clean = mc.compose(parts, (H, W), dictionary=dictionary)
    cc.SS = old_ss
    img = np.clip(np.rint(clean.astype(np.float64) + np.random.default_rng(0).normal(0, 4, (H, W))), 0, 255).astype(np.uint8)

    one_pass = lambda x: imgproc.find_charuco_boards(x, mc.SQUARES, dictionary, first_ids, mc.RATIO, return_info=True)  # noqa: E731
    per_board = lambda x: [imgproc.find_charuco_corners(x, mc.SQUARES, dictionary, mc.RATIO, f, return_info=True) for f in first_ids]  # noqa: E731
    got = one_pass(img)
    rec = dict(boards=BOARDS, squares=list(mc.SQUARES), bits=mc.BITS, marker_ratio=list(mc.RATIO), size=[W, H], noise_sigma=4,
               candidates=int(got[4]), boards_found_one_pass=int((got[3] == 0).sum()),
               boards_found_five_calls=int(sum(bool(r[0]) for r in per_board(img))),
               device=torch.cuda.get_device_name(0), runs=[])
    g1 = torch.from_numpy(img).cuda()
    for f in FRAMES:
        gray = g1[None].repeat(f, 1, 1)
        resp, top = imgproc.chess_response(gray)
        rlo, rhi = gpu_ms(lambda: imgproc.chess_response(gray))
        plo, phi = gpu_ms(lambda: imgproc.chess_peaks(resp, top))
        mlo, mhi = gpu_ms(lambda: one_pass(gray))
        slo, shi = gpu_ms(lambda: per_board(gray))
        rec["runs"].append(dict(frames=f, response_ms=[rlo, rhi], peaks_ms=[plo, phi], one_pass_ms=[mlo, mhi],
                                one_pass_new_stage_and_rest_ms=mlo - rlo - plo, five_calls_ms=[slo, shi],
                                one_pass_over_five_calls=mlo / slo, one_pass_us_per_frame=1e3 * mlo / f))
        del gray, resp, top
    # the worst case: as many peaks as a frame keeps, none of them a board's, a set of 8
    rng = np.random.default_rng(11)
    cells = rng.integers(0, 2, (H // 17 + 1, W // 17 + 1))  # (one corner in eight of random cells is an X-junction: about 900)
    texture = np.where(np.kron(cells, np.ones((17, 17), int))[:H, :W] == 1, sc.BRIGHT, sc.DARK).astype(np.uint8)
    big = boards.make_marker_dictionary(8 * 10, mc.BITS, 1, 3)
    eight = [10 * k for k in range(8)]
    worst = lambda x, **kw: imgproc.find_charuco_boards(x, mc.SQUARES, big, eight, mc.RATIO, return_info=True, **kw)  # noqa: E731
    relative = 1
    for relative in range(1, 65):  # the first threshold at which the texture leaves more than the capacity, and the one before
        if int(worst(texture, relative=relative)[4]) > imgproc.CHESS_CAPACITY:
            break
    relative = max(1, relative - 1)
    w = worst(texture, relative=relative)
    t100 = torch.from_numpy(texture).cuda()[None].repeat(100, 1, 1)
    wlo, whi = gpu_ms(lambda: worst(t100, relative=relative))
    r100, top100 = imgproc.chess_response(t100)
    rlo, _ = gpu_ms(lambda: imgproc.chess_response(t100))
    plo, _ = gpu_ms(lambda: imgproc.chess_peaks(r100, top100, relative))
    rec["worst_case"] = dict(boards=8, relative=relative, candidates=int(w[4]), status=sorted(set(np.asarray(w[3]).tolist())), frames=100,
                             whole_ms=[wlo, whi], new_stage_and_rest_ms=wlo - rlo - plo)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
