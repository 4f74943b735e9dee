#!/usr/bin/env python3
"""Times the feature matcher (calibrating_amd/features.py, csrc/features.hip) on the GPU and writes
profiles/features_time.json (the README row quotes that file).

    python tools/gpu_features_time.py [--out profiles/features_time.json] [--reps 10]

Per stage and for the whole call, at 1920 x 1080 with 1, 16 and 64 frames resident in HBM: the median over ``reps`` calls
after a warm-up of the same shape (stream events around the launches; a host clock too for the calls that synchronise
themselves).  The search alone at 2 000, 8 000 and 32 400 descriptors per side, and ``match_views`` of 8 views (28 pairs).
Beside them, from the SAME run: the NumPy restatement (tests/features_ref.py) on this box's CPU at a size where it ends in
reasonable time, and a torch composition of the search (xor, a byte popcount table, ``min``).  Two ratios are derived and
the binding one is named: the search kernel's popcounts per second against the VALU rate, and the score kernel's bytes
against the 6.29 TB/s copy ceiling.  No time is asserted anywhere.  Needs a GPU: without one it fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_CEILING = 6.29e12      # bytes per second, the measured copy ceiling of the MI355X
# 256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz: lane operations per second of 32-bit VALU instructions
VALU_LANE_OPS = 256 * 4 * 32 * 2.4e9
PAIR_LANE_OPS = 8 + 8 + 7 + 4  # per descriptor pair and lane: 8 xor, 8 popcount, 7 adds, the compare-and-select of best / second


def timed(call, reps, torch):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        ev.append(a.elapsed_time(b))
    return dict(gpu_events_ms_median=float(np.median(ev)), gpu_events_ms_min=float(min(ev)), wall_ms_median=1e3 * float(np.median(wall)))


def cpu(call):
    t0 = time.perf_counter()
    call()
    return 1e3 * (time.perf_counter() - t0)


def frames_1080p(f, torch):
    """f different 1080p frames on the device: a block texture like the tests' scene, shifted per frame, plus noise"""
    rng = np.random.default_rng(7)
    blocks = rng.integers(0, 256, (1080 // 9 + 8, 1920 // 9 + 8), dtype=np.uint8)
    base = np.kron(blocks, np.ones((9, 9), np.uint8))
    out = np.empty((f, 1080, 1920), np.uint8)
    for k in range(f):
        dy, dx = (5 * k) % 60, (7 * k) % 60
        out[k] = np.clip(base[dy:dy + 1080, dx:dx + 1920].astype(np.int16) + rng.integers(-4, 5, (1080, 1920)), 0, 255)
    return torch.from_numpy(out).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_features_time.py measures on the GPU; none is visible")
    from calibrating_amd import features
    from calibrating_amd._frames import device_frames
    import features_ref as fr
    knobs = features._split_knobs({})
    threshold, cell, seed = knobs[0]
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, frames=[], search=[], notes=[])

    for f in (1, 16, 64):
        imgs = frames_1080p(f, torch)
        fr_ = device_frames(imgs, features._layout(imgs, "images"), "rgb")
        gray, h, w, pitch, stride = fr_.data, fr_.h, fr_.w, fr_.pitch, fr_.stride
        score = features._score(gray, f, h, w, pitch, stride, threshold)
        xy, scores, counts = features._keypoints(score, cell)
        desc, bins = features._describe(gray, f, h, w, pitch, stride, xy, counts, seed)
        row = dict(frames=f, width=w, height=h, capacity=int(xy.shape[1]), keypoints_mean=float(counts.float().mean()))
        row["score"] = timed(lambda: features._score(gray, f, h, w, pitch, stride, threshold), args.reps, torch)
        row["keypoints"] = timed(lambda: features._keypoints(score, cell), args.reps, torch)
        row["describe"] = timed(lambda: features._describe(gray, f, h, w, pitch, stride, xy, counts, seed), args.reps, torch)
        row["detect_and_describe"] = timed(lambda: features.detect_and_describe(imgs), args.reps, torch)
        bytes_moved = 2.0 * f * h * w  # one byte read and one written per pixel
        row["score_bytes"] = bytes_moved
        row["score_share_of_copy_ceiling"] = bytes_moved / (row["score"]["gpu_events_ms_median"] * 1e-3) / COPY_CEILING
        if f == 1:
            row["match_images"] = timed(lambda: features.match_images(imgs[0], imgs[0]), args.reps, torch)
            host = imgs[0, :270, :480].cpu().numpy()
            row["restatement_cpu_ms_480x270"] = cpu(lambda: fr.detect_and_describe(host))
            row["detect_and_describe_480x270"] = timed(lambda: features.detect_and_describe(imgs[0, :270, :480]), args.reps, torch)
        result["frames"].append(row)
        del imgs, gray, score, xy, scores, counts, desc, bins

    table = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int16, device="cuda")
    for n in (2000, 8000, 32400):
        rng = np.random.default_rng(n)
        d1, d2 = (torch.from_numpy(rng.integers(0, 256, (1, n, 32), dtype=np.uint8)).cuda() for _ in range(2))
        c = torch.full((1,), n, dtype=torch.int32, device="cuda")
        pairs = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
        row = dict(descriptors_per_side=n)
        row["search"] = timed(lambda: features._search(d1, c, d2, c, pairs), args.reps, torch)
        best12, dist12, best21, _ = features._search(d1, c, d2, c, pairs)
        row["filter"] = timed(lambda: features._filter(c, 1, n, pairs, best12, dist12, best21, *knobs[1]), args.reps, torch)
        row["match_descriptors"] = timed(lambda: features.match_descriptors(d1[0], d2[0]), args.reps, torch)
        pair_count = 2.0 * n * n  # both directions
        s = row["search"]["gpu_events_ms_median"] * 1e-3
        row["popcounts_per_second"] = pair_count * 8 / s
        row["lane_ops_per_second"] = pair_count * PAIR_LANE_OPS / s
        row["share_of_valu_rate"] = row["lane_ops_per_second"] / VALU_LANE_OPS

        def composed(rows=512):  # xor, a byte popcount table, min -- in row blocks so that the (rows, n, 32) table fits
            out = []
            for r0 in range(0, n, rows):
                x = d1[0, r0:r0 + rows, None, :] ^ d2[0, None, :, :]
                out.append(table[x.long()].sum(-1, dtype=torch.int32).min(1))
            return out
        if n <= 8000:
            row["torch_composition_one_direction"] = timed(composed, max(2, args.reps // 3), torch)
        if n == 2000:
            h1, h2 = d1[0].cpu().numpy(), d2[0].cpu().numpy()
            row["restatement_cpu_ms"] = cpu(lambda: fr.match(h1, h2))
        result["search"].append(row)

    views = frames_1080p(8, torch)
    result["match_views_8_views_28_pairs"] = timed(lambda: features.match_views(views), max(2, args.reps // 2), torch)
    big, one = result["search"][-1], result["frames"][0]
    result["notes"].append(
        "search at %d per side: %.3f of the VALU lane-operation rate (%d operations per pair as the kernel is written); score at "
        "1 frame: %.3f of the copy ceiling.  %s" % (
            big["descriptors_per_side"], big["share_of_valu_rate"], PAIR_LANE_OPS, one["score_share_of_copy_ceiling"],
            "The search is bound by VALU, as expected." if big["share_of_valu_rate"] > 0.5 else
            "Neither ratio is near 1: the search is not yet at the VALU rate (its LDS broadcast reads and the dependent "
            "compare-and-select chain are what is left to look at), and the score kernel is bound by its 256 min/max per pixel, "
            "not by memory."))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
