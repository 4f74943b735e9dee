#!/usr/bin/env python3
"""Times the marker detector (csrc/markers.hip) on the GPU -- HIP events after warm-up, gray frames resident in HBM -- and
writes one JSON record:
    python tools/gpu_markers_time.py [--out profiles/markers_time.json]
A 5 x 5 grid board at 1920 x 1080 with sigma = 4 grey levels of noise; 1, 100 and 1 000 frames; per stage: mask,
labelling, candidates, quadrilateral plus decode, refinement, and the whole ``find_markers``.  Beside it in the same run: the
NumPy restatement tests/markers_ref.py on this machine's CPU, ``find_charuco_corners`` at the same frame size for scale, and
a worst case -- nested square rings up to 500 px about six centres, so that hundreds of candidates have boxes near
``max_side`` and one wave scans up to max_side^2 pixels three times.  The event time is that of the Python binding: the
allocations and the launches.  Every frame is a copy of one image: a best case for the caches."""
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


def gpu_ms(fn, warmup=2, reps=3):
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


def nested_rings():
    img = np.full((H, W), 235, np.uint8)
    for cy in (270, 810):
        for cx in (320, 960, 1600):
            for half in range(250, 8, -5):  # a dark outline 2 px wide every 5 px
                for t in range(2):
                    a = half - t
                    img[cy - a, cx - a:cx + a + 1] = 40
                    img[cy + a, cx - a:cx + a + 1] = 40
                    img[cy - a:cy + a + 1, cx - a] = 40
                    img[cy - a:cy + a + 1, cx + a] = 40
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU fallback to time"
    from calibrating_amd import boards, detect, imgproc
    from calibrating_amd._frames import Frames
    import charuco_cases as cc
    import markers_cases as mc
    import markers_ref as ref
    import subpix_cases as sc

    dictionary = boards.make_marker_dictionary(25, 4, seed=0)
    board = boards.ArucoGridBoard((5, 5), 60.0, 10.0, dictionary)
    K = np.array([[1400.0, 0, 959.5], [0, 1400.0, 539.5], [0, 0, 1]])
    R, t = sc.rodrigues((0.2, -0.25, 0.05)), np.array([0.01, -0.005, 0.62])
    placed, truth = [], []
    for i in board.ids:
        p = board.object_points[int(i)].astype(np.float64)
        Hm = K @ np.stack([R[:, 0], R[:, 1], R @ p[0] + t], 1) @ np.diag([0.06, 0.06, 1.0])
        placed.append((int(i), Hm))
        truth.append(mc.corners_of(Hm))
    old_ss, mc.SS = mc.SS, 2
    clean = mc.render((H, W), placed, dictionary)
    mc.SS = old_ss
    img = np.clip(np.rint(clean.astype(np.float64) + np.random.default_rng(0).normal(0, 4, (H, W))), 0, 255).astype(np.uint8)
    truth = np.stack(truth)

    t0 = time.perf_counter()
    mask = ref.dark_mask(img)
    t1 = time.perf_counter()
    labels = ref.label(mask)
    t2 = time.perf_counter()
    cand = ref.candidates(labels)
    t3 = time.perf_counter()
    exp = ref.find(img, dictionary)
    t4 = time.perf_counter()
    seen, coarse, info = imgproc.find_markers(img, dictionary, refine_win=None, return_info=True)
    assert np.array_equal(seen, exp["seen"][0]) and np.array_equal(coarse, exp["corners"][0], equal_nan=True) and \
        np.array_equal(info["id_turn"], exp["id_turn"][0]), "the kernels and the restatement disagree"
    refined = imgproc.find_markers(img, dictionary)[1]
    rec = dict(grid=[5, 5], bits=4, size=[W, H], noise_sigma=4, candidates=int(info["counts"]), markers_seen=int(seen.sum()),
               coarse_offset_px_max=float(np.abs(coarse - truth)[seen].max()), refined_offset_px_max=float(np.abs(refined - truth)[seen].max()),
               cpu_numpy_restatement_ms_per_frame=dict(mask=1e3 * (t1 - t0), labelling=1e3 * (t2 - t1), candidates=1e3 * (t3 - t2),
                                                       whole=1e3 * (t4 - t3)),
               device=torch.cuda.get_device_name(0), runs=[])
    words = torch.from_numpy(boards.marker_words(dictionary).view(np.int64)).cuda()
    g1 = torch.from_numpy(img).cuda()
    setup = cc.Setup((9, 5), 4, (1, 2), (H, W), 0.5, seed=0)
    setup.K = K
    old_ss, cc.SS = cc.SS, 2
    charuco = torch.from_numpy(cc.render(setup, cc.homography_of_pose(setup, R, np.array([0.01, -0.005, 0.5])))).cuda()
    cc.SS = old_ss
    for f in FRAMES:
        gray = g1[None].repeat(f, 1, 1)
        n = min(f, imgproc.MARKER_PLANE_BUDGET // (20 * H * W))  # the stages alone on one chunk of frames
        part = gray[:n]
        fr = Frames(part, n, H, W, W, H * W, batched=True, was_np=False, colour=False)
        stage = lambda: detect._marker_stages(fr, words, 25, 4, 8, 7, 12, 512, 0)  # noqa: E731
        m = detect._dark_mask(fr, 8, 7)
        mask_ms = gpu_ms(lambda: detect._dark_mask(fr, 8, 7))
        label_ms = gpu_ms(lambda: detect._label_components(m))
        stages_ms = gpu_ms(stage)
        coarse_ms = gpu_ms(lambda: imgproc.find_markers(gray, dictionary, refine_win=None))
        whole_ms = gpu_ms(lambda: imgproc.find_markers(gray, dictionary))
        ch = charuco[None].repeat(f, 1, 1)
        charuco_ms = gpu_ms(lambda: imgproc.find_charuco_corners(ch, setup.squares, setup.dictionary, setup.ratio, setup.first_id))
        rec["runs"].append(dict(frames=f, chunk_frames=n, chunk_mask_ms=mask_ms, chunk_labelling_ms=label_ms,
                                chunk_stages_1_to_6_ms=stages_ms, chunk_candidates_quad_decode_ms=stages_ms[0] - mask_ms[0] - label_ms[0],
                                coarse_ms=coarse_ms, whole_ms=whole_ms, refinement_ms=whole_ms[0] - coarse_ms[0],
                                whole_us_per_frame=1e3 * whole_ms[0] / f, find_charuco_corners_ms=charuco_ms))
        del gray, part, fr, m, ch
    rings = nested_rings()
    s, c, i = imgproc.find_markers(rings, dictionary, refine_win=None, return_info=True)
    boxes = i["candidates"][:int(i["counts"])]
    r1 = torch.from_numpy(rings).cuda()
    rec["worst_case"] = dict(candidates=int(i["counts"]), status=int(i["status"]), largest_box=int((boxes[:, 3] - boxes[:, 1] + 1).max()),
                             box_pixels_scanned_three_times=int(((boxes[:, 3] - boxes[:, 1] + 1) * (boxes[:, 4] - boxes[:, 2] + 1)).sum()),
                             one_frame_ms=gpu_ms(lambda: imgproc.find_markers(r1, dictionary, refine_win=None)),
                             ten_frames_ms=gpu_ms(lambda: imgproc.find_markers(r1[None].repeat(10, 1, 1), dictionary, refine_win=None)))
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
