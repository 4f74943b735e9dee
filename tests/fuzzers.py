"""Seeded fuzzers of the HIP path against the CPU oracle.  One implementation, two users: bounded slices run in the
driver's GPU suite (tests/test_gpu_fuzz.py), and tools/gpu_fuzz*.py run thousands of cases by hand and keep the log.

Every run returns a dict {fuzzer, seed, cases, branches: {name: count}, mismatches: [...]}; ``stamp()`` adds what
identifies the code that was tested (the git SHA handed in through CAMD_GIT_SHA -- .git does not travel to the GPU box --
and a hash of the shipped library)."""
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stamp():
    so = os.path.join(ROOT, "calibrating_amd", "lib", "libcalibrating_amd.so")
    h = hashlib.sha256(open(so, "rb").read()).hexdigest()[:16] if os.path.exists(so) else None
    return dict(git_sha=os.environ.get("CAMD_GIT_SHA", "unknown"), lib_sha256_16=h)


def _count(d, key):
    d[key] = d.get(key, 0) + 1


# ------------------------------------------------------------------------------------------------------------------
def _sgbm_pair(kind, H, W, cn, D, seed, split, slot):
    """One pair of fuzz_sgbm's case kind: 0 noise, 1 opposite sawtooth ramps (shifted by the batch slot), 2 / 3
    rectified texture, 4 drift (synthetic.drift_pair).  Every slot of a batch gets its own pair (seed and shift)."""
    from calibrating_amd import synthetic
    if kind == 4:  # saturation in the upper part, none below: C drifts under P2 / negative -> the exact int path
        left, right = synthetic.drift_pair(H, W, cn, split=split, seed=seed)
        if cn == 1:
            left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    elif kind == 0:
        r2 = np.random.default_rng(seed)
        shape = (H, W) if cn == 1 else (H, W, cn)
        left, right = r2.integers(0, 256, shape, dtype=np.uint8), r2.integers(0, 256, shape, dtype=np.uint8)
    elif kind == 1:  # opposite sawtooth ramps: drives the window sums into saturation when preFilterCap is raised
        x, y = np.arange(W)[None, :], np.arange(H)[:, None]
        ramp = ((x * 16 + y * 40 + 8 * slot) % 256).astype(np.uint8)
        left = ramp if cn == 1 else ramp[..., None].repeat(3, 2)
        right = 255 - left
    else:
        left, right = synthetic.rectified_pair(seed=seed, H=H, W=W, D=max(min(D, W // 2), 8), cn=cn)
    return left, right


# ------------------------------------------------------------------------------------------------------------------
def fuzz_sgbm(n, seed=77, log=print):
    """SGBM against oracle.sgbm_compute: random sizes (incl. widths that leave partial strips / single columns), channel
    counts, disparity ranges, block sizes up to 11, penalties up to the library's P2 limit, preFilterCap up to 63 (the
    saturating regime), all four modes, batches, both cost-kernel paths; every fifth case is built to drift out of the
    int16 regime (synthetic.drift_pair) and must still match bit for bit.  A batch holds distinct pairs of the case's
    kind, each against its own oracle result, so a kernel that reads another slot's data fails."""
    import calibrating_amd as ca
    import oracle
    rng = np.random.default_rng(seed)
    br, bad = {}, []
    for case in range(n):
        cn = int(rng.choice([1, 3]))
        D = int(rng.choice([8, 16, 24, 32, 48, 50, 64, 80, 96, 128, 144, 160, 176, 192, 200, 218, 224, 256, 300]))  # every lane shape
        bs = int(rng.choice([0, 1, 3, 5, 7, 9, 11]))
        minD = int(rng.integers(-9, 10))
        mode = int(rng.choice([0, 1, 2, 3]))
        force_band = bool(rng.integers(0, 2))  # (AUTO sends small 3WAY calls down the scan path)
        b = max(bs, 1)
        W = D + abs(minD) + int(rng.integers(b // 2 + 2, 140))
        H = int(rng.integers(3, 90)) if mode != 2 else int(rng.integers(40, 110))
        P1 = int(rng.integers(1, 8 * cn * b * b + 2))
        P2 = P1 + int(rng.integers(1, 32 * cn * b * b + 2))
        if rng.random() < 0.3:  # up to the library's limit (cv2's rule of thumb 32*cn*b*b is 21600 at block 15 RGB)
            P2 = int(rng.integers(max(P1 + 1, 12000), 24001))
        p = dict(minDisparity=minD, numDisparities=D, blockSize=bs, P1=P1, P2=P2, disp12MaxDiff=int(rng.integers(-1, 4)),
                 uniquenessRatio=int(rng.integers(0, 30)), preFilterCap=int(rng.choice([0, 15, 31, 63])),
                 speckleWindowSize=int(rng.choice([0, 0, 40])), speckleRange=int(rng.integers(1, 4)), mode=mode)
        kind = case % 5
        split = float(rng.uniform(0.2, 0.8)) if kind == 4 else None
        left, right = _sgbm_pair(kind, H, W, cn, D, seed * 100003 + case, split, 0)
        try:
            want = oracle.sgbm_compute(left, right, **p)
        except ValueError:
            _count(br, "refused_by_oracle")
            try:  # the product must refuse too
                ca.StereoSGBM_create(**p).compute(left, right)
                bad.append(dict(case=case, why="oracle refuses, product does not", shape=(H, W, cn), params=p))
            except ValueError:
                pass
            continue
        _count(br, "mode%d" % mode)
        batch, slots = [(left, right)], {0: want}
        _count(br, ("gray" if cn == 1 else "rgb") + ("_drift_input" if kind == 4 else ""))
        try:
            for cost in ((1, 2) if mode != 2 and bs <= 11 else (0,)):
                m = ca.StereoSGBM_create(**p)
                m.set_option("cost", cost)
                if mode == 2 and force_band:
                    m.set_option("path", 2)
                nb = int(rng.choice([1, 1, 3]))
                while len(batch) < nb:
                    batch.append(_sgbm_pair(kind, H, W, cn, D, seed * 100003 + case + 7919 * len(batch), split, len(batch)))
                got = (m.compute(np.stack([a for a, _ in batch[:nb]]), np.stack([b for _, b in batch[:nb]])) if nb > 1
                       else m.compute(left, right)[None])
                _count(br, "cost%d" % cost)
                _count(br, "Dp%d" % m.geometry()["Dp"])  # which lane shape (16 lanes x Dp/32 registers from 96 on)
                if nb > 1:
                    _count(br, "batched")
                if cost != 2 and nb == 1 and mode != 2:
                    # how many cases leave the packed-u16 regime (C < P2 after an int16 overflow): the exact int path
                    P2n = max(p["P2"] if p["P2"] > 0 else 5, (p["P1"] if p["P1"] > 0 else 2) + 1)
                    if int(m.debug_volume("C").min()) < P2n:
                        _count(br, "left_u16_regime")
                for i in range(nb):
                    if i not in slots:  # slot i of a batch holds its own pair of the case's kind
                        slots[i] = oracle.sgbm_compute(*batch[i], **p)
                    if not np.array_equal(got[i], slots[i]):
                        bad.append(dict(case=case, cost=cost, batch="%d/%d" % (i, nb), shape=(H, W, cn), params=p,
                                        pixels=int((got[i] != slots[i]).sum())))
                        log("MISMATCH", bad[-1])
                        break
        except ValueError as e:
            bad.append(dict(case=case, why="refused by the product only: %s" % e, shape=(H, W, cn), params=p))
            log("MISMATCH", bad[-1])
    return dict(fuzzer="sgbm", seed=seed, cases=n, branches=br, mismatches=bad)


# ------------------------------------------------------------------------------------------------------------------
def fuzz_remap(n, seed=5, log=print):
    """The remap kernels through the raw C ABI against oracle.remap_u8: source sizes down to 1x1 (narrower than the 8x8
    window), odd base addresses and padded pitches, maps that wander far outside the image, magnify, fold back and hit
    exact half-phase coordinates; all three interpolations, both channel counts, x-shifts."""
    import torch
    import oracle
    from calibrating_amd import _native, imgproc
    rng = np.random.default_rng(seed)
    br, bad = {}, []
    for case in range(n):
        cn = int(rng.choice([1, 3]))
        sh, sw = int(rng.choice([1, 2, 3, 7, 8, 9, 20, 61])), int(rng.choice([1, 2, 5, 8, 9, 17, 64, 130]))
        dh, dw = int(rng.integers(1, 40)), int(rng.choice([1, 3, 63, 64, 65, 255, 256, 257, 300]))
        img = rng.integers(0, 256, (sh, sw, cn), dtype=np.uint8)
        pad, lead = int(rng.integers(0, 7)), int(rng.integers(0, 9))
        pitch = sw * cn + pad
        buf = np.full(lead + sh * pitch + 64, 255, np.uint8)
        np.lib.stride_tricks.as_strided(buf[lead:], (sh, sw * cn), (pitch, 1))[:] = img.reshape(sh, sw * cn)
        kind = case % 4
        yy, xx = np.mgrid[:dh, :dw].astype(np.float32)
        if kind == 0:    # smooth warp crossing every edge
            mapx = xx * ((sw + 12) / dw) - 6 + rng.uniform(-0.5, 0.5, (dh, dw))
            mapy = yy * ((sh + 12) / dh) - 6 + rng.uniform(-0.5, 0.5, (dh, dw))
        elif kind == 1:  # pure noise, mostly outside
            mapx = rng.uniform(-40, sw + 40, (dh, dw))
            mapy = rng.uniform(-40, sh + 40, (dh, dw))
        elif kind == 2:  # strong magnification on the 1/32 grid (exact phases, half-way rounding cases)
            mapx = np.round(xx * 0.07 * 64) / 64 + rng.integers(-2, max(sw, 2))
            mapy = np.round(yy * 0.11 * 64) / 64 + rng.integers(-2, max(sh, 2))
        else:            # fold-over with huge excursions (the short-range clamp of the cell index)
            mapx = np.where(rng.random((dh, dw)) < 0.1, rng.choice([-1e6, 1e6, 40000.3, -40000.7]), (dw - xx) * sw / dw)
            mapy = np.where(rng.random((dh, dw)) < 0.1, rng.choice([-1e6, 1e6, 32767.5, -32768.5]), (dh - yy) * sh / dh)
        mapx, mapy = mapx.astype(np.float32), mapy.astype(np.float32)
        d_buf, mx, my = torch.from_numpy(buf).cuda(), torch.from_numpy(mapx).cuda(), torch.from_numpy(mapy).cuda()
        _count(br, ("warp", "noise", "magnify", "fold")[kind])
        for interp, iname in ((imgproc.INTER_LANCZOS4, "lanczos4"), (imgproc.INTER_LINEAR, "linear"),
                              (imgproc.INTER_NEAREST, "nearest")):
            shift = int(rng.choice([0, 0, 3, -2]))
            out = torch.full((dh, dw, cn), 77, dtype=torch.uint8, device="cuda")
            rc = _native.lib().camd_remap_u8(d_buf.data_ptr() + lead, sw, sh, cn, pitch, sh * pitch, mx.data_ptr(),
                                             my.data_ptr(), out.data_ptr(), dw, dh, dw * cn, dh * dw * cn, interp, shift, 1,
                                             _native.current_stream())
            _native.check(rc, "remap")
            ref = oracle.remap_u8(img if cn > 1 else img[..., 0], mapx, mapy, interp).reshape(dh, dw, cn)
            if shift:  # stereo_camera.py:230-240: translate the remapped image, zero fill
                sref = np.zeros_like(ref)
                if shift > 0:
                    sref[:, shift:] = ref[:, :-shift] if shift < dw else 0
                else:
                    sref[:, :shift] = ref[:, -shift:] if -shift < dw else 0
                ref = sref
                _count(br, "shifted")
            _count(br, iname)
            got = out.cpu().numpy()
            if not np.array_equal(got, ref):
                d = np.argwhere(got != ref)
                bad.append(dict(case=case, cn=cn, src=(sh, sw), dst=(dh, dw), pad=pad, lead=lead, kind=kind, interp=iname,
                                shift=shift, pixels=len(d), first=d[0].tolist()))
                log("MISMATCH", bad[-1])
    return dict(fuzzer="remap", seed=seed, cases=n, branches=br, mismatches=bad)


# ------------------------------------------------------------------------------------------------------------------
def fuzz_pipeline(n, seed=11, log=print):
    """The whole Stereo.get_depth against tests/oracle_pipeline.oracle_get_depth: random rigs (rotation, baseline,
    distortion, focal lengths; every fourth with a second camera of ANOTHER resolution), xy_target / K_target,
    max_depth (and with it the min_disparity translation), matcher parameters incl. max_size downsizing; and the batched
    form against the same oracle result."""
    import calibrating_amd as ca
    import oracle
    from calibrating_amd import synthetic
    from oracle_pipeline import compare, oracle_get_depth
    rng = np.random.default_rng(seed)
    br, bad, inexact_total = {}, [], {}
    for case in range(n):
        W, H = int(rng.choice([160, 200, 256, 320])), int(rng.choice([96, 120, 150, 200]))
        hetero = case % 4 == 3
        W2, H2 = (int(rng.choice([128, 240, 333])), int(rng.choice([100, 144, 180]))) if hetero else (W, H)
        f = W * rng.uniform(0.6, 1.1)
        f2 = f * W2 / W
        K1 = [[f, 0, W / 2 + rng.uniform(-6, 6)], [0, f * rng.uniform(0.98, 1.02), H / 2 + rng.uniform(-5, 5)], [0, 0, 1]]
        K2 = [[f2 * rng.uniform(0.97, 1.03), 0, W2 / 2 + rng.uniform(-6, 6)],
              [0, f2 * rng.uniform(0.97, 1.03), H2 / 2 + rng.uniform(-5, 5)], [0, 0, 1]]
        dscale = [0.2, 0.08, 2e-3, 2e-3, 0.02]
        rig = dict(R=synthetic.rodrigues(rng.uniform(-0.04, 0.04, 3)).tolist(),
                   t=[[-rng.uniform(0.05, 0.3)], [rng.uniform(-0.01, 0.01)], [rng.uniform(-0.01, 0.01)]],
                   cam1=dict(K=K1, D=[(rng.uniform(-1, 1, 5) * dscale).tolist()], xy=[W, H], name="a"),
                   cam2=dict(K=K2, D=[(rng.uniform(-1, 1, 5) * dscale).tolist()], xy=[W2, H2], name="b"))
        xy_target = [None, None, 0.75, (W + 16, H - 8)][int(rng.integers(0, 4))]
        K_target = float(rng.choice([1, 1, 0.8, 1.2]))
        try:
            stereo = ca.Stereo(ca.Cam.load(rig["cam1"]), ca.Cam.load(rig["cam2"]), xy_target=xy_target, K_target=K_target,
                               R=np.array(rig["R"]), t=np.array(rig["t"]))
        except Exception as e:  # (a degenerate random rig)
            _count(br, "rig_refused")
            log("case", case, "rig refused:", str(e)[:80])
            continue
        Wt, Ht = stereo.xy
        D = int(rng.choice([16, 32, 48, 64]))
        bs = int(rng.choice([3, 5, 7, 11]))
        if Wt - D < 24:
            _count(br, "too_narrow")
            continue
        big = max(Wt, Ht)
        cfg = dict(max_size=int(rng.choice([big, big, int(big * 0.7), big - 1, big // 2])), minDisparity=int(rng.integers(0, 4)),
                   numDisparities=D, blockSize=bs, P1=8 * 3 * bs * bs, P2=32 * 3 * bs * bs,
                   disp12MaxDiff=int(rng.integers(0, 3)), uniquenessRatio=int(rng.integers(0, 15)),
                   speckleWindowSize=int(rng.choice([0, 60])), speckleRange=2, mode=int(rng.choice([0, 1, 3])))
        max_depth = [None, 3.0, 8.0][int(rng.integers(0, 3))]
        stereo.set_stereo_matching(ca.SemiGlobalBlockMatching(cfg), max_depth=max_depth)
        if case % 2:
            img1, img2 = synthetic.render_plane_pair(rig, (rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), 1.0),
                                                     float(rng.uniform(1.0, 2.5)), seed=case)[:2]
        else:
            img1 = synthetic.scene_pair(seed * 100003 + case, W, H, 3)[0]
            img2 = synthetic.scene_pair(seed * 100003 + case, W2, H2, 3)[1]
        downsized = cfg["max_size"] < big
        _count(br, "downsizing" if downsized else "full_resolution")
        _count(br, "hetero_rig" if hetero else "same_size_rig")
        _count(br, "translated" if max_depth else "untranslated")
        ref = oracle_get_depth(oracle, stereo, cfg, img1, img2)
        if (ref["rectify_depth"] > 0).mean() > 0.25:
            _count(br, "over_25pct_valid_depth")
        problems, inexact = compare(stereo.get_depth(img1, img2), ref)
        for k in inexact:
            _count(inexact_total, k)
        # batched form against the same oracle result (second slot; the first holds another pair)
        o1 = synthetic.scene_pair(case + 1000, W, H, 3)[0]
        o2 = synthetic.scene_pair(case + 1000, W2, H2, 3)[1]
        gb = stereo.get_depth_batch(np.stack([o1, img1]), np.stack([o2, img2]))
        pb, ib = compare({k: v[1] for k, v in gb.items()}, ref)
        problems += ["batch:" + k for k in pb]
        if problems:
            bad.append(dict(case=case, cam1=(W, H), cam2=(W2, H2), target=(int(Wt), int(Ht)), cfg=cfg, max_depth=max_depth,
                            problems=problems))
            log("MISMATCH", bad[-1])
    return dict(fuzzer="pipeline", seed=seed, cases=n, branches=br, mismatches=bad,
                within_tolerance_but_not_bit_identical=inexact_total)


def speckle_image(rng, kind, h, w, new_val):
    """Disparity-like int16 images for the speckle filter: smooth regions with noise and holes, few-level noise (many
    tiny components), one-pixel-wide serpentines (a long component through many strips and segments) and combs (teeth
    that only meet at the bottom: every tooth is born as its own tree and merged late)."""
    if kind == 0:
        yy, xx = np.mgrid[:h, :w]
        img = (16 * 20 + 3 * xx + 5 * yy).astype(np.int16)
        for _ in range(int(rng.integers(1, 5))):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            img[y0:y0 + int(rng.integers(1, h + 1)), x0:x0 + int(rng.integers(1, w + 1))] += np.int16(rng.integers(-400, 400))
        spk = rng.random((h, w)) < 0.03
        img[spk] = (rng.integers(0, 100, int(spk.sum())) * 16).astype(np.int16)
        img[rng.random((h, w)) < 0.05] = new_val
    elif kind == 1:
        img = (rng.integers(0, int(rng.integers(2, 6)), (h, w)) * 40).astype(np.int16)
        img[rng.random((h, w)) < 0.2] = new_val
    elif kind == 2:
        tr = rng.random() < 0.5  # (vertical serpentine: built lying down, then transposed)
        hh, ww = (w, h) if tr else (h, w)
        img = np.full((hh, ww), new_val, np.int16)
        step = int(rng.integers(2, 5))
        for r, y in enumerate(range(0, hh, step)):
            img[y, :] = 500
            img[y:min(y + step, hh), ww - 1 if r % 2 == 0 else 0] = 500  # connector alternately right / left
        if tr:
            img = np.ascontiguousarray(img.T)
    else:
        img = np.full((h, w), new_val, np.int16)
        pitch = int(rng.integers(2, 7))
        img[:, ::pitch] = 300
        img[h - 1 if rng.random() < 0.5 else 0, :] = 300
        if rng.random() < 0.3:
            img[(np.indices((h, w)).sum(0) % 2 == 0) & (img == new_val)] = 1000
    return img


def fuzz_speckle(n, seed=9, log=print):
    """camd_filter_speckles_s16 against oracle.filter_speckles_s16 (= cv2.filterSpeckles' flood fill): sizes around the
    64-column segments and 16-row strips of the kernels, batches, thresholds from 0 to "everything", and -- through one
    StereoSGBM handle used for several different pairs -- the handle-owned workspace that is never re-initialised."""
    import oracle
    from calibrating_amd import imgproc
    rng = np.random.default_rng(seed)
    br, bad = {}, []
    for case in range(n):
        kind = case % 4
        h = int(rng.choice([1, 2, 15, 16, 17, 31, 32, 33, 48, 70, 130]))
        w = int(rng.choice([1, 2, 63, 64, 65, 127, 128, 129, 200, 256, 257, 300, 520]))
        new_val = int(rng.choice([-16, 16, 0]))
        nb = int(rng.choice([1, 1, 2, 5]))
        imgs = np.stack([speckle_image(rng, kind, h, w, new_val) for _ in range(nb)])
        max_size = int(rng.choice([0, 1, 5, 40, 200, 5000, h * w]))
        max_diff = int(rng.choice([0, 16, 32, 200]))
        got = imgproc.filterSpeckles(imgs if nb > 1 else imgs[0], new_val, max_size, max_diff)
        got = got if nb > 1 else got[None]
        _count(br, ("smooth", "noise", "serpentine", "comb")[kind])
        if nb > 1:
            _count(br, "batched")
        for i in range(nb):
            want = oracle.filter_speckles_s16(imgs[i], new_val, max_size, max_diff)
            if (want != imgs[i]).any():
                _count(br, "images_with_erased_pixels")
            if not np.array_equal(got[i], want):
                bad.append(dict(case=case, kind=kind, shape=(h, w), image="%d/%d" % (i, nb), new_val=new_val,
                                max_size=max_size, max_diff=max_diff, pixels=int((got[i] != want).sum())))
                log("MISMATCH", bad[-1])
                break
    return dict(fuzzer="speckle", seed=seed, cases=n, branches=br, mismatches=bad)


def report(res, log=print):
    """One greppable summary line per run (what profiles/*_fuzz_*.log keep)."""
    st = stamp()
    log("FUZZ %s git=%s lib=%s seed=%d cases=%d mismatches=%d branches=%s%s" % (
        res["fuzzer"], st["git_sha"], st["lib_sha256_16"], res["seed"], res["cases"], len(res["mismatches"]),
        dict(sorted(res["branches"].items())),
        (" inexact=%s" % res["within_tolerance_but_not_bit_identical"])
        if "within_tolerance_but_not_bit_identical" in res else ""))


# ------------------------------------------------------------------------------------------------------------------
# The kernels around SGBM on the get_depth path.  Each fuzzer is a pure case generator gen_*(seed, case) -> description
# (parameters, host arrays and the branch names the case exercises; NumPy only, so tests/test_fuzzers_cpu.py can check
# the branch floors of the GPU slices without a GPU) and a runner fuzz_*(n, seed, log) that runs the descriptions on the
# device and compares every result with its reference bit for bit (floats as unsigned integers: the sign of zero and
# infinities count).  Every slot of a batch holds its own content.

def same_bits(a, b):
    from oracle_pipeline import same_bits as sb
    return sb(a, b)


def _first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return dict(shape=(a.shape, b.shape))
    if a.dtype.kind in "fc":
        u = np.dtype("u%d" % a.dtype.itemsize)
        d = np.argwhere(np.ascontiguousarray(a).view(u) != np.ascontiguousarray(b).view(u))
    else:
        d = np.argwhere(a != b)
    return dict(elements=len(d), first=d[0].tolist() if len(d) else None,
                got=a[tuple(d[0])].item() if len(d) else None, want=b[tuple(d[0])].item() if len(d) else None)


def _rng(seed, case):
    return np.random.default_rng([seed, case, 0x5eed])


def images_per_group(groups_per_image, batch):
    """The host rule of remap.hip / depth.hip that splits a batch into image groups of one workgroup (zb)."""
    zb = min(batch, 16)
    while zb > 1 and groups_per_image * -(-batch // zb) < 4096:
        zb = (zb + 1) // 2
    return zb


def _group_branches(br, cols, rows, nb):
    zb = images_per_group(cols * rows, nb)
    br.append("batch%d" % nb)
    if zb > 1:
        br.append("grouped_zb%d" % zb)
        if nb % zb:
            br.append("partial_group")
    return zb


# ---- resize (resize.hip: k_resize_u8 / k_resize_f32) ----------------------------------------------------------------
RESIZE_KINDS = ("tiny_axes", "wide_out", "area2", "one_axis_2to1", "same_size", "near_1", "far_ratio", "matcher_ratio")


def _resize_content(rng, kind, shape, f32, slot):
    if kind == 1 and slot == 0:
        return np.zeros(shape, np.float32 if f32 else np.uint8)
    if kind == 2 and slot == 0:
        return np.full(shape, 1e30 if f32 else 255, np.float32 if f32 else np.uint8)
    if not f32:
        if kind == 3:  # steep ramps: the 11-bit weights meet 0 and 255 side by side
            x = np.indices(shape).sum(0)
            return ((x * (97 + slot)) % 2 * 255).astype(np.uint8)
        return rng.integers(0, 256, shape, dtype=np.uint8)
    v = (rng.standard_normal(shape) * 100).astype(np.float32)
    if kind == 3:  # zeros of both signs, negatives, large and tiny magnitudes
        pick = rng.integers(0, 6, shape)
        v = np.select([pick == 0, pick == 1, pick == 2, pick == 3],
                      [np.float32(0), np.float32(-0.0), -np.abs(v) * 1e20, np.abs(v) * 1e-20], v).astype(np.float32)
    return v


def gen_resize(seed, case):
    rng = _rng(seed, case)
    kind = RESIZE_KINDS[case % len(RESIZE_KINDS)]
    fmt = ("u8c1", "u8c3", "f32")[(case // len(RESIZE_KINDS)) % 3]
    r = lambda lo, hi: int(rng.integers(lo, hi + 1))  # noqa: E731
    if kind == "tiny_axes":
        sw, sh, dw, dh = (int(rng.choice([1, 2, 3, 7])) for _ in range(4))
    elif kind == "wide_out":
        dw = int(rng.choice([255, 256, 257, r(258, 2000)]))
        sw = int(rng.choice([1, 2, 3, 7, r(8, 300), r(300, 2000)]))
        sh, dh = r(1, 40), r(1, 30)
    elif kind == "area2":
        dw, dh = int(rng.choice([1, 2, 3, r(4, 300), 500])), r(1, 21)
        sw, sh = 2 * dw, 2 * dh
    elif kind == "one_axis_2to1":
        dw, dh = r(1, 300), r(1, 21)
        if rng.random() < 0.5:
            sw, sh = 2 * dw, int(rng.choice([v for v in (dh, dh + 1, 3 * dh, max(1, dh - 1)) if v != 2 * dh]))
        else:
            sh, sw = 2 * dh, int(rng.choice([v for v in (dw, dw + 1, 3 * dw, max(1, dw - 1)) if v != 2 * dw]))
    elif kind == "same_size":
        sw, sh = r(1, 400), r(1, 30)
        dw, dh = sw, sh
    elif kind == "near_1":
        sw, sh = r(20, 600), r(9, 40)
        dw, dh = sw + int(rng.choice([-1, 1, -3, 2])), sh + int(rng.choice([-1, 0, 1]))
    elif kind == "far_ratio":
        if rng.random() < 0.5:  # <= 1/4
            dw, dh = r(1, 80), r(1, 9)
            sw, sh = dw * r(4, 9) + r(0, 3), dh * r(4, 7) + r(0, 3)
        else:                   # >= 4
            sw, sh = r(1, 60), r(1, 6)
            dw, dh = sw * r(4, 9) + r(0, 3), sh * r(4, 7) + r(0, 3)
    else:  # the matcher's widths and ratios: 1920 / 3840 -> 1000 and back (heights cut to a band of rows)
        big = int(rng.choice([1920, 3840]))
        sh = r(9, 40)
        dh = max(1, int(round(sh * 562 / (1080 if big == 1920 else 2160))))
        sw, dw = big, 1000
        if rng.random() < 0.5:
            sw, sh, dw, dh = dw, dh, sw, sh
    nb = r(1, 5)
    cn = 3 if fmt == "u8c3" else 1
    f32 = fmt == "f32"
    content = int(rng.integers(0, 4))
    shape = (sh, sw, cn) if cn == 3 else (sh, sw)
    src = np.stack([_resize_content(rng, content, shape, f32, i) for i in range(nb)])
    br = [kind, fmt]
    path = ("memcpy" if (sw, sh) == (dw, dh) else "area" if (sw == 2 * dw and sh == 2 * dh) else "generic")
    br.append("path_" + path)
    if min(sw, sh, dw, dh) == 1:
        br.append("axis_of_1")
    if dw > 256:
        br.append("dw_over_256")
    if dw in (255, 256, 257):
        br.append("dw_255_257")
    if dh % 8:
        br.append("dh_not_multiple_of_8")
    if nb > 1:
        br.append("batched")
    if content == 2 and not f32:
        br.append("const255")
    if content == 1:
        br.append("const0")
    if content == 3 and f32:
        br.append("f32_signed_zeros_large")
    return dict(fmt=fmt, cn=cn, src=src, sw=sw, sh=sh, dw=dw, dh=dh, nb=nb, branches=br)


GUARD = 256  # elements behind every output buffer that a kernel must not touch


def fuzz_resize(n, seed=21, log=print):
    """camd_resize_linear_u8 (cn 1 / 3) and camd_resize_linear_f32 through the raw C ABI against oracle.resize_linear,
    image by image in a batch of 1-5: axes of 1..7 px, outputs 255..2000 px wide, heights off the 8-row blocks, the
    area, memcpy and generic paths, ratios near 1, <= 1/4 and >= 4, the matcher's own ratios, constant 0 / 255
    content and float32 with zeros of both signs, negatives and large magnitudes."""
    import torch
    import oracle
    from calibrating_amd import _native
    br, bad = {}, []
    for case in range(n):
        c = gen_resize(seed, case)
        f32, nb, dw, dh, cn = c["fmt"] == "f32", c["nb"], c["dw"], c["dh"], c["cn"]
        src = torch.from_numpy(np.ascontiguousarray(c["src"])).cuda()
        m = nb * dh * dw * cn
        if f32:
            out = torch.full((m + GUARD,), 0x7fbadbad, dtype=torch.int32, device="cuda")
            rc = _native.lib().camd_resize_linear_f32(src.data_ptr(), c["sw"], c["sh"], out.data_ptr(), dw, dh, nb,
                                                      _native.current_stream())
            got = out.cpu().numpy()
            guard_ok = (got[m:] == 0x7fbadbad).all()
            got = got[:m].view(np.float32).reshape((nb, dh, dw))
        else:
            out = torch.full((m + GUARD,), 77, dtype=torch.uint8, device="cuda")
            rc = _native.lib().camd_resize_linear_u8(src.data_ptr(), c["sw"], c["sh"], cn, out.data_ptr(), dw, dh, nb,
                                                     _native.current_stream())
            got = out.cpu().numpy()
            guard_ok = (got[m:] == 77).all()
            got = got[:m].reshape((nb, dh, dw) + ((cn,) if cn == 3 else ()))
        _native.check(rc, "resize")
        for k in c["branches"]:
            _count(br, k)
        where = dict(case=case, fmt=c["fmt"], src=(c["sh"], c["sw"]), dst=(dh, dw), nb=nb)
        if not guard_ok:
            bad.append(dict(where, why="wrote past the output"))
            log("MISMATCH", bad[-1])
            continue
        for i in range(nb):
            want = oracle.resize_linear(c["src"][i], (dh, dw))
            if not same_bits(got[i], want):
                bad.append(dict(where, image="%d/%d" % (i, nb), **_first_diff(got[i], want)))
                log("MISMATCH", bad[-1])
                break
    return dict(fuzzer="resize", seed=seed, cases=n, branches=br, mismatches=bad)


# ---- depth (depth.hip: k_disp_to_depth, k_unrectify; resize.hip: k_disp16_up_to_depth) -----------------------------
DEPTH_ENTRIES = ("disp_to_depth", "disp16_resized", "unrectify")


def _disp16(rng, shape, extremes):
    v = rng.integers(-40, 16 * 120, shape).astype(np.int16)
    if extremes:
        hit = rng.random(shape) < 0.15
        v[hit] = rng.choice(np.array([-32768, 32767, -16, 0, -1, 1], np.int16), int(hit.sum()))
    return v


def _depth_params(rng, br):
    minD = int(rng.choice([-5, -1, 0, 0, 1, 2, 7]))
    translate = bool(rng.integers(0, 2))
    add = int(rng.choice([-3, -1, 0, 1, 2, 5]))
    bf = float(rng.uniform(5, 400)) * (-1 if rng.random() < 0.15 else 1)
    max_depth = float("inf") if rng.random() < 0.4 else float(rng.uniform(0.5, 60))
    br.append("minD_neg" if minD < 0 else "minD_zero" if minD == 0 else "minD_pos")
    br.append("max_depth_inf" if max_depth == float("inf") else "max_depth_finite")
    if bf < 0:
        br.append("negative_baseline_fx")
    if translate:
        br.append("translated")
        if add < 0:
            br.append("translated_negative_add")  # masked pixels become -0.0
    return dict(sgbm_min_disparity=minD, add_min_disparity=add, translate=translate, baseline_fx=bf,
                max_depth=max_depth)


def gen_depth(seed, case):
    rng = _rng(seed, case)
    entry = DEPTH_ENTRIES[case % 3]
    br = [entry]
    r = lambda lo, hi: int(rng.integers(lo, hi + 1))  # noqa: E731
    if entry == "disp_to_depth":
        w, h = r(1, 300), r(1, 40)
        if (w * h) % 2 != (case // 3) % 2:  # odd and even w*h in turn: images of a batch start on odd elements
            w = w + 1 if w < 300 else w - 1
            if (w * h) % 2 != (case // 3) % 2:
                h += 1
        nb = int(rng.choice([1, 2, 3, 4]))
        extremes = rng.random() < 0.5
        p = _depth_params(rng, br)
        br.append("odd_wh" if (w * h) % 2 else "even_wh")
        if nb > 1:
            br.append("batched")
            if (w * h) % 2:
                br.append("batched_odd_wh")
        if extremes:
            br.append("int16_extremes")
        return dict(entry=entry, disp16=np.stack([_disp16(rng, (h, w), extremes) for _ in range(nb)]),
                    mask=(rng.random((h, w)) < 0.8).astype(np.uint8), branches=br, **p)
    if entry == "disp16_resized":
        sw, sh = int(rng.choice([1, r(2, 40), r(40, 200)])), int(rng.choice([1, r(2, 12), r(12, 40)]))
        if rng.random() < 0.3:  # just above 1
            w, h = sw + r(1, 2), sh + r(0, 1)
        else:
            rx = float(rng.choice([1.5, 2.0, 3.0, 4.0, rng.uniform(1.01, 4.0)]))
            w, h = max(sw + 1, int(round(sw * rx))), max(sh, int(round(sh * rx)))
        if rng.random() < 0.25:  # outputs wider than a 256-lane block
            sw = r(120, 300)
            w = int(round(sw * rng.uniform(1.05, 3.0)))
        nb = int(rng.choice([1, 2, 3]))
        p = _depth_params(rng, br)
        br.append("src_axis_of_1" if min(sw, sh) == 1 else "src_2d")
        if w % sw:
            br.append("non_integer_ratio")
        if w > 256:
            br.append("w_over_256")
        if nb > 1:
            br.append("batched")
        return dict(entry=entry, disp16=np.stack([_disp16(rng, (sh, sw), rng.random() < 0.3) for _ in range(nb)]),
                    hw=(h, w), mask=(rng.random((h, w)) < 0.8).astype(np.uint8), branches=br, **p)
    # unrectify: z-rescale + nearest remap through float maps, shared by every image of the batch
    w, h = r(1, 120), r(1, 90)
    nb = int(rng.choice([1, 15, 16, 17, 33]))
    tall = nb >= 15 and rng.random() < 0.5  # enough workgroups per image that the batch is split into groups of zb
    ow = int(rng.choice([1, 100, 255, 256, 257, 300, 600]))
    oh = r(1100, 1300) if tall and ow > 256 else r(1, 30)
    if tall and ow <= 256:
        ow = 257
        oh = r(1100, 1300)
    kind = int(rng.integers(0, 3))
    yy, xx = np.mgrid[:oh, :ow].astype(np.float64)
    mapx = xx * ((w + 6) / ow) - 3 + rng.uniform(-0.3, 0.3, (oh, ow))
    mapy = yy * ((h + 6) / oh) - 3 + rng.uniform(-0.3, 0.3, (oh, ow))
    if kind == 1:  # exact halves: cvRound rounds them to even
        mapx = np.floor(mapx) + 0.5
        mapy = np.where(rng.random((oh, ow)) < 0.5, np.floor(mapy) + 0.5, mapy)
        br.append("half_coordinates")
    elif kind == 2:  # saturation of the int16 cast and far outside
        hit = rng.random((oh, ow)) < 0.2
        mapx = np.where(hit, rng.choice([-32768.5, 32768.5, -32767.5, 32767.5, -1e6, 1e6], (oh, ow)), mapx)
        hit = rng.random((oh, ow)) < 0.2
        mapy = np.where(hit, rng.choice([-32768.5, 32768.5, 32767.5, -1e6, 1e6, -40000.0], (oh, ow)), mapy)
        br.append("saturating_far_coordinates")
    else:
        br.append("smooth_map")
    depth = rng.uniform(0.2, 30, (nb, h, w))
    depth[rng.random((nb, h, w)) < 0.2] = 0
    _group_branches(br, -(-ow // 256), oh, nb)
    if ow > 256:
        br.append("ow_over_256")
    M = rng.uniform(-2e-3, 2e-3, 3)
    M[2] = rng.uniform(0.8, 1.2)
    return dict(entry=entry, depth=depth, M=M, mapx=mapx.astype(np.float32), mapy=mapy.astype(np.float32),
                branches=br)


def depth_reference(oracle, c, i):
    """The reference result of image i of a gen_depth description (float32 disparity / float64 depth as a tuple)."""
    from oracle_pipeline import resized_disparity_to_depth
    keys = ("sgbm_min_disparity", "add_min_disparity", "translate", "baseline_fx", "max_depth")
    if c["entry"] == "disp_to_depth":
        return oracle.disp_to_depth(c["disp16"][i], c["mask"], *(c[k] for k in keys))
    if c["entry"] == "disp16_resized":
        return resized_disparity_to_depth(oracle, c["disp16"][i], c["hw"], c["mask"], *(c[k] for k in keys))
    return (oracle.unrectify_depth(c["depth"][i], c["M"], c["mapx"], c["mapy"]),)


def fuzz_depth(n, seed=31, log=print):
    """camd_disp_to_depth against oracle.disp_to_depth, camd_disp16_resized_to_depth against the NumPy composition of
    oracle_pipeline (resize of the prepared float32 disparity, then the reference's lines) and camd_unrectify_depth
    against oracle.unrectify_depth: odd w*h in batches, int16 extremes, minDisparity < = > 0, translation with a
    negative min_disparity (-0.0 on masked pixels), max_depth finite / inf, a negative baseline*fx; up-ratios from just
    above 1 to 4 and 1-px source axes; maps with exact halves, at the int16 saturation and far outside, batches that
    cross the 16-image groups.  Float outputs are compared bit for bit."""
    import ctypes
    import torch
    import oracle
    from calibrating_amd import _native
    br, bad = {}, []
    for case in range(n):
        c = gen_depth(seed, case)
        st = _native.current_stream()
        if c["entry"] == "unrectify":
            nb, h, w = c["depth"].shape
            oh, ow = c["mapx"].shape
            z = torch.from_numpy(c["depth"]).cuda()
            mx, my = torch.from_numpy(c["mapx"]).cuda(), torch.from_numpy(c["mapy"]).cuda()
            m = nb * oh * ow
            out = torch.full((m + GUARD,), 0x7ff00000badbad00, dtype=torch.int64, device="cuda")
            M = (ctypes.c_double * 3)(*[float(v) for v in c["M"]])
            rc = _native.lib().camd_unrectify_depth(z.data_ptr(), w, h, M, mx.data_ptr(), my.data_ptr(), out.data_ptr(),
                                                    ow, oh, nb, st)
            _native.check(rc, "unrectify")
            o = out.cpu().numpy()
            outs = [(o[:m].view(np.float64).reshape(nb, oh, ow),)]
            guard_ok = (o[m:] == 0x7ff00000badbad00).all()
        else:
            nb = c["disp16"].shape[0]
            sh, sw = c["disp16"].shape[1:]
            h, w = c["hw"] if c["entry"] == "disp16_resized" else (sh, sw)
            d = torch.from_numpy(c["disp16"]).cuda()
            mk = torch.from_numpy(c["mask"]).cuda()
            m = nb * h * w
            disp = torch.full((m + GUARD,), 0x7fbadbad, dtype=torch.int32, device="cuda")
            dep = torch.full((m + GUARD,), 0x7ff00000badbad00, dtype=torch.int64, device="cuda")
            args = (c["sgbm_min_disparity"], c["add_min_disparity"], int(c["translate"]), ctypes.c_double(c["baseline_fx"]),
                    ctypes.c_double(c["max_depth"]), disp.data_ptr(), dep.data_ptr(), nb, st)
            if c["entry"] == "disp_to_depth":
                rc = _native.lib().camd_disp_to_depth(d.data_ptr(), mk.data_ptr(), w, h, *args)
            else:
                rc = _native.lib().camd_disp16_resized_to_depth(d.data_ptr(), sw, sh, mk.data_ptr(), w, h, *args)
            _native.check(rc, c["entry"])
            g1, g2 = disp.cpu().numpy(), dep.cpu().numpy()
            guard_ok = (g1[m:] == 0x7fbadbad).all() and (g2[m:] == 0x7ff00000badbad00).all()
            outs = [(g1[:m].view(np.float32).reshape(nb, h, w), g2[:m].view(np.float64).reshape(nb, h, w))]
        for k in c["branches"]:
            _count(br, k)
        where = dict(case=case, entry=c["entry"], nb=nb, params={k: c[k] for k in (
            "sgbm_min_disparity", "add_min_disparity", "translate", "baseline_fx", "max_depth") if k in c})
        if not guard_ok:
            bad.append(dict(where, why="wrote past the output"))
            log("MISMATCH", bad[-1])
            continue
        signed_zero = False
        for i in range(nb):
            want = depth_reference(oracle, c, i)
            for name, g, r in zip(("disparity", "depth") if len(want) == 2 else ("depth",), outs[0], want):
                signed_zero |= bool(np.signbit(r[r == 0]).any())
                if not same_bits(g[i], r):
                    bad.append(dict(where, image="%d/%d" % (i, nb), output=name, **_first_diff(g[i], r)))
                    log("MISMATCH", bad[-1])
                    break
            else:
                continue
            break
        if signed_zero:
            _count(br, "reference_has_negative_zero")
    return dict(fuzzer="depth", seed=seed, cases=n, branches=br, mismatches=bad)


# ---- fixed-point bilinear remap (remap.hip: k_remap_fixed_bilinear, the cv2.undistort step) -------------------------
FIXED_REMAP_KINDS = ("arbitrary", "undistort_maps", "high_mapa_bits", "grouped_batch")


def _undistort_rig(rng, w, h, ndist):
    f = w * rng.uniform(0.7, 1.3)
    K = np.array([[f, 0, w / 2 + rng.uniform(-5, 5)], [0, f * rng.uniform(0.95, 1.05), h / 2 + rng.uniform(-5, 5)],
                  [0, 0, 1]])
    scale = np.array([0.3, 0.1, 3e-3, 3e-3, 0.05, 0.1, 0.05, 0.02, 3e-3, 1e-3, 3e-3, 1e-3])[:ndist]
    return K, rng.uniform(-1, 1, ndist) * scale


def gen_fixed_remap(seed, case):
    rng = _rng(seed, case)
    kind = FIXED_REMAP_KINDS[case % 4]
    cn = int(rng.choice([1, 3])) if kind != "grouped_batch" else 1
    r = lambda lo, hi: int(rng.integers(lo, hi + 1))  # noqa: E731
    br = [kind, "cn%d" % cn]
    K = D = None
    if kind == "undistort_maps":
        ndist = int((4, 5, 8, 12)[(case // 4) % 4])
        sw, sh = r(8, 200), r(4, 120)
        dw, dh = sw, sh
        K, D = _undistort_rig(rng, sw, sh, ndist)
        br.append("ndist%d" % ndist)
        mapxy = mapa = None  # built by the runner (host and device), compared with each other
    else:
        sw, sh = int(rng.choice([1, 2, 3, r(4, 40), r(40, 300)])), int(rng.choice([1, 2, r(3, 30), r(30, 100)]))
        if kind == "grouped_batch":  # enough workgroups per image that remap splits the batch into groups of zb
            dw, dh = r(257, 300), r(1024, 1100)
        else:
            dw, dh = int(rng.choice([1, 3, 64, 255, 256, 257, r(2, 400)])), r(1, 30)
        sx = rng.integers(-3, sw + 3, (dh, dw))
        sy = rng.integers(-3, sh + 3, (dh, dw))
        # cells hanging over every edge and corner, and the int16 extremes
        pick = rng.random((dh, dw))
        sx = np.where(pick < 0.1, rng.choice([-1, sw - 1, -2, sw], (dh, dw)), sx)
        sy = np.where((pick > 0.05) & (pick < 0.15), rng.choice([-1, sh - 1, -2, sh], (dh, dw)), sy)
        ext = rng.random((dh, dw)) < 0.03
        sx = np.where(ext, rng.choice([-32768, 32767, -32767, 32766], (dh, dw)), sx)
        sy = np.where(rng.random((dh, dw)) < 0.03, rng.choice([-32768, 32767, -32767, 32766], (dh, dw)), sy)
        mapxy = np.stack([sx, sy], -1).astype(np.int16)
        mapa = rng.integers(0, 1024, (dh, dw)).astype(np.uint16)
        if kind == "high_mapa_bits":
            mapa |= (rng.integers(1, 64, (dh, dw)) << 10).astype(np.uint16)
    nb = int(rng.choice([17, 33])) if kind == "grouped_batch" else int(rng.choice([1, 1, 2, 5]))
    pad, lead = int(rng.integers(0, 7)), int(rng.integers(0, 9))
    dpad, dlead = int(rng.integers(0, 5)), int(rng.integers(0, 4))
    gap, dgap = int(rng.choice([0, 0, 5, 64])), int(rng.choice([0, 0, 3, 40]))  # extra bytes between the images
    src = rng.integers(0, 256, (nb, sh, sw, cn), dtype=np.uint8)
    if rng.random() < 0.2:
        src[0] = 255
    _group_branches(br, -(-dw // 256), dh, nb)
    if nb > 1:
        br.append("batched")
    if pad:
        br.append("padded_pitch")
    if lead % 2:
        br.append("odd_base")
    if gap or dgap:
        br.append("pair_stride_gap")
    if mapxy is not None and (np.abs(mapxy.astype(np.int32)) >= 32766).any():
        br.append("int16_extreme_cells")
    if min(sw, sh) <= 2:
        br.append("src_axis_1_or_2")
    return dict(kind=kind, cn=cn, src=src, sw=sw, sh=sh, dw=dw, dh=dh, nb=nb, mapxy=mapxy, mapa=mapa, K=K, D=D,
                pad=pad, lead=lead, dpad=dpad, dlead=dlead, gap=gap, dgap=dgap, branches=br)


def fuzz_fixed_remap(n, seed=41, log=print):
    """camd_remap_fixed_bilinear_u8 through the raw C ABI against tests/np_fixed_remap (a NumPy model of cv2's
    remapBilinear on CV_16SC2 + CV_16UC1 maps, BORDER_CONSTANT 0): arbitrary int16 cells (incl. -32768 / 32767, over
    every edge and corner), phase maps with bits above 1023, padded pitches, odd base addresses, gaps between the
    images, batches split into 16-image groups, cn 1 / 3; and the maps of camd_undistort_maps for random K / D with
    4, 5, 8 and 12 coefficients, which must equal the host's (camd_undistort_maps_host).  Before the model judges the
    kernel it must reproduce oracle.undistort_u8 on those host maps."""
    import torch
    import oracle
    from calibrating_amd import _native, imgproc
    import np_fixed_remap
    itab = oracle.bilinear_itab()
    br, bad = {}, []
    for case in range(n):
        c = gen_fixed_remap(seed, case)
        nb, cn, sw, sh, dw, dh = c["nb"], c["cn"], c["sw"], c["sh"], c["dw"], c["dh"]
        where = dict(case=case, kind=c["kind"], cn=cn, src=(sh, sw), dst=(dh, dw), nb=nb)
        mapxy, mapa = c["mapxy"], c["mapa"]
        if c["kind"] == "undistort_maps":
            mapxy, mapa = imgproc.undistort_maps(c["K"], c["D"], (sw, sh))
            dxy, da = imgproc.undistort_maps_device(c["K"], c["D"], (sw, sh))
            if not (np.array_equal(dxy.cpu().numpy(), mapxy) and np.array_equal(da.cpu().numpy().view(np.uint16), mapa)):
                bad.append(dict(where, why="device maps differ from the host maps"))
                log("MISMATCH", bad[-1])
                continue
            img0 = c["src"][0] if cn == 3 else c["src"][0, ..., 0]
            model = np_fixed_remap.remap_fixed_bilinear(img0, mapxy, mapa, itab)
            assert np.array_equal(model, oracle.undistort_u8(img0, c["K"], c["D"])), \
                "np_fixed_remap does not reproduce oracle.undistort_u8 (case %d)" % case
        pitch, dpitch = sw * cn + c["pad"], dw * cn + c["dpad"]
        stride, dstride = sh * pitch + c["gap"], dh * dpitch + c["dgap"]
        buf = np.full(c["lead"] + nb * stride + 64, 255, np.uint8)
        for i in range(nb):
            o = c["lead"] + i * stride
            np.lib.stride_tricks.as_strided(buf[o:], (sh, sw * cn), (pitch, 1))[:] = c["src"][i].reshape(sh, sw * cn)
        dn = c["dlead"] + nb * dstride + GUARD
        d_buf = torch.from_numpy(buf).cuda()
        mxy = torch.from_numpy(np.ascontiguousarray(mapxy)).cuda()
        ma = torch.from_numpy(np.ascontiguousarray(mapa).view(np.int16)).cuda()
        out = torch.full((dn,), 77, dtype=torch.uint8, device="cuda")
        rc = _native.lib().camd_remap_fixed_bilinear_u8(
            d_buf.data_ptr() + c["lead"], sw, sh, cn, pitch, stride, mxy.data_ptr(), ma.data_ptr(),
            out.data_ptr() + c["dlead"], dw, dh, dpitch, dstride, nb, _native.current_stream())
        _native.check(rc, "remap_fixed_bilinear")
        got = out.cpu().numpy()
        for k in c["branches"]:
            _count(br, k)
        written = np.zeros(dn, bool)
        wants = np_fixed_remap.remap_fixed_bilinear_batch(c["src"], mapxy, mapa, itab)
        for i in range(nb):
            o = c["dlead"] + i * dstride
            view = np.lib.stride_tricks.as_strided(got[o:], (dh, dw * cn), (dpitch, 1))
            np.lib.stride_tricks.as_strided(written[o:], (dh, dw * cn), (dpitch, 1))[:] = True
            want = wants[i].reshape(dh, dw * cn)
            if not np.array_equal(view, want):
                bad.append(dict(where, image="%d/%d" % (i, nb), **_first_diff(view, want)))
                log("MISMATCH", bad[-1])
                break
        else:
            if (got[~written] != 77).any():
                bad.append(dict(where, why="wrote outside the destination rows"))
                log("MISMATCH", bad[-1])
    return dict(fuzzer="fixed_remap", seed=seed, cases=n, branches=br, mismatches=bad)


# ---- median 3x3 (post.hip: k_median3) -------------------------------------------------------------------------------
def gen_median(seed, case):
    rng = _rng(seed, case)
    w = int(rng.choice([1, 2, 3, 511, 512, 513, int(rng.integers(4, 120))]))
    h = int(rng.choice([1, 2, 7, 8, 9, int(rng.integers(3, 40))]))
    nb = int(rng.choice([1, 2, 3, 5]))
    if nb > 1 and case % 2 and (w * h) % 2 == 0:  # every other batched case with odd w*h: images start on odd elements
        if w not in (2, 512):
            w += 1 - w % 2
        if h not in (2, 8):
            h += 1 - h % 2
    content = int(rng.integers(0, 3))
    if content == 0:
        imgs = rng.integers(-32768, 32768, (nb, h, w)).astype(np.int16)
    elif content == 1:  # few levels: ties everywhere
        imgs = (rng.integers(0, 3, (nb, h, w)) * 16 - 16).astype(np.int16)
    else:               # extremes scattered over a smooth field
        imgs = (np.indices((h, w)).sum(0)[None] * 7 + rng.integers(0, 50, (nb, 1, 1))).astype(np.int16)
        hit = rng.random((nb, h, w)) < 0.3
        imgs[hit] = rng.choice(np.array([-32768, 32767, -16, 0], np.int16), int(hit.sum()))
    br = ["w%d" % w if w in (1, 2, 3, 511, 512, 513) else "w_other", "h%d" % h if h in (1, 2, 7, 8, 9) else "h_other",
          ("noise", "few_levels", "int16_extremes")[content]]
    if nb > 1:
        br.append("batched")
        if (w * h) % 2:
            br.append("batched_odd_wh")
    return dict(imgs=imgs, branches=br)


def fuzz_median(n, seed=51, log=print):
    """camd_median3_s16 (cv2.medianBlur(disp, 3) on int16, replicate border) against oracle.median3_s16: widths 1, 2,
    3 and around 512 (two pixels per lane, 256 lanes), heights 1, 2 and around the 8-row blocks, batches whose images
    start on odd elements, int16 extremes and ties."""
    import oracle
    from calibrating_amd import imgproc
    br, bad = {}, []
    for case in range(n):
        c = gen_median(seed, case)
        imgs = c["imgs"]
        got = imgproc.medianBlur3_s16(imgs)
        for k in c["branches"]:
            _count(br, k)
        for i in range(len(imgs)):
            want = oracle.median3_s16(imgs[i])
            if not np.array_equal(got[i], want):
                bad.append(dict(case=case, shape=imgs.shape, image=i, **_first_diff(got[i], want)))
                log("MISMATCH", bad[-1])
                break
    return dict(fuzzer="median", seed=seed, cases=n, branches=br, mismatches=bad)


# ---- rectify tables (tables.hip: camd_init_undistort_rectify_map with the valid mask) --------------------------------
TABLE_SIZES = ((1, 1), (2, 3), (7, 5), (1023, 4), (1024, 3), (1025, 6), (2049, 3), (640, 480), (3840, 2160))


def gen_tables(seed, case):
    rng = _rng(seed, case)
    ndist = (0, 4, 5, 8, 12)[case % 5]
    if case % 23 == 22:
        w, h = 3840, 2160
    elif case % 3 == 0:
        w, h = TABLE_SIZES[int(rng.integers(0, len(TABLE_SIZES) - 1))]
    else:
        w, h = int(rng.integers(1, 700)), int(rng.integers(1, 300))
    sw, sh = int(rng.integers(max(1, w // 2), w + 40)), int(rng.integers(max(1, h // 2), h + 40))
    f = max(sw, 8) * rng.uniform(0.6, 1.4)
    A = np.array([[f, rng.uniform(-1, 1), sw / 2 + rng.uniform(-9, 9)],
                  [0, f * rng.uniform(0.9, 1.1), sh / 2 + rng.uniform(-9, 9)], [0, 0, 1]])
    fn = max(w, 8) * rng.uniform(0.5, 1.5)
    Anew = np.array([[fn, 0, w / 2 + rng.uniform(-9, 9)], [0, fn * rng.uniform(0.9, 1.1), h / 2 + rng.uniform(-9, 9)],
                     [0, 0, 1]])
    from calibrating_amd import synthetic
    R = None if case % 4 == 1 else synthetic.rodrigues(rng.uniform(-0.1, 0.1, 3))
    strong = rng.random() < 0.35
    scale = np.array([0.3, 0.1, 3e-3, 3e-3, 0.05, 0.1, 0.05, 0.02, 3e-3, 1e-3, 3e-3, 1e-3])[:ndist]
    D = rng.uniform(-1, 1, ndist) * scale * (12 if strong else 1)
    br = ["ndist%d" % ndist, "R_none" if R is None else "R_given", "w_over_1024" if w > 1024 else "w_le_1024"]
    if strong and ndist:
        br.append("strong_distortion")
    if (w, h) == (1, 1):
        br.append("size_1x1")
    if (w, h) == (3840, 2160):
        br.append("size_3840x2160")
    return dict(A=A, D=D if ndist else None, R=R, Anew=Anew, size=(w, h), src=(sw, sh), branches=br)


def fuzz_tables(n, seed=61, log=print):
    """camd_init_undistort_rectify_map (float maps and the rectify valid mask) against oracle.init_undistort_rectify_map
    and geometry.init_undistort_rectify_map: random K, Anew and R (or none), 0/4/5/8/12 distortion coefficients with
    strong ones that fold the map, targets from 1x1 to 3840x2160 and across the 1024-column chunks of the kernel."""
    import oracle
    from calibrating_amd import geometry, imgproc
    br, bad = {}, []
    for case in range(n):
        c = gen_tables(seed, case)
        mx, my, mk = imgproc.init_undistort_rectify_map(c["A"], c["D"], c["R"], c["Anew"], c["size"], valid_for=c["src"])
        got = (mx.cpu().numpy(), my.cpu().numpy(), mk.cpu().numpy())
        ox, oy = oracle.init_undistort_rectify_map(c["A"], c["D"], c["R"], c["Anew"], c["size"])
        gx, gy = geometry.init_undistort_rectify_map(c["A"], c["D"], c["R"], c["Anew"], c["size"])
        want_mask = geometry.valid_mask_from_maps(ox, oy, c["src"]).astype(np.uint8)
        for k in c["branches"]:
            _count(br, k)
        if not np.isfinite(ox).all() or not np.isfinite(oy).all():
            _count(br, "non_finite_map_values")
        if want_mask.all() or not want_mask.any():
            _count(br, "mask_uniform")
        else:
            _count(br, "mask_mixed")
        where = dict(case=case, size=c["size"], ndist=0 if c["D"] is None else len(c["D"]), R=c["R"] is not None)
        for name, g, r in (("mapx", got[0], ox), ("mapy", got[1], oy), ("mapx_vs_geometry", got[0], gx),
                           ("mapy_vs_geometry", got[1], gy), ("mask", got[2], want_mask)):
            if not same_bits(g, r):
                bad.append(dict(where, output=name, **_first_diff(g, r)))
                log("MISMATCH", bad[-1])
                break
    return dict(fuzzer="tables", seed=seed, cases=n, branches=br, mismatches=bad)


# The bounded slices of tests/test_gpu_fuzz.py for the fuzzers above: (cases per seed, seeds, branch floors).  The
# floors are checked twice: on the GPU against what the runs counted, and without one (tests/test_fuzzers_cpu.py)
# against what the generators promise.
POST_SLICES = {
    "resize": (120, (441, 442), dict(
        tiny_axes=25, wide_out=25, area2=25, one_axis_2to1=25, same_size=25, near_1=25, far_ratio=25, matcher_ratio=25,
        u8c1=70, u8c3=70, f32=70, path_memcpy=25, path_area=25, path_generic=150, axis_of_1=25, dw_over_256=60,
        dw_255_257=10, dh_not_multiple_of_8=150, batched=150, const255=15, const0=30, f32_signed_zeros_large=10)),
    "depth": (120, (451, 452), dict(
        disp_to_depth=75, disp16_resized=75, unrectify=75, batched_odd_wh=10, odd_wh=20, even_wh=20, int16_extremes=30,
        minD_neg=30, minD_zero=30, minD_pos=30, translated_negative_add=15, max_depth_inf=50, max_depth_finite=50,
        negative_baseline_fx=10, src_axis_of_1=20, non_integer_ratio=20, w_over_256=15, half_coordinates=20,
        saturating_far_coordinates=20, batch1=8, batch15=8, batch16=8, batch17=8, batch33=8, grouped_zb16=5,
        partial_group=5, ow_over_256=30)),
    "fixed_remap": (48, (461, 462), dict(
        arbitrary=20, undistort_maps=20, high_mapa_bits=20, grouped_batch=20, cn1=30, cn3=20, ndist4=4, ndist5=4,
        ndist8=4, ndist12=4, grouped_zb16=8, partial_group=8, padded_pitch=40, odd_base=30, pair_stride_gap=20,
        int16_extreme_cells=40, src_axis_1_or_2=10, batched=20)),
    "median": (100, (471, 472), dict(
        w1=15, w2=15, w3=15, w511=15, w512=15, w513=15, h1=15, h2=15, h7=15, h8=15, h9=15, batched=100,
        batched_odd_wh=30, int16_extremes=40, few_levels=40)),
    "tables": (46, (481, 482), dict(
        ndist0=10, ndist4=10, ndist5=10, ndist8=10, ndist12=10, R_none=15, R_given=40, w_over_1024=8,
        strong_distortion=15, size_1x1=2, size_3840x2160=2)),
}
POST_FUZZERS = dict(resize=(gen_resize, fuzz_resize), depth=(gen_depth, fuzz_depth),
                    fixed_remap=(gen_fixed_remap, fuzz_fixed_remap), median=(gen_median, fuzz_median),
                    tables=(gen_tables, fuzz_tables))
