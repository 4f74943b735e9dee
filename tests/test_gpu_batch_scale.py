"""SGBM and the depth path at the scale the benchmark runs them (-m gpu), pair by pair against the CPU oracle.

At 1920x1080 RGB, D=128, one pair's cost volume is 495 MB, so inside a batch the volume of pair 5 starts past 2^31
bytes and that of pair 9 past 2^32; C4 (4K gray, D=256) puts 3.96 GB in every pair volume, and 4K at D=512 holds more
than 2^31 elements in ONE volume.  Every offset that is per pair or per volume (images, volumes, band edge records,
chunk flags, winner-take-all state, the exact path's int32 volumes, remap's image groups, the speckle scratch) is only
checked here at these sizes.  Batches hold distinct pairs, so a kernel that reads a neighbour's data cannot pass.

Every comparison is bit-exact except depth (oracle_pipeline.compare: 1e-4 m, identical invalid sets).  The oracle
runs the sampled pairs of a case through sgbm_compute_batch, one thread per pair.  The largest cases allocate about
80 GB (get_depth_batch of 64 pairs), 127 GB (C4) and 160 GB (the bench child): one at a time, freed in between."""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bench  # noqa: E402
import calibrating_amd as ca  # noqa: E402
from calibrating_amd import synthetic  # noqa: E402
from oracle_pipeline import compare, oracle_get_depth  # noqa: E402
from test_gpu_int16_regime import CASES as INT16_CASES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = bench.parse([])                      # bench.py's defaults: 64 pairs of 1080p RGB, D=128, 2 in flight
H, W, D = BENCH.height, BENCH.width, BENCH.disparities
GiB4 = 2 ** 32


@pytest.fixture(autouse=True)
def _free_between_cases():
    """One large case at a time: handles and cached blocks of the previous case go back before the next starts."""
    _free()
    yield
    _free()


def _free():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _host(t, idx):
    return t[torch.as_tensor(idx, device=t.device)].cpu().numpy()


def _oracle(oracle, lefts, rights, p):
    """The oracle's disparity of every pair of the host stacks, one thread per pair (at most 16)."""
    return oracle.sgbm_compute_batch(lefts, rights, nthreads=min(16, len(lefts)), **p)


def _assert_pairs(got, want, idx, what):
    bad = {i: int((got[k] != want[k]).sum()) for k, i in enumerate(idx) if not np.array_equal(got[k], want[k])}
    assert not bad, "%s: pixels that differ, by pair: %s" % (what, bad)


def _volume_bytes(m):
    g = m.geometry()
    return H * g["width1"] * g["Dp"] * 2


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [2, 3], ids=["set0", "set1"])
def test_bench_workload_dumped_pairs_vs_oracle(oracle, tmp_path, steps):
    """bench.py as it runs for the headline number (a plain run: 64 pairs of 1080p RGB per launch, two handles on two
    streams), in a child process; the pairs it dumps of the last timed step against the oracle.  steps=2 ends on the
    first handle's set (seed 1234), steps=3 on the second's (seed 2234)."""
    free, total = torch.cuda.mem_get_info()
    assert total - free < 8e9, "the child needs ~160 GB of the device; %.1f GB are taken" % ((total - free) / 1e9)
    warmup = 1
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CAMD_BENCH_FORCE_DIST"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["config"]["pairs_per_gpu_per_step"] == 64 and line["config"]["batches_in_flight_per_gpu"] == 2
    idx = np.load(tmp_path / "pair_index.npy")
    disp = np.load(tmp_path / "disparity.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.round(idx))
    idx = idx.astype(np.int64).tolist()
    assert disp.shape == (len(idx), H, W)
    assert max(idx) >= 9, idx  # a pair whose volume starts past 2^32 bytes
    # step k (warm-up counted) ran on set k % 2; set i's inputs are seeded 1234 + 1000 * i (bench.main)
    seed = 1234 + 1000 * ((warmup + steps - 1) % 2)
    L, R = synthetic.rectified_batch_torch(seed, BENCH.batch, H, W, D, BENCH.channels, "cuda")
    lefts, rights = _host(L, idx), _host(R, idx)
    del L, R
    _free()
    want = _oracle(oracle, lefts, rights, bench.sgbm_params(BENCH))
    assert np.array_equal(disp, np.round(disp))
    _assert_pairs(disp.astype(np.int16), want, idx, "bench set seeded %d" % seed)


# ------------------------------------------------------------------------------------------------------------------
PAST_4G = [0, 4, 5, 8, 9]  # pair 5's volume starts past 2^31 bytes, pair 9's at 4.46 GB


@pytest.mark.parametrize("cn", [3, 1], ids=["rgb", "gray"])
def test_every_mode_past_4gib_of_volume(oracle, cn):
    """Ten distinct 1080p pairs, D=128, in every mode (gray: the LDS-tile store path of k_cost<1, 5>); RGB MODE_SGBM
    also through k_hsum + k_vsum and both aggregation paths.  Pairs on either side of 2^31 and 2^32 bytes of volume."""
    L, R = synthetic.rectified_batch_torch(4321 + cn, 10, H, W, D, cn, "cuda")
    lefts, rights = _host(L, PAST_4G), _host(R, PAST_4G)
    for mode in (ca.MODE_SGBM, ca.MODE_HH, ca.MODE_HH4, ca.MODE_SGBM_3WAY):
        p = dict(bench.sgbm_params(BENCH, channels=cn), mode=mode)
        runs = [(0, 0)]                                # (path, cost): AUTO
        if cn == 3 and mode == ca.MODE_SGBM:
            runs += [(0, 2), (1, 0), (2, 0)]           # split cost kernels; line scans; band passes
        got = {}
        for path, cost in runs:
            m = ca.StereoSGBM_create(**p)
            m.set_option("path", path).set_option("cost", cost)
            out = m.compute(L, R)
            m.status()
            assert 9 * _volume_bytes(m) >= GiB4
            got[path, cost] = _host(out, PAST_4G)
            del m, out
            _free()
        want = _oracle(oracle, lefts, rights, p)
        for (path, cost), g in got.items():
            _assert_pairs(g, want, PAST_4G, "cn %d mode %d path %d cost %d" % (cn, mode, path, cost))


# ------------------------------------------------------------------------------------------------------------------
def test_exact_path_at_a_far_volume_index(oracle):
    """A batch of ten 1080p pairs in which pairs 1 and 9 drift out of the int16 regime (16 lanes x 2 vectors, padded
    D = 200): they take the exact int path, which reads the flagged pair's volume at its offset -- pair 9's past
    2^32 bytes.  Both drift pairs and an ordinary one against the oracle, through the band passes and AUTO."""
    _, _, Dc, bs, cn, cap, P1, P2, minD = INT16_CASES[3]  # at 1080p instead of its 64 x 330
    p = dict(minDisparity=minD, numDisparities=Dc, blockSize=bs, P1=P1, P2=P2, preFilterCap=cap, uniquenessRatio=5,
             disp12MaxDiff=1, mode=ca.MODE_SGBM)
    L, R = synthetic.rectified_batch_torch(99, 10, H, W, Dc, cn, "cuda")
    for i, (split, seed) in ((1, (0.5, 1)), (9, (0.3, 2))):
        a, b = synthetic.drift_pair(H, W, cn, split=split, seed=seed)
        L[i], R[i] = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    idx = [1, 4, 9]
    got = {}
    for path in (2, 0):
        m = ca.StereoSGBM_create(**p)
        m.set_option("path", path)
        got[path] = _host(m.compute(L, R), idx)
        m.status()
        assert 9 * _volume_bytes(m) >= GiB4
        if path == 2:
            # the case cannot pass without the exact path: pair 9's C fell below P2 (fuzz_sgbm's rule)
            P2n = max(P2, P1 + 1)
            assert int(m.debug_volume("C", 9).min()) < P2n
        del m
        _free()
    want = _oracle(oracle, _host(L, idx), _host(R, idx), p)
    del L, R
    for path, g in got.items():
        _assert_pairs(g, want, idx, "path %d" % path)


# ------------------------------------------------------------------------------------------------------------------
C4_P = dict(minDisparity=0, numDisparities=256, blockSize=5, P1=8 * 25, P2=32 * 25, disp12MaxDiff=1, preFilterCap=0,
            uniquenessRatio=10, speckleWindowSize=0, speckleRange=0, mode=0)  # bench.config_c4


def test_c4_whole_frames_as_bench_measures_it(oracle):
    """C4 as bench.py --full measures it: 16 pairs of 3840x2160 gray, D=256, seed 7, one launch (3.96 GB of volume
    per pair, pair 2's starts at 7.9 GB); whole frames of pairs 0, 1, 2 and 15, AUTO and the forced band passes."""
    Hc, Wc, nb = 2160, 3840, 16
    L, R = synthetic.rectified_batch_torch(7, nb, Hc, Wc, C4_P["numDisparities"], 1, "cuda")
    idx = [0, 1, 2, 15]
    m = ca.StereoSGBM_create(**C4_P)
    out = torch.empty((nb, Hc, Wc), dtype=torch.int16, device="cuda")
    got = {}
    for path in (0, 2):
        m.set_option("path", path)
        out.fill_(-32768)  # (a sentinel no disparity takes: a path that skips rows cannot show the previous path's)
        m.compute(L, R, out=out)
        got[path] = _host(out, idx)
    m.status()
    g = m.geometry()
    assert 2 * Hc * g["width1"] * g["Dp"] * 2 > 7.9e9
    lefts, rights = _host(L, idx), _host(R, idx)
    del m, out, L, R
    _free()
    want = _oracle(oracle, lefts, rights, C4_P)
    for path, gp in got.items():
        _assert_pairs(gp, want, idx, "C4 path %d" % path)


def test_one_volume_past_2_31_elements(oracle):
    """3840x2160 gray at D=512, the largest D the library takes: 3.68e9 int16 elements in one pair's volume, past
    what an int element index reaches.  The whole frame, AUTO and the line scans."""
    Hc, Wc, Dc = 2160, 3840, 512
    p = dict(C4_P, numDisparities=Dc)
    L, R = synthetic.rectified_batch_torch(13, 1, Hc, Wc, Dc, 1, "cuda")
    got = {}
    for path in (0, 1):
        m = ca.StereoSGBM_create(**p)
        m.set_option("path", path)
        got[path] = m.compute(L, R).cpu().numpy()
        m.status()
        g = m.geometry()
        assert Hc * g["width1"] * g["D"] > 2 ** 31
        del m
        _free()
    want = _oracle(oracle, L.cpu().numpy(), R.cpu().numpy(), p)
    assert (want[0] >= 0).mean() > 0.3
    for path, gp in got.items():
        _assert_pairs(gp, want, [0], "D=512 path %d" % path)


# ------------------------------------------------------------------------------------------------------------------
def _depth_pairs(res, idx):
    return [{k: (v[i].cpu().numpy() if torch.is_tensor(v) else np.asarray(v[i])) for k, v in res.items()} for i in idx]


def _check_depth(oracle, stereo, cfg, got, pairs, idx, min_valid):
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(min(16, len(pairs))) as ex:  # (the oracle's C stages release the GIL)
        refs = list(ex.map(lambda ab: oracle_get_depth(oracle, stereo, cfg, *ab), pairs))
    for i, g, ref in zip(idx, got, refs):
        bad, _ = compare(g, ref)
        assert not bad, (i, bad)
        assert (ref["rectify_depth"] > 0).mean() > min_valid, i


def test_get_depth_batch_at_bench_scale(oracle):
    """bench.py --full's get_depth_batch: 64 pairs of 1080p RGB through the whole path (rectify x2, SGBM, depth,
    unrectify, undistort) on the synthetic rig.  Pairs 15 and 16 sit on either side of remap's 16-image group
    boundary, pair 63 at the end of every batched buffer."""
    L, R = synthetic.rectified_batch_torch(1234, BENCH.batch, H, W, D, 3, "cuda")
    stereo = ca.Stereo.load(synthetic.rig(W, H))
    cfg = dict(bench.sgbm_params(BENCH), max_size=max(W, H))
    stereo.set_stereo_matching(ca.SemiGlobalBlockMatching(cfg), max_depth=20.0)
    idx = [0, 15, 16, 63]
    got = _depth_pairs(stereo.get_depth_batch(L, R), idx)
    stereo.stereo_matching.stereo_sgbm.status()
    pairs = list(zip(_host(L, idx), _host(R, idx)))
    del L, R
    _free()
    _check_depth(oracle, stereo, cfg, got, pairs, idx, 0.1)


def test_c5_get_depth_batch_256_pairs(oracle):
    """C5 as bench.py --full measures it on the rendered scene: 640x480 RGB, D=64, LR check and speckle filter on,
    256 pairs per call.  Bench's batch repeats four scenes (pair i = scene i % 4): one pair of each at both ends of it.
    Then the same scenes rolled by a different number of columns in every pair, so that all 256 inputs differ and a
    kernel that reads another pair's data (four pairs back included) cannot pass: both ends and both sides of the
    middle."""
    Wc, Hc = 640, 480
    P = dict(minDisparity=0, numDisparities=64, blockSize=5, P1=8 * 3 * 25, P2=32 * 3 * 25, disp12MaxDiff=1,
             preFilterCap=0, uniquenessRatio=10, speckleWindowSize=100, speckleRange=2, mode=0)  # bench.config_c5
    rec = synthetic.rig(Wc, Hc)
    planes = [((0.3, 0.1, 1.0), 2.0), ((-0.2, 0.15, 1.0), 1.6), ((0.0, 0.0, 1.0), 2.5), ((0.1, -0.25, 1.0), 1.3)]
    scene = [synthetic.render_plane_pair(rec, n_, d_, seed=i)[:2] for i, (n_, d_) in enumerate(planes)]
    nb = 256
    stereo = ca.Stereo.load(rec)
    cfg = dict(P, max_size=max(Wc, Hc))
    stereo.set_stereo_matching(ca.SemiGlobalBlockMatching(cfg), max_depth=3.5)
    bench_pair = lambda i: scene[i % len(scene)]  # noqa: E731
    rolled_pair = lambda i: tuple(np.roll(im, 3 * (i // len(scene)), axis=1) for im in scene[i % len(scene)])  # noqa: E731
    for pair, idx in ((bench_pair, [0, 1, 2, 3, 252, 253, 254, 255]), (rolled_pair, [0, 127, 128, 255])):
        pairs = [pair(i) for i in range(nb)]
        B1 = torch.from_numpy(np.stack([a for a, _ in pairs])).cuda()
        B2 = torch.from_numpy(np.stack([b for _, b in pairs])).cuda()
        got = _depth_pairs(stereo.get_depth_batch(B1, B2), idx)
        stereo.stereo_matching.stereo_sgbm.status()
        del B1, B2
        _check_depth(oracle, stereo, cfg, got, [pairs[i] for i in idx], idx, 0.5)
