"""Catalogue and fuzz generator of the ``Stereo.distort_depth`` tests.  DATA and pure NumPy only (no GPU, no reference):
tests/golden/make_distort_depth_golden.py feeds the catalogue to the reference's own Python, the CPU and GPU tests feed
it to ``calibrating_amd`` and to the restatement (tests/distort_depth_ref.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

from calibrating_amd import synthetic  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "reference_distort_depth.npz")

# name -> camera-1 image size and distortion.  K is synthetic.rig's (principal point off centre by (+3.3, -2.1)).
RIGS = {
    "barrel": dict(wh=(320, 240), D=[-0.12, 0.05, 1e-3, -5e-4, 0.01]),   # synthetic.rig's own camera 1
    "zero": dict(wh=(160, 120), D=[0.0, 0.0, 0.0, 0.0, 0.0]),             # not the identity table: float32 hand-overs
    "rational12": dict(wh=(200, 150), D=[-0.10, 0.03, 5e-4, -3e-4, 0.005, 0.01, -0.002, 0.001, 2e-4, -1e-4, 1e-4, 5e-5]),
    # pincushion: targets beyond both edges; the reference raises IndexError (and would wrap the negative ones)
    "pincushion_out": dict(wh=(320, 240), D=[0.08, -0.03, -8e-4, 6e-4, 0.002]),
}
GOOD_RIGS = ("barrel", "zero", "rational12")
OUT_RIG = "pincushion_out"

# the full call: Stereo.load -> set_stereo_matching -> get_depth(return_distort_depth=True) on the barrel rig, with the
# reference's default plugin (its SemiGlobalBlockMatching reads nothing but max_size from cfg: stereo_matching.py:27-58)
GET_DEPTH = dict(rig="barrel", cfg={}, setm=dict(max_depth=3.5), scene=((0.2, 0.1, 1.0), 2.0, 3))


def rig_record(name, spelled=False):
    """The rig as ``Stereo.load`` takes it: synthetic.rig at the case's size with camera 1's distortion replaced.
    ``spelled``: intrinsics as fx / fy / cx / cy, the spelling ``Cam.dump`` writes and both packages load."""
    spec = RIGS[name]
    rec = synthetic.rig(*spec["wh"])
    rec["cam1"]["D"] = [list(spec["D"])]
    if spelled:
        for cam in (rec["cam1"], rec["cam2"]):
            K = cam.pop("K")
            cam.update(fx=K[0][0], fy=K[1][1], cx=K[0][2], cy=K[1][2])
    return rec


def camera(name):
    """(K float64 (3, 3), D list, (w, h)) of camera 1."""
    rec = rig_record(name)
    return np.array(rec["cam1"]["K"], np.float64), list(RIGS[name]["D"]), tuple(RIGS[name]["wh"])


def depth_input(name, dtype, seed=0):
    """A depth image of the rig's size with holes (zeros), values exact in float32 and float64 alike."""
    w, h = RIGS[name]["wh"]
    rng = np.random.default_rng(1000 + seed)
    z = rng.integers(1, 1 << 8, (h, w)).astype(np.float64) / 8.0  # (few distinct values: the fixture stays small)
    z[rng.random((h, w)) < 0.15] = 0
    return z.astype(dtype)


def index_probe(name):
    """A float64 'depth' whose value at source pixel i is i + 1: what ``distort_depth`` makes of it, minus 1, is the
    source-index table itself (-1 = hole) -- read off the reference's own code without touching it."""
    w, h = RIGS[name]["wh"]
    return np.arange(1, w * h + 1, dtype=np.float64).reshape(h, w)


def scene_images():
    rec = rig_record(GET_DEPTH["rig"])
    normal, distance, seed = GET_DEPTH["scene"]
    return synthetic.render_plane_pair(rec, normal, distance, seed=seed)[:2]


def load_fixture():
    if not os.path.exists(FIXTURE):
        return None
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ---- fuzz --------------------------------------------------------------------------------------------------------
FUZZ_SEED, FUZZ_CASES = 20261016, 40
FUZZ_MAX_REFUSED = 0.25  # at most a quarter of the committed slice may be rigs the product has to refuse


def gen_case(seed, case):
    """One seeded rig: odd width, w * h not a multiple of 256, principal point off centre, 5 / 8 / 12 coefficients,
    barrel-dominant (k1 <= 0) with small higher-order, tangential and thin-prism terms."""
    rng = np.random.default_rng([seed, case])
    w = 2 * int(rng.integers(16, 200)) + 1
    h = int(rng.integers(17, 300))
    if (w * h) % 256 == 0:
        h += 1
    fx = w * rng.uniform(0.6, 1.2)
    fy = fx * rng.uniform(0.97, 1.03)
    cx = w / 2 + rng.choice([-1, 1]) * rng.uniform(0.01, 0.08) * w  # off centre by 1 .. 8 % of the side
    cy = h / 2 + rng.choice([-1, 1]) * rng.uniform(0.01, 0.08) * h
    nd = int(rng.choice([5, 8, 12]))
    D = [-rng.uniform(0, 0.25), rng.uniform(-0.05, 0.05), rng.uniform(-1e-3, 1e-3), rng.uniform(-1e-3, 1e-3),
         rng.uniform(-0.01, 0.01)]
    if nd >= 8:
        D += list(rng.uniform(-0.02, 0.02, 3))
    if nd == 12:
        D += list(rng.uniform(-5e-4, 5e-4, 4))
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    return dict(case=case, w=w, h=h, K=K, D=[float(v) for v in D],
                dtype=np.float32 if rng.integers(0, 2) else np.float64, batch=int(rng.choice([1, 1, 2, 3])),
                depth_seed=int(rng.integers(0, 1 << 30)))


def case_depth(c):
    rng = np.random.default_rng(c["depth_seed"])
    shape = (c["h"], c["w"]) if c["batch"] == 1 else (c["batch"], c["h"], c["w"])
    z = rng.integers(1, 1 << 20, shape).astype(np.float64) / 1024.0
    z[rng.random(shape) < 0.1] = 0
    return z.astype(c["dtype"])


def fuzz_on_gpu(seed=FUZZ_SEED, cases=FUZZ_CASES, log=None):
    """The runner: every case's table and gather against the restatement, bit for bit; a case whose rig leaves the image
    must be refused (IndexError) by the product too.  -> dict(cases, refused, mismatches=[...])."""
    import torch
    import distort_depth_ref as ref
    from calibrating_amd import imgproc
    refused, bad = 0, []
    for i in range(cases):
        c = gen_case(seed, i)
        size = (c["w"], c["h"])
        st = ref.target_stats(c["K"], c["D"], *size)
        if st["n_out"]:
            refused += 1
            try:
                imgproc.distort_index_map(c["K"], c["D"], size)
                bad.append("case %d: %d targets outside %s and the product did not refuse" % (i, st["n_out"], size))
            except IndexError as e:
                if "%d of %d" % (st["n_out"], c["w"] * c["h"]) not in str(e):
                    bad.append("case %d: refused with other counts than %s: %s" % (i, st, e))
            continue
        want_idx = ref.index_map_unique(c["K"], c["D"], *size)
        idx = imgproc.distort_index_map(c["K"], c["D"], size)
        if not np.array_equal(idx.cpu().numpy(), want_idx):
            bad.append("case %d %s nD=%d: %d table entries differ" % (i, size, len(c["D"]),
                                                                       (idx.cpu().numpy() != want_idx).sum()))
            continue
        z = case_depth(c)
        got = imgproc.distort_depth(torch.from_numpy(z).cuda(), idx).cpu().numpy()
        want = ref.gather(z, want_idx)
        if got.dtype != want.dtype or got.shape != want.shape or got.tobytes() != want.tobytes():
            bad.append("case %d %s %s batch %d: gather differs" % (i, size, z.dtype, c["batch"]))
        if log:
            log("case %d %s nD=%d %s batch %d ok" % (i, size, len(c["D"]), z.dtype, c["batch"]))
    return dict(cases=cases, refused=refused, mismatches=bad)
