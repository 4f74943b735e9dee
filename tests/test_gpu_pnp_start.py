"""The start stage of every solver on the MI355X (-m gpu): ``camd_pnp_init`` and ``camd_calib_homography`` alone, driven
through ``_native.call`` with ``pnp.pack_points`` as calibrating_amd/pnp.py and calibrate.py drive them, into buffers
filled with a sentinel.  Against the exact fixture tests/golden/pnp_start_exact.npz within the bounds of
tests/golden/pnp_start_tolerance.json (8 x the NumPy restatement's own error, in units of 2^-52 kappa), and against
themselves bit for bit."""
import ctypes

import numpy as np
import pytest

# (the fixture's arrays are read-only, and nothing here writes to the tensors made from them)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

torch = pytest.importorskip("torch")

from calibrating_amd import _native, calibrate, pnp  # noqa: E402
from calibrating_amd._arrays import FLOAT_TYPES, K9, dist, dtype_name  # noqa: E402

import calibrate_ref  # noqa: E402
import pnp_start_cases as cases  # noqa: E402
import pnp_start_tolerance as tolerance  # noqa: E402

SENTINEL = -7.25
GUARD = 3  # rows of sentinel behind the last frame's
POSE_CASES = [n for n in cases.NAMES if cases.kind_of(n) != "homography"]
HOMOGRAPHY_CASES = [n for n in cases.NAMES if cases.kind_of(n) == "homography"]


@pytest.fixture(scope="module")
def fixture():
    return tolerance.fixture()


@pytest.fixture(scope="module")
def bound():
    return tolerance.load()["bound"]


def launch(entry, pts, dev, width, head, frames=None):
    """one call into a sentinel-filled buffer of ``frames + GUARD`` rows -> (frames, width) on the host; nothing is written
    behind the frames' rows"""
    frames = pts.frames if frames is None else frames
    out = torch.full((frames + GUARD, width), SENTINEL, dtype=torch.float64, device=dev)
    _native.call(entry, dev, ctypes.byref(pts), *head, out.data_ptr())
    out = out.cpu().numpy()
    assert (out[frames:] == SENTINEL).all(), "%s wrote behind frames x %d" % (entry, width)
    return out[:frames]


def init_args(K, D, planar, plane):
    Kf, (Dv, dptr, nd) = K9(K), dist(D if D is not None and len(D) else None)
    plane = np.ascontiguousarray(plane, np.float64)
    return (Kf.ctypes.data, dptr, nd, int(planar), plane.ctypes.data), (Kf, Dv, plane)


def pnp_init(obj, uv, K, D, planar, plane, counts=None):
    """``camd_pnp_init`` as pnp.solve_pnp_batch calls it -> (frames, 12)"""
    frames, lengths, shared = pnp.batch_layout(obj, uv, counts)
    pts, dev, alive = pnp.pack_points(obj, uv, lengths, shared)
    head, keep = init_args(K, D, planar, plane)
    return launch("camd_pnp_init", pts, dev, 12, head)


def homography(obj, uv, plane, counts=None):
    """``camd_calib_homography`` as calibrate.calibrate_camera calls it -> (frames, 9)"""
    frames, lengths, shared = pnp.batch_layout(obj, uv, counts)
    pts, dev, alive = pnp.pack_points(obj, uv, lengths, shared)
    plane = np.ascontiguousarray(plane, np.float64)
    return launch("camd_calib_homography", pts, dev, 9, (plane.ctypes.data,))


def start(c, obj=None, uv=None, counts=None):
    """a fixture case (or other rows under its camera and plane) through its entry point"""
    obj, uv = c["obj"] if obj is None else obj, c["uv"] if uv is None else uv
    if c["kind"] == "homography":
        return homography(obj, uv, c["plane"], counts)
    return pnp_init(obj, uv, c["K"], c["D"], c["kind"] == "planar", c["plane"], counts)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- against the exact fixture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POSE_CASES)
def test_start_pose_against_the_exact_reference(name, fixture, bound):
    c = fixture[name]
    pose = start(c)
    assert np.isfinite(pose).all(), name
    e = tolerance.pose_error(pose, c)
    print("%-34s pose error %.3f of a bound of %.3f (x 2^-52 kappa, kappa %.3g): |pose - exact| %.3e" %
          (name, e.max(), bound["pose"], c["kappa"].max(), np.abs(pose - c["pose"]).max()))
    assert e.max() <= bound["pose"], (name, e)
    if name in cases.OFF_ORIGIN:  # the sign, outright: every point in front of the camera, a proper rotation
        for p in pose:
            R, t = p[:9].reshape(3, 3), p[9:]
            assert ((c["obj"] @ R.T + t)[:, 2] > 0).all() and abs(np.linalg.det(R) - 1) < 1e-14, name


@pytest.mark.parametrize("name", HOMOGRAPHY_CASES)
def test_homography_against_the_exact_reference(name, fixture, bound):
    """H's scale and sign are unspecified: both sides at unit Frobenius norm, with the exact one's sign.  Then the host's
    follow-on: the start intrinsics of the GPU's homographies against those of the exact ones."""
    c = fixture[name]
    H = start(c)
    assert np.isfinite(H).all(), name
    e = tolerance.g_error(H, c)
    K0 = calibrate.initial_camera_matrix(H, tolerance.XY)
    want = calibrate_ref.initial_camera_matrix(c["G"].reshape(-1, 3, 3), tolerance.XY)
    k = tolerance.k0_error(K0, c)
    print("%-34s H error %.3f of a bound of %.3f, K0 error %.3f of %.3f (x 2^-52 kappa, kappa %.3g): fx %.9g (exact %.9g)" %
          (name, e.max(), bound["G/homography"], k, bound["K0"], c["kappa"].max(), K0[0, 0], want[0, 0]))
    assert e.max() <= bound["G/homography"], (name, e)
    assert k <= bound["K0"] and K0[0, 2] == want[0, 2] and K0[1, 2] == want[1, 2], (name, k)


# ---- bit for bit -------------------------------------------------------------------------------------------------------
BITS = ["planar-n65-f4-d12-noisy", "cloud-n65-f4-d12-noisy", "homography-n65-f3-noisy", "planar-tilted-n24-f3-d8-noisy"]


@pytest.mark.parametrize("name", BITS)
def test_a_frame_gets_the_same_bits_alone_and_anywhere_in_a_batch(name, fixture):
    c = fixture[name]
    whole = start(c)
    assert same(whole, start(c))                                     # two runs
    frames = len(whole)
    for f in range(frames):                                           # a frame alone
        assert same(start(c, uv=c["uv"][f:f + 1]), whole[f:f + 1]), f
    order = [(5 * i + 2) % frames for i in range(9)]                  # other waves, other workgroups
    moved = start(c, uv=np.ascontiguousarray(c["uv"][order]))
    assert same(moved, whole[order])


@pytest.mark.parametrize("name", BITS)
def test_layouts_of_the_same_values_give_the_same_bits(name, fixture):
    """shared object rows and the same rows per frame; float32 rows and their float64 copies; rows read in place from a
    wider array (strides 5 and 3) and the contiguous copy"""
    c = fixture[name]
    frames, n = c["uv"].shape[:2]
    whole = start(c)
    per_frame = np.ascontiguousarray(np.repeat(c["obj"][None], frames, 0))
    assert same(start(c, obj=per_frame), whole)
    obj32, uv32 = c["obj"].astype(np.float32), c["uv"].astype(np.float32)
    for o, u in ((obj32, c["uv"]), (c["obj"], uv32), (obj32, uv32), (per_frame.astype(np.float32), uv32)):
        assert same(start(c, obj=o, uv=u), start(c, obj=o.astype(np.float64), uv=u.astype(np.float64)))
    # noisy rows ARE float32 values, and so are the object rows: then every layout above is the whole fixture case
    if np.array_equal(uv32, c["uv"]):
        assert same(start(c, obj=obj32, uv=uv32), whole)
    for dtype in (np.float64, np.float32):
        wide_o = np.full((frames * n, 5), np.nan, dtype)
        wide_u = np.full((frames * n, 3), np.nan, dtype)
        wide_o[:, :3], wide_u[:, :2] = per_frame.reshape(-1, 3), c["uv"].reshape(-1, 2)
        o, u = torch.from_numpy(wide_o).cuda(), torch.from_numpy(wide_u).cuda()
        begin = torch.arange(0, frames * n + 1, n, dtype=torch.int64, device=o.device)
        pts = _native.PnpPoints(o.data_ptr(), u.data_ptr(), begin.data_ptr(), frames * n, frames * n, FLOAT_TYPES[dtype_name(o)],
                                FLOAT_TYPES[dtype_name(u)], 5, 3, 0, frames)
        if c["kind"] == "homography":
            got = launch("camd_calib_homography", pts, o.device, 9, (c["plane"].ctypes.data,))
        else:
            head, keep = init_args(c["K"], c["D"], c["kind"] == "planar", c["plane"])
            got = launch("camd_pnp_init", pts, o.device, 12, head)
        assert same(got, start(c, obj=wide_o[:, :3].astype(np.float64).reshape(frames, n, 3),
                               uv=wide_u[:, :2].astype(np.float64).reshape(frames, n, 2))), dtype


def ragged_rows(fixture, kind, names, camera):
    """[(obj, uv)]: the first frame of each named case, and the case whose camera and plane the batch runs under"""
    return [(fixture[n]["obj"], fixture[n]["uv"][0]) for n in names], fixture[camera]


@pytest.mark.parametrize("kind", ["planar", "cloud", "homography"])
def test_a_ragged_batch_and_each_frame_alone(kind, fixture):
    """frames of 4 (6 in space), 65 and 129 points in one call: each gets the bits it gets alone"""
    names = {"planar": ["planar-n4-f9-d0", "planar-n65-f4-d12-noisy", "planar-n129-f1-d0-noisy", "planar-n5-f5-d4-noisy"],
             "cloud": ["cloud-n6-f9-d0", "cloud-n65-f4-d12-noisy", "cloud-n129-f1-d0-noisy", "cloud-n7-f5-d4-noisy"],
             "homography": ["homography-n4-f9", "homography-n65-f3-noisy", "homography-n129-f1-noisy", "homography-n5-f5-noisy"]}[kind]
    rows, c = ragged_rows(fixture, kind, names, names[1])
    rows = rows + rows[:2]  # six frames: a second workgroup
    whole = start(c, np.concatenate([o for o, _ in rows]), np.concatenate([u for _, u in rows]), [len(o) for o, _ in rows])
    assert np.isfinite(whole).all()
    for f, (o, u) in enumerate(rows):
        assert same(start(c, o, u[None]), whole[f:f + 1]), f
    assert same(whole[:2], whole[4:])


# ---- frames that cannot be started ---------------------------------------------------------------------------------------
def spoilt(rows, value, where):
    o, u = (a.copy() for a in rows)
    (o if where == "obj" else u)[len(o) // 2, 1] = value
    return o, u


@pytest.mark.parametrize("kind", ["planar", "cloud", "homography"])
def test_bad_frames_get_nan_and_their_neighbours_keep_their_bits(kind, fixture):
    """too few points, a NaN or an infinite coordinate, all points identical: NaN in all 12 (or 9) places; a frame of
    collinear points comes back all finite or all NaN; the good frames between them are what they are alone"""
    few = 5 if kind == "cloud" else 3
    names = {"planar": ["planar-n65-f4-d12-noisy", "planar-n4-f9-d0", "planar-n129-f1-d0-noisy"],
             "cloud": ["cloud-n65-f4-d12-noisy", "cloud-n6-f9-d0", "cloud-n129-f1-d0-noisy"],
             "homography": ["homography-n65-f3-noisy", "homography-n4-f9", "homography-n129-f1-noisy"]}[kind]
    good, c = ragged_rows(fixture, kind, names, names[0])
    o65, u65 = good[0]
    line = (np.outer(np.linspace(-1, 1, 9), [0.03, 0.02, 0.0]), np.outer(np.linspace(-1, 1, 9), [90.0, 60.0]) + c["K"][:2, 2])
    rows = [good[0],
            (o65[:few], u65[:few]),                                     # 1: too few
            good[1],
            spoilt(good[0], np.nan, "uv"),                             # 3
            spoilt(good[0], np.inf, "obj"),                            # 4
            spoilt(good[2], -np.inf, "uv"),                            # 5
            spoilt(good[2], np.nan, "obj"),                            # 6
            good[2],
            (np.repeat(o65[:1], 7, 0), np.repeat(u65[:1], 7, 0)),      # 8: all points identical
            line,                                                       # 9: collinear
            good[1]]
    bad, either, fine = (1, 3, 4, 5, 6, 8), 9, (0, 2, 7, 10)
    with np.errstate(all="ignore"):
        whole = start(c, np.concatenate([o for o, _ in rows]), np.concatenate([u for _, u in rows]), [len(o) for o, _ in rows])
    for f in bad:
        assert np.isnan(whole[f]).all(), (f, whole[f])
    assert np.isnan(whole[either]).all() or np.isfinite(whole[either]).all(), whole[either]
    for f in fine:
        alone = start(c, rows[f][0], rows[f][1][None])
        assert np.isfinite(alone).all() and same(alone, whole[f:f + 1]), f


@pytest.mark.parametrize("kind", ["planar", "cloud", "homography"])
def test_a_range_outside_the_rows_is_not_read(kind, fixture):
    """``start`` ranges that leave the image rows, leave the object rows, or run backwards: NaN, and the good frames keep
    their bits"""
    c = fixture[{"planar": "planar-n65-f4-d12-noisy", "cloud": "cloud-n65-f4-d12-noisy", "homography": "homography-n65-f3-noisy"}[kind]]
    n = c["uv"].shape[1]
    whole = start(c, uv=c["uv"][:3])
    o = torch.from_numpy(np.ascontiguousarray(np.repeat(c["obj"][None], 3, 0)).reshape(-1, 3)).cuda()
    u = torch.from_numpy(np.ascontiguousarray(c["uv"][:3]).reshape(-1, 2)).cuda()
    head, keep = init_args(c["K"], c["D"], kind == "planar", c["plane"])  # (keep: the host arrays the addresses point into)
    if kind == "homography":
        head = (keep[2].ctypes.data,)
    entry, width = ("camd_calib_homography", 9) if kind == "homography" else ("camd_pnp_init", 12)
    for begin, obj_rows, bad in (([0, n, 2 * n, 3 * n + 1], 3 * n, [2]),     # one row beyond the image rows
                                 ([0, n, 2 * n, 3 * n], 3 * n - 1, [2]),    # the object rows end one row early
                                 ([0, n, n - 8, 2 * n], 3 * n, [1]),        # a range that runs backwards
                                 ([-n, 0, n, 2 * n], 3 * n, [0])):          # a range that begins before the rows
        s = torch.tensor(begin, dtype=torch.int64, device=o.device)
        pts = _native.PnpPoints(o.data_ptr(), u.data_ptr(), s.data_ptr(), obj_rows, 3 * n, FLOAT_TYPES["float64"], FLOAT_TYPES["float64"],
                                3, 2, 0, 3)
        got = launch(entry, pts, o.device, width, head)
        for f in range(3):
            if f in bad:
                assert np.isnan(got[f]).all(), (begin, f)
            elif begin[f] == f * n and begin[f + 1] == (f + 1) * n:
                assert same(got[f], whole[f]), (begin, f)


def test_no_frames_launch_nothing():
    pts = _native.PnpPoints(0, 0, 0, 0, 0, FLOAT_TYPES["float64"], FLOAT_TYPES["float64"], 3, 2, 0, 0)
    dev = torch.device("cuda", torch.cuda.current_device())
    head, keep = init_args(np.eye(3), None, True, np.eye(3))
    assert launch("camd_pnp_init", pts, dev, 12, head).shape == (0, 12)  # (returns OK, or _native.call raises)
    assert launch("camd_calib_homography", pts, dev, 9, (keep[2].ctypes.data,)).shape == (0, 9)


# ---- the public call uses this stage and nothing else ------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in POSE_CASES if "noisy" in n])
def test_solve_pnp_batch_starts_from_this_stage(name, fixture):
    """without T0 the public call gives, bit for bit, what it gives with T0 = this stage's output"""
    c = fixture[name]
    D = c["D"] if len(c["D"]) else None
    T0 = pnp.poses_to_T(torch.from_numpy(start(c))).numpy()
    a = pnp.solve_pnp_batch(c["obj"], c["uv"], c["K"], D)
    b = pnp.solve_pnp_batch(c["obj"], c["uv"], c["K"], D, T0=T0)
    assert (a["status"] == 0).all(), (name, a["status"])
    for k in ("T", "reprojection_error", "iterations", "status"):
        assert same(a[k], b[k]), (name, k)
