"""Inputs of the reconstruction tests (tests/test_reconstruction_cpu.py, tests/test_gpu_reconstruction.py), of the fixture
maker (tests/golden/make_reconstruction_golden.py) and of tools/gpu_reconstruction_time.py.  Only DATA lives here: a seeded
scene generator and the list of cases; everything is regenerated from seeds on both sides of a comparison.

The scene.  N cameras share one K (f = 1.1 w, principal point in the centre).  Their poses are a few degrees and a few
tenths of a unit apart and they look at the surface z = 3 + 0.4 sin(1.7 x) + 0.3 cos(1.3 y).  A pixel's depth is found by
fixed-point iteration along its ray; the dense flow a -> b is where the pixel's surface point lands in view b minus where
it is in view a (float32); ``common_fov_mask`` marks the pixels that land inside image b."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_reconstruction.npz")
HW = (48, 64)
SEED_SEARCH = 60  # the maker tries this many seeds from a case's first seed on for one that meets the case's conditions

# name -> views, first seed, and what the case is there for (the maker asserts it and stores the seed it took)
CASES = {
    "one_triple": dict(views=3, seed=1),
    "ten_triples": dict(views=5, seed=2),
    "rerooted": dict(views=6, seed=9, rerooted=True),
    "two_sizes": dict(views=4, seed=4, last_hw=(40, 56)),
    "deferred_seed": dict(views=6, seed=0, reference_raises="KeyError"),
    "two_groups": dict(views=6, seed=5, groups=((0, 1, 2), (3, 4, 5))),
}
REFERENCE_SUCCEEDS = ("one_triple", "ten_triples", "rerooted", "two_sizes")


def _rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def surface(x, y):
    return 3 + 0.4 * np.sin(1.7 * x) + 0.3 * np.cos(1.3 * y)


def intrinsics(hw):
    h, w = hw
    return np.array([[1.1 * w, 0, w / 2], [0, 1.1 * w, h / 2], [0, 0, 1.0]])


def poses(n, rng):
    """Camera-to-world 4x4 of n cameras: rotations of a few degrees, centres a few tenths of a unit apart."""
    out = []
    for _ in range(n):
        T = np.eye(4)
        T[:3, :3] = _rodrigues(rng.uniform(-0.07, 0.07, 3))
        T[:3, 3] = rng.uniform(-0.35, 0.35, 3) * (1, 1, 0.3)
        out.append(T)
    return out


def surface_points(K, T, hw, iters=40):
    """World points (h, w, 3) the pixel centres (x + 0.5, y + 0.5) of a camera see on the surface."""
    h, w = hw
    ys, xs = np.mgrid[:h, :w]
    rays = np.stack([xs + 0.5, ys + 0.5, np.ones_like(xs, float)], -1) @ np.linalg.inv(K).T @ T[:3, :3].T
    zc = np.full((h, w), 3.0)
    for _ in range(iters):
        P = T[:3, 3] + rays * zc[..., None]
        zc = (surface(P[..., 0], P[..., 1]) - T[2, 3]) / rays[..., 2]
    return T[:3, 3] + rays * zc[..., None]


def flow_between(P, Ka, Kb, Tb, hw_b):
    """(flow_abs float32 (h, w, 2), common_fov_mask) of view a's surface points P seen by view b."""
    h, w = P.shape[:2]
    ys, xs = np.mgrid[:h, :w]
    Xb = (P - Tb[:3, 3]) @ Tb[:3, :3]  # R^T (P - c)
    p = Xb @ Kb.T
    uv = p[..., :2] / p[..., 2:]
    flow = (uv - np.stack([xs + 0.5, ys + 0.5], -1)).astype(np.float32)
    mask = (Xb[..., 2] > 0) & (uv[..., 0] >= 0) & (uv[..., 0] < hw_b[1]) & (uv[..., 1] >= 0) & (uv[..., 1] < hw_b[0])
    return flow, mask


def scene(views, seed, hw=HW, last_hw=None, groups=None):
    """(viewds, flowds, true camera-to-world poses).  ``viewds[k]``: K and an ``img`` of the view's size; ``flowds[(a, b)]``:
    flow_abs and common_fov_mask for every ordered pair (within a group only, when ``groups`` is given)."""
    rng = np.random.default_rng(seed)
    Ts = poses(views, rng)
    hws = [hw] * views
    if last_hw is not None:
        hws[-1] = tuple(last_hw)
    Ks = [intrinsics(s) for s in hws]
    viewds = {k: dict(K=Ks[k], img=np.zeros(hws[k] + (3,), np.uint8)) for k in range(views)}
    Ps = [surface_points(Ks[k], Ts[k], hws[k]) for k in range(views)]
    flowds = {}
    for a in range(views):
        for b in range(views):
            if a == b or (groups is not None and not any(a in g and b in g for g in groups)):
                continue
            flow, mask = flow_between(Ps[a], Ks[a], Ks[b], Ts[b], hws[b])
            flowds[(a, b)] = dict(flow_abs=flow, common_fov_mask=mask)
    return viewds, flowds, Ts


def case(name, seed=None):
    c = CASES[name]
    return scene(c["views"], c["seed"] if seed is None else seed, last_hw=c.get("last_hw"), groups=c.get("groups"))


def fresh(viewds):
    """The views without what a reconstruction left in them."""
    return {k: {kk: vv for kk, vv in v.items() if kk not in ("T_re", "uvzis")} for k, v in viewds.items()}


def rotation_error(T_re, Ts):
    """Largest |R_re(0 -> k) - R_true(0 -> k)| entry over the views: rotations relative to view 0."""
    worst = 0.0
    for k in T_re:
        got = T_re[0][:3, :3].T @ T_re[k][:3, :3]
        want = Ts[0][:3, :3].T @ Ts[k][:3, :3]
        worst = max(worst, float(np.abs(got - want).max()))
    return worst


def triple_name(set3):
    return ",".join(str(v) for v in sorted(set3))


def load_fixture():
    if not os.path.exists(FIXTURE):
        return None
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
