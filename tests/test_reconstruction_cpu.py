"""ReconstructionExtrinsics without a GPU: the argument errors that are raised before the device is touched, the path
planning (calibrating_amd.reconstruction_epipolar_geometry.plan_triples / plan_propagation, which take counts only)
against what the reference's own class decided (tests/golden/reference_reconstruction.npz, made by
tests/golden/make_reconstruction_golden.py), and the scene generator's own properties."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import reference_cases as rc  # noqa: E402
import reconstruction_cases as rcc  # noqa: E402

import calibrating_amd as ca  # noqa: E402
from calibrating_amd import reconstruction_epipolar_geometry as reg  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    f = rcc.load_fixture()
    assert f is not None, "tests/golden/reference_reconstruction.npz is missing (python tests/golden/make_reconstruction_golden.py)"
    return f


def _set3(name):
    return frozenset(int(v) for v in str(name).split(","))


def planned_from_fixture(fx, name):
    """[(set3, idx_sorted, not_include_uvsn, count)] of the triples that match, from the recorded counts alone."""
    p = name + "/"
    out = []
    for nm, idx_sorted, not_include, count in zip(fx[p + "planned"], fx[p + "planned_idx_sorted"], fx[p + "planned_not_include"],
                                                  fx[p + "planned_counts"]):
        set3 = _set3(nm)
        if count >= 10:
            out.append((set3, [int(v) for v in idx_sorted], dict(zip(sorted(set3), (int(v) for v in not_include))), int(count)))
    return out


# ---- arguments ---------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_the_device():
    K = rcc.intrinsics(rcc.HW)
    size = dict(K=K, xy=(64, 48))
    pair = {frozenset((0, 1)): dict(uvs_i=np.zeros((20, 2)), uvs_j=np.zeros((20, 2)))}
    with pytest.raises(ValueError, match="img.*xy.*mask"):
        ca.ReconstructionExtrinsics({0: dict(size), 1: dict(K=K), 2: dict(size)}, set2ds=pair)
    with pytest.raises(KeyError, match="key 0"):
        ca.ReconstructionExtrinsics({1: dict(size), 2: dict(size), 3: dict(size)}, set2ds=pair)
    with pytest.raises(ValueError, match="at least 3 views"):
        ca.ReconstructionExtrinsics({0: dict(size), 1: dict(size)}, set2ds=pair)
    with pytest.raises(ValueError, match="triple_stage"):
        ca.ReconstructionExtrinsics({0: dict(size), 1: dict(size), 2: dict(size)}, set2ds=pair, cfg=dict(triple_stage="fast"))
    with pytest.raises(ValueError, match="set2ds or flowds"):
        ca.ReconstructionExtrinsics({0: dict(size), 1: dict(size), 2: dict(size)})
    # the size comes from img (its shape only), xy or mask, in that order
    assert reg.view_xy(dict(img=np.zeros((48, 64, 3), np.uint8), xy=(1, 2))) == (64, 48)
    assert reg.view_xy(dict(xy=[64, 48], mask=np.zeros((3, 4), bool))) == (64, 48)
    assert reg.view_xy(dict(mask=np.zeros((48, 64), bool))) == (64, 48)
    assert ca.ReconstructionExtrinsics.build_set2ds_by_flowds is ca.build_set2ds_by_flowds


# ---- planning against the reference's decisions ------------------------------------------------------------------------
@pytest.mark.parametrize("name", rcc.REFERENCE_SUCCEEDS)
def test_planning_from_counts_equals_the_reference(fx, name):
    p = name + "/"
    views = list(range(rcc.CASES[name]["views"]))
    triples = planned_from_fixture(fx, name)
    asked = []
    plan = reg.plan_propagation(views, triples, lambda set3, order: asked.append((set3, order)) or True)
    assert sorted(plan["seed"]) == fx[p + "seed3"].tolist()
    assert [[i] + sorted(s) for i, s in plan["propagate_path"]] == fx[p + "propagate_path"].tolist()
    assert sorted(rcc.triple_name(s) for s in plan["rerooted"]) == sorted(str(s) for s in fx[p + "rerooted"])
    assert [s for s, _ in asked] == plan["rerooted"]
    final = dict(zip((str(s) for s in fx[p + "triples"]), fx[p + "idx_sorted"].tolist()))
    for set3, order in asked:  # the new main view is the reference's
        assert final[rcc.triple_name(set3)] == order
    if name == "rerooted":
        assert plan["rerooted"], "the case is there for a re-rooted triple"


@pytest.mark.parametrize("name", rcc.REFERENCE_SUCCEEDS + ("deferred_seed", "two_groups"))
def test_plan_triples_equals_the_recorded_order(fx, name):
    p = name + "/"
    sizes = {}
    for nm, not_include in zip(fx[p + "planned"], fx[p + "planned_not_include"]):
        set3 = _set3(nm)
        for idx, n in zip(sorted(set3), not_include):
            sizes[set3 - {idx}] = int(n)
    got = reg.plan_triples(list(range(rcc.CASES[name]["views"])), {k: v for k, v in sizes.items() if v})
    assert [rcc.triple_name(s) for s, _, _ in got] == [str(s) for s in fx[p + "planned"]]
    assert [o for _, o, _ in got] == fx[p + "planned_idx_sorted"].tolist()


def test_deferred_seed_and_two_groups_plans(fx):
    assert str(fx["deferred_seed/raises"]) == "KeyError: 'T_re'"  # what the reference does with this case
    plan = reg.plan_propagation(list(range(6)), planned_from_fixture(fx, "deferred_seed"), lambda s, o: True)
    reached = set(plan["seed"]).union(*(s for _, s in plan["propagate_path"]))
    assert len(reached) >= 6
    # the reference's loop would meet a triple whose main view is the seed's second view before that view has a pose
    order = {t[0]: t[1] for t in planned_from_fixture(fx, "deferred_seed")}
    for s, o in order.items():
        if s in plan["rerooted"]:
            order[s] = o[1:] + o[:1]
    second = order[plan["seed"]][1]
    assert any(order[s][0] == second for _, s in plan["propagate_path"])
    assert str(fx["two_groups/raises"]) != ""
    with pytest.raises(ValueError, match=r"3 views are not reached.*\[(0, 1, 2|3, 4, 5)\]$"):
        reg.plan_propagation(list(range(6)), planned_from_fixture(fx, "two_groups"), lambda s, o: True)
    # a triple with two empty pairs is skipped, the triples after it are kept (the reference stops there)
    names = [str(s) for s in fx["two_groups/planned"]]
    assert names == ["0,1,2", "3,4,5"]
    with pytest.raises(ValueError, match="no triple"):
        reg.plan_propagation([0, 1, 2], [])


# ---- the generator -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rcc.CASES))
def test_generator_gives_what_the_fixture_was_made_from(fx, name):
    viewds, flowds, Ts = rcc.case(name, int(fx[name + "/seed"]))
    assert "".join(rc.sha(flowds[k]["flow_abs"]) + rc.sha(flowds[k]["common_fov_mask"]) for k in sorted(flowds)) == str(fx[name + "/in_sha"])
    c = rcc.CASES[name]
    assert len(viewds) == len(Ts) == c["views"]
    pairs = c["views"] * (c["views"] - 1) if "groups" not in c else sum(len(g) * (len(g) - 1) for g in c["groups"])
    assert len(flowds) == pairs
    for (a, b), d in flowds.items():
        h, w = viewds[a]["img"].shape[:2]
        assert d["flow_abs"].dtype == np.float32 and d["flow_abs"].shape == (h, w, 2)
        assert d["common_fov_mask"].dtype == bool and d["common_fov_mask"].shape == (h, w) and d["common_fov_mask"].sum() > 10


def test_generator_geometry():
    viewds, flowds, Ts = rcc.case("two_sizes")
    assert viewds[3]["img"].shape == (40, 56, 3) and viewds[0]["img"].shape == (48, 64, 3)
    assert viewds[3]["K"][0, 0] == 1.1 * 56 and viewds[0]["K"][0, 2] == 32 and viewds[0]["K"][1, 2] == 24
    for k in (0, 3):  # the fixed-point iteration has converged: the points lie on the surface and on their rays
        hw = viewds[k]["img"].shape[:2]
        P = rcc.surface_points(viewds[k]["K"], Ts[k], hw)
        assert np.abs(P[..., 2] - rcc.surface(P[..., 0], P[..., 1])).max() < 1e-12
        p = ((P - Ts[k][:3, 3]) @ Ts[k][:3, :3]) @ viewds[k]["K"].T
        ys, xs = np.mgrid[:hw[0], :hw[1]]
        assert np.abs(p[..., 0] / p[..., 2] - (xs + 0.5)).max() < 1e-9 and np.abs(p[..., 1] / p[..., 2] - (ys + 0.5)).max() < 1e-9
    # the mask marks exactly the pixels that land inside the other image, and the flow there leads back: following 0 -> 3
    # and then 3 -> 0 (nearest pixel of view 3) returns within the flow's variation over one pixel
    f, m = flowds[(0, 3)]["flow_abs"], flowds[(0, 3)]["common_fov_mask"]
    ys, xs = np.mgrid[:48, :64]
    u, v = xs + 0.5 + f[..., 0], ys + 0.5 + f[..., 1]
    assert np.array_equal(m, (u >= 0) & (u < 56) & (v >= 0) & (v < 40))
    back = flowds[(3, 0)]["flow_abs"][np.floor(v[m]).astype(int), np.floor(u[m]).astype(int)]
    assert np.abs(back + f[m]).max() < 1.5
    # poses: a few degrees, a few tenths of a unit
    for T in Ts:
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14) and np.abs(T[:3, 3]).max() <= 0.35
        assert np.degrees(np.arccos((np.trace(T[:3, :3]) - 1) / 2)) < 8
    assert rcc.rotation_error({k: T for k, T in enumerate(Ts)}, Ts) == 0
