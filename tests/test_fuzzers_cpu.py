"""Without a GPU: the case generators of the fuzzers around SGBM (tests/fuzzers.py, gen_*) reach every branch floor
their GPU slices demand, the NumPy model of the fixed-point remap is checked against the oracle and by hand, the
NumPy composition behind camd_disp16_resized_to_depth against the oracle's C, and compare() sees the sign of zero."""
import numpy as np
import pytest

import fuzzers
import np_fixed_remap
from oracle_pipeline import compare, disparity_to_depth, prepared_disparity, resized_disparity_to_depth, same_bits


@pytest.mark.parametrize("name", sorted(fuzzers.POST_SLICES))
def test_generators_reach_the_slice_floors(name):
    n, seeds, floors = fuzzers.POST_SLICES[name]
    gen = fuzzers.POST_FUZZERS[name][0]
    total = {}
    for seed in seeds:
        for case in range(n):
            for b in gen(seed, case)["branches"]:
                total[b] = total.get(b, 0) + 1
    short = {b: (total.get(b, 0), need) for b, need in floors.items() if total.get(b, 0) < need}
    assert not short, short


@pytest.mark.parametrize("name", sorted(fuzzers.POST_SLICES))
def test_generators_are_pure_and_slots_distinct(name):
    gen = fuzzers.POST_FUZZERS[name][0]
    for case in range(12):
        a, b = gen(7, case), gen(7, case)
        assert a["branches"] == b["branches"]
        for k, v in a.items():
            if isinstance(v, np.ndarray):
                assert same_bits(v, b[k]), (case, k)
        stack = a.get("src", a.get("imgs", a.get("disp16", a.get("depth"))))
        if isinstance(stack, np.ndarray) and name != "tables" and len(stack) > 1 and stack[1].size > 4:
            assert not np.array_equal(stack[0], stack[1]), (case, "batch slots 0 and 1 hold the same content")


def test_group_rule_matches_the_library():
    """images_per_group restates remap.hip / depth.hip: all images (up to 16) per workgroup while the grid fills."""
    assert fuzzers.images_per_group(2 * 1024, 17) == 16
    assert fuzzers.images_per_group(2 * 683, 33) == 16
    assert fuzzers.images_per_group(10, 33) == 1
    assert fuzzers.images_per_group(4096, 1) == 1


# ---- the NumPy model of cv2's fixed-point bilinear remap -------------------------------------------------------------
@pytest.mark.parametrize("ndist", [0, 4, 5, 8, 12])
@pytest.mark.parametrize("cn", [1, 3])
def test_np_fixed_remap_reproduces_oracle_undistort(oracle, ndist, cn):
    from calibrating_amd import imgproc
    rng = np.random.default_rng(ndist * 10 + cn)
    for w, h in ((97, 61), (40, 130), (1, 9)):
        K, D = fuzzers._undistort_rig(rng, w, h, ndist)
        img = rng.integers(0, 256, (h, w, cn) if cn == 3 else (h, w), dtype=np.uint8)
        mapxy, mapa = imgproc.undistort_maps(K, D, (w, h))
        got = np_fixed_remap.remap_fixed_bilinear(img, mapxy, mapa, oracle.bilinear_itab())
        assert np.array_equal(got, oracle.undistort_u8(img, K, D)), (w, h)


def test_np_fixed_remap_by_hand(oracle):
    """Phase 0 copies the pixel; the half phase in x averages two neighbours; taps outside read 0 (a cell hanging over
    the top-left corner keeps only its bottom-right tap); bits of the phase map above 1023 are ignored."""
    itab = oracle.bilinear_itab()
    img = np.array([[10, 20], [30, 40]], np.uint8)
    mapxy = np.array([[[0, 0], [0, 0], [-1, -1], [1, 1], [-32768, 32767]]], np.int16)
    half_x = 16                     # (phase y 0) * 32 + (phase x 16)
    corner = 31 * 32 + 31           # weight of the (1, 1) tap: round(31/32 * 31/32 * 32768)
    mapa = np.array([[0, half_x | 0xfc00, corner, 0, 5]], np.uint16)
    got = np_fixed_remap.remap_fixed_bilinear(img, mapxy, mapa, itab)
    w11 = int(itab[corner][3])
    assert got.tolist() == [[10, 15, (10 * w11 + 16384) >> 15, 40, 0]]


# ---- the composition behind camd_disp16_resized_to_depth -------------------------------------------------------------
def test_resized_composition_at_the_same_size_is_the_oracles_disp_to_depth(oracle):
    """At the same size the resize is the identity and ``* w / sw`` is k_disp_to_depth's ``(d * w) / w``: the NumPy lines
    of oracle_pipeline and the C of oracle/depth_ref.c must give the same bits, signed zeros included."""
    rng = np.random.default_rng(3)
    for case in range(40):
        c = fuzzers.gen_depth(5, 3 * case)  # disp_to_depth descriptions
        keys = ("sgbm_min_disparity", "add_min_disparity", "translate", "baseline_fx", "max_depth")
        d16 = c["disp16"][0]
        want = oracle.disp_to_depth(d16, c["mask"], *(c[k] for k in keys))
        got = resized_disparity_to_depth(oracle, d16, d16.shape, c["mask"], *(c[k] for k in keys))
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), case
    d16 = rng.integers(-20, 30, (9, 13)).astype(np.int16)  # (< 2 px after /16: negative once 2 is subtracted)
    mask = np.ones((9, 13), np.uint8)
    mask[::2] = 0
    disp, _ = resized_disparity_to_depth(oracle, d16, (9, 13), mask, 0, -2, True, 100.0, np.inf)
    assert np.signbit(disp[mask == 0]).all() and (disp[mask == 0] == 0).all()  # masked * negative = -0.0


def test_resized_composition_against_float64_bilinear(oracle):
    """An upsizing by a non-integer ratio against cv2's INTER_LINEAR written out in float64 (half-pixel centres, edge
    clamp): within float32 rounding, and the depth is baseline*fx over that disparity."""
    rng = np.random.default_rng(8)
    sh, sw, h, w = 7, 11, 17, 29
    d16 = rng.integers(16, 16 * 40, (sh, sw)).astype(np.int16)
    sd = prepared_disparity(d16, 1).astype(np.float64)

    def axis(n_out, n_in):
        f = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
        s = np.floor(f).astype(int)
        f = f - s
        s0, s1 = np.clip(s, 0, n_in - 1), np.clip(s + 1, 0, n_in - 1)
        f = np.where(s < 0, 0, np.where(s >= n_in - 1, 0, f))
        return s0, s1, f
    y0, y1, fy = axis(h, sh)
    x0, x1, fx = axis(w, sw)
    top = sd[y0][:, x0] * (1 - fx) + sd[y0][:, x1] * fx
    bot = sd[y1][:, x0] * (1 - fx) + sd[y1][:, x1] * fx
    want = (top * (1 - fy[:, None]) + bot * fy[:, None]) * w / sw
    disp, depth = resized_disparity_to_depth(oracle, d16, (h, w), np.ones((h, w), np.uint8), 1, 0, False, 50.0, np.inf)
    assert disp.dtype == np.float32 and depth.dtype == np.float64
    assert np.abs(disp - want).max() <= 1e-5 * np.abs(want).max()
    assert np.array_equal(depth, np.float64(50.0) / disp)


# ---- compare() is bitwise on disparities and depths --------------------------------------------------------------------
def test_compare_sees_the_sign_of_zero():
    disp = np.array([[0.0, 1.5]], np.float32)
    depth = np.array([[0.0, 2.0]], np.float64)
    ref = dict(disparity=disp, rectify_depth=depth)
    assert compare(dict(disparity=disp.copy(), rectify_depth=depth.copy()), ref) == ([], [])
    assert compare(dict(disparity=np.array([[-0.0, 1.5]], np.float32), rectify_depth=depth), ref)[0] == ["disparity"]
    assert compare(dict(disparity=disp, rectify_depth=np.array([[-0.0, 2.0]])), ref) == ([], ["rectify_depth"])
    # inside the tolerance but other bits: inexact; outside: bad
    assert compare(dict(disparity=disp, rectify_depth=np.array([[0.0, np.nextafter(2.0, 3)]])), ref) == \
        ([], ["rectify_depth"])
    assert compare(dict(disparity=disp, rectify_depth=np.array([[0.0, 2.001]])), ref)[0] == ["rectify_depth"]


def test_compare_infinities_and_nan():
    ref = dict(rectify_depth=np.array([np.inf, 1.0]))
    assert compare(dict(rectify_depth=np.array([np.inf, 1.0])), ref) == ([], [])
    assert compare(dict(rectify_depth=np.array([1e300, 1.0])), ref)[0] == ["rectify_depth"]
    assert compare(dict(rectify_depth=np.array([np.nan, 1.0])), ref)[0] == ["rectify_depth"]
    assert compare(dict(rectify_depth=np.array([-np.inf, 1.0])), ref)[0] == ["rectify_depth"]


def test_disparity_to_depth_lines():
    """The NumPy lines of the reference on hand-picked values: d == 0 -> inf -> 0; beyond max_depth -> 0; negative
    -> 0; a masked negative disparity is -0.0, its depth +0.0 (bf / -0.0 = -inf, then clamped)."""
    disp = np.array([0.0, 0.5, 2.0, -1.0, -4.0], np.float32)
    mask = np.array([1, 1, 1, 1, 0], bool)
    d, z = disparity_to_depth(disp, mask, 0, False, 10.0, 15.0)
    assert d.dtype == np.float32 and z.dtype == np.float64
    assert same_bits(d, np.array([0.0, 0.5, 2.0, -1.0, -0.0], np.float32))
    assert same_bits(z, np.array([0.0, 0.0, 5.0, 0.0, 0.0]))


# ---- regression: the host rectify tables formed Anew * R with NumPy's matmul ------------------------------------------
# fuzz_tables (seed 2004, cases 114 and 482, 3840x2160 targets) found one float32 map value 1 ulp away from the oracle
# and the kernel: geometry.init_undistort_rectify_map multiplied Anew @ R through a BLAS with fused multiply-adds, while
# OpenCV's loop (oracle/remap_ref.c, tables.hip) rounds every product and sum.  Shrunk to the rows and columns up to
# the pixel that differed.
TABLE_REGRESSIONS = [
    dict(A=[[4339.603609973168, -0.45625449414592123, 1808.1941762198185], [0.0, 4191.458922448028, 785.9665900196784],
            [0.0, 0.0, 1.0]],
         D=[0.11540766498348973, 0.014756625550803105, -0.0015070547718969824, -0.002666012613483137,
            -0.02059224073631998, 0.06830467787003168, -0.024674158356366674, -0.012169492371551299,
            -0.000912858432388346, 0.0002645302196443609, -0.0008408458141665918, 0.0003735191743574382],
         R=[[0.9997108871002394, -0.02328616266013583, -0.005991397317659387],
            [0.023713815397966232, 0.9960478624588719, 0.08559387040193646],
            [0.003974565702506389, -0.08571120299982966, 0.9963120959357056]],
         Anew=[[3966.4626883465057, 0.0, 1915.7544985716215], [0.0, 3631.8529172970784, 1087.19947545491],
               [0.0, 0.0, 1.0]],
         size=(3813, 778), pixel=(777, 3812)),
    dict(A=[[4641.4496790354215, 0.547559738584265, 1815.8583016963273], [0.0, 4849.844896612277, 800.5593281692117],
            [0.0, 0.0, 1.0]],
         D=[-0.0264252405705931, 0.008008159837453399, -0.0026431742660066103, -0.0012755361284318843,
            0.045898383813411915],
         R=[[0.9977730204757836, -0.00815496869310633, -0.06620042368630139],
            [0.01185581177365702, 0.9983768940867923, 0.05570473122453235],
            [0.06563870304796532, -0.056365537691254484, 0.9962502129600559]],
         Anew=[[5413.551549959062, 0.0, 1928.1940675216838], [0.0, 5359.422540039881, 1088.3920602572207],
               [0.0, 0.0, 1.0]],
         size=(3343, 540), pixel=(539, 3342)),
]


@pytest.mark.parametrize("case", range(len(TABLE_REGRESSIONS)), ids=["seed2004_case114", "seed2004_case482"])
def test_host_rectify_table_forms_anew_r_like_opencv(oracle, case):
    from calibrating_amd import geometry
    c = TABLE_REGRESSIONS[case]
    A, D, R, Anew = (np.array(c[k]) for k in ("A", "D", "R", "Anew"))
    # the product in the plain loop's order, written out with Python floats (one rounding per product and per sum)
    want = [[(Anew[i, 0] * R[0, j] + Anew[i, 1] * R[1, j]) + Anew[i, 2] * R[2, j] for j in range(3)] for i in range(3)]
    assert same_bits(geometry.matmul3_loop(Anew, R), np.array(want))
    gx, gy = geometry.init_undistort_rectify_map(A, D, R, Anew, c["size"])
    ox, oy = oracle.init_undistort_rectify_map(A, D, R, Anew, c["size"])
    assert same_bits(gx, ox) and same_bits(gy, oy), c["pixel"]
