"""The order of an entry point's checks, pinned without a GPU: what every stream-taking entry point of
include/calibrating_amd.h (the SGBM handle calls aside) answers -- status and camd_last_error() text -- to

  null    every pointer NULL, every number 0;
  formed  a well-formed call: made-up, aligned device addresses that nothing on the host may read, real host arrays
          where the header says "host" (camera matrices, poses, the tables of the batched cell calls).  Without a device
          it ends at the probe, CAMD_ERR_NO_DEVICE, after every argument check and before anything is queued;
  empty   the formed call with its row count (camd_vis_l1_bar: the bar's width) set to 0, for the entry points that have
          one: some answer CAMD_OK before the probe, some reach the probe first, some refuse it -- all three are
          behaviour the Python side relies on.

EXPECTED was recorded with these very calls from the library as it stood BEFORE the entry points got their shared
value-type dispatch and probe macro (csrc/common.hpp), the way WORKSPACE_BYTES of test_boundary_cpu.py was; it is never
re-recorded from the code under test.  The module skips itself where a GPU is visible: there the formed calls would
pass the probe and hand the made-up addresses to a kernel."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from calibrating_amd import _native
from calibrating_amd._native import VALUE_F32, VALUE_F64, VALUE_U8, VALUE_U16

if torch.cuda.is_available():
    pytest.skip("a GPU is present: the well-formed calls must not reach a kernel", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def A(k):
    """made-up device address number k: 1 MiB apart, aligned to anything; never dereferenced"""
    return 0x7000000000 + (k << 20)


W, H, NPIX, N = 8, 6, 48, 5
K = np.array([500.0, 0, 4, 0, 500, 3, 0, 0, 1])
KINV = np.array([0.002, 0, -0.008, 0, 0.002, -0.006, 0, 0, 1])
DIST = np.array([0.1, -0.05, 0.001, 0.002, 0.01])
R3, T3, M3 = np.eye(3).ravel(), np.array([0.1, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
T4 = np.eye(4).ravel()
T64 = np.tile(T4, 4)
SETS = (_native.CellSet * 2)(_native.CellSet(A(0), N, 0, VALUE_F64, 0, 0, W, H, 0),
                             _native.CellSet(A(1), N, NPIX, VALUE_F32, 0, 0, W, H, 0))
TRIPLES = (_native.CellTriple * 1)(_native.CellTriple(0, NPIX, 0, W, H))


def host(a):
    return a.ctypes.data


# name -> (the formed call's arguments without the stream, index of the row count or None)
CASES = {
    "camd_median3_s16": ((A(0), A(1), W, H, 1), None),
    "camd_filter_speckles_s16": ((A(0), W, H, 0, 10, 16, A(1), 1), None),
    "camd_remap_u8": ((A(0), W, H, 1, W, NPIX, A(1), A(2), A(3), W, H, W, NPIX, _native.INTER_LINEAR, 0, 1), None),
    "camd_remap_fixed_bilinear_u8": ((A(0), W, H, 1, W, NPIX, A(1), A(2), A(3), W, H, W, NPIX, 1), None),
    "camd_init_undistort_rectify_map": ((host(K), host(DIST), 5, host(R3), host(K), W, H, A(0), A(1), A(2), W, H), None),
    "camd_undistort_maps": ((host(K), host(DIST), 5, W, H, A(0), A(1)), None),
    "camd_depth_to_point_cloud": ((A(0), W, H, host(KINV), 1.0, A(1), A(2), NPIX, A(3), A(4)), None),
    "camd_apply_T_to_point_cloud": ((A(0), N, host(T4), A(1)), 1),
    "camd_point_cloud_to_depth": ((A(0), N, 3, host(K), W, H, 0.0, A(1), A(2)), 1),
    "camd_project_depth": ((A(0), W, H, host(KINV), host(T4), host(K), 1.0, W, H, A(1), A(2)), None),
    "camd_reproject_remap": ((A(0), W, H, NPIX, host(KINV), host(T4), host(K), 1.0, W, H, A(1), A(2), NPIX, A(3), A(4), 1),
                             None),
    "camd_point_cloud_to_arr2d": ((A(0), N, 3, host(K), W, H, A(1), 1, VALUE_F32, 0.0, A(2), A(3), A(4)), 1),
    "camd_uvzs_to_arr2d": ((A(0), N, 2, W, H, A(1), 1, VALUE_U8, 0.0, 0, A(2), A(3)), 1),
    "camd_arr2d_to_uvzs": ((A(0), W, H, 0, A(1)), None),
    "camd_arr2d_to_uvzs_masked": ((A(0), A(1), W, H, 0, A(2), NPIX, A(3), A(4)), None),
    "camd_sparse_bin_count": ((A(0), N, 2, W, H, 2.0, A(1)), 1),
    "camd_sparse_bin_fill": ((A(0), N, 2, W, H, 2.0, A(1), N, A(2), A(3)), 1),
    "camd_nearest_fill": ((A(0), A(1), A(2), A(3), VALUE_F64, W, H, 2.0, A(4), W, H), None),
    "camd_plane_sums": ((A(0), 2, A(1), VALUE_F32, N, A(2), A(3)), 4),
    "camd_plane_eval": ((1.0, 2.0, 3.0, W, H, A(0)), None),
    "camd_matched_uvs_to_zs": ((A(0), A(1), N, host(KINV), host(KINV), host(T4), A(2), A(3)), 2),
    "camd_cell_first_index": ((A(0), VALUE_F64, N, 2, 1.5, 0, 0, W, H, A(1), A(2)), 2),
    "camd_cell_population": ((A(0), VALUE_F32, N, 2, 0, 0, W, H, A(1), A(2)), 2),
    "camd_cell_intersect_count": ((A(0), A(1), W, H, A(2)), None),
    "camd_cell_intersect_emit": ((A(0), A(1), W, H, A(2), A(3), A(4), NPIX, A(5)), None),
    "camd_overlap_keep": ((A(0), A(1), VALUE_F64, N, 2, 0, 0, W, H, A(2), A(3), A(4), A(5)), 3),
    "camd_overlap_emit": ((A(0), A(1), VALUE_F32, N, 2, A(2), A(3), A(4), A(5), N, A(6)), 3),
    "camd_epipolar_sums": ((A(0), A(1), N, host(KINV), host(KINV), host(T64), A(2), A(3)), 2),
    "camd_vector_sum": ((A(0), N, None, N, A(1), A(2)), 3),
    "camd_flow_to_matched_uvs": ((A(0), VALUE_F32, A(1), W, H, A(2), A(3), NPIX, A(4), A(5)), None),
    "camd_flow_abs_to_normal": ((A(0), VALUE_F64, W, H, A(1)), None),
    "camd_flow_normal_to_abs": ((A(0), VALUE_F32, W, H, 8.0, 6.0, A(1)), None),
    "camd_warp_flow_backward_u8": ((A(0), 1, W, NPIX, A(1), VALUE_F32, 2 * NPIX, A(2), W, H, W, NPIX, _native.INTER_LINEAR, 1),
                                   None),
    "camd_warp_flow_forward_u8": ((A(0), W, H, 1, W, NPIX, A(1), VALUE_F64, 2 * NPIX, A(2), W, H, W, NPIX,
                                   _native.INTER_NEAREST, A(3), 1), None),
    "camd_vis_l1_error": ((A(0), A(1), 0.0, VALUE_F32, W, H, 1, 0, 0, 1.0, A(2), A(3), A(4), A(5)), None),
    "camd_vis_l1_limit": ((A(0), A(1), NPIX, 1, 2, 0.5, A(2), A(3), A(4)), None),
    "camd_vis_l1_bar": ((A(0), A(1), W, H, 1, 1, 2, A(2)), 6),
    "camd_vis_l1_colour": ((A(0), A(1), NPIX, 1, A(2), 0, A(3)), None),
    "camd_vis_depth_range": ((A(0), VALUE_U16, NPIX, 1, 1000.0, 0.0, 10.0, A(1)), None),
    "camd_vis_depth": ((A(0), VALUE_U16, NPIX, 1, 1000.0, 0.0, 10.0, 0.0, 1.0, A(1), 1, 0.0, 255.0, A(2), 1, A(3)), None),
    "camd_vis_lines": ((A(0), 3, A(1), 1, W, H, 1, A(2), None, 2, A(3), 3 * W, 3 * NPIX, 6 * NPIX), None),
    "camd_uv_bounds_batch": ((SETS, 2, A(2), A(3)), None),
    "camd_cell_first_index_batch": ((SETS, 2, A(2), 1.5, A(3), 2 * NPIX, A(4)), None),
    "camd_cell_intersect_count_batch": ((A(0), 2 * NPIX, TRIPLES, 1, A(1), A(2), W), None),
    "camd_cell_intersect_emit_batch": ((A(0), 2 * NPIX, TRIPLES, 1, A(1), A(2), W, A(3), A(4), NPIX, A(5)), None),
    "camd_uvzi_pack": ((A(0), VALUE_F32, A(1), N, 1.0, A(2), 2 * N, 2), 3),
    "camd_column_sum": ((A(0), 2 * N, 4, 2, 2, N, A(1), A(2)), 5),
    "camd_column_scale": ((A(0), 2 * N, 4, 2, 2, N, 0.5), 5),
    "camd_resize_linear_u8": ((A(0), W, H, 1, A(1), 5, 4, 1), None),
    "camd_resize_linear_f32": ((A(0), W, H, A(1), 2 * W, 2 * H, 1), None),
    "camd_disp_to_depth": ((A(0), A(1), W, H, 0, 0, 0, 100.0, 10.0, A(2), A(3), 1), None),
    "camd_disp16_resized_to_depth": ((A(0), 5, 4, A(1), W, H, 0, 0, 0, 100.0, 10.0, A(2), A(3), 1), None),
    "camd_unrectify_depth": ((A(0), W, H, host(M3), A(1), A(2), A(3), W, H, 1), None),
    "camd_distort_index_map": ((host(K), host(DIST), 5, W, H, A(0), A(1)), None),
    "camd_distort_depth": ((A(0), 8, W, H, A(1), A(2), 1), None),
    "camd_undistort_points": ((A(0), VALUE_F32, N, 2, host(K), host(DIST), 5, 5, A(1), VALUE_F64 | _native.POINTS_PIXELS), 2),
    "camd_project_points": ((A(0), VALUE_F64, N, 3, host(R3), host(T3), host(K), host(DIST), 5, A(1)), 2),
}

# camd_median3_s16 and camd_filter_speckles_s16 have no probe: without a device their formed call ends in the HIP
# runtime's own launch error, a text with a source line in it, so only their null call is pinned.
NO_PROBE = ("camd_median3_s16", "camd_filter_speckles_s16")


def calls(name):
    """[(kind, arguments with the NULL stream)] of one entry point"""
    args, n_at = CASES[name]
    types = _native.SIGNATURES[name][1]
    assert len(args) + 1 == len(types), name
    pointer = lambda t: t is _native.c_void_p or issubclass(t, ctypes._Pointer)
    out = [("null", tuple(None if pointer(t) else 0.0 if t is _native.c_double else 0 for t in types))]
    if name not in NO_PROBE:
        out.append(("formed", args + (None,)))
        if n_at is not None:
            out.append(("empty", args[:n_at] + (0,) + args[n_at + 1:] + (None,)))
    return out


def answer(name, args):
    rc = getattr(_native.lib(), name)(*args)
    return (rc, None if rc == _native.CAMD_OK else _native.last_error())  # (CAMD_OK leaves an older message in place)


NO_DEVICE = (-3, "no HIP device available (no ROCm-capable device is detected): the MI355X kernels cannot run and "
                 "there is no CPU fallback")
BAD = -1
EXPECTED = {
    "camd_apply_T_to_point_cloud": {"null": (BAD, "camd_apply_T_to_point_cloud: NULL argument"),
                                    "formed": NO_DEVICE, "empty": (0, None)},
    "camd_arr2d_to_uvzs": {"null": (BAD, "camd_arr2d_to_uvzs: bad arguments"),
                           "formed": NO_DEVICE},
    "camd_arr2d_to_uvzs_masked": {"null": (BAD, "camd_arr2d_to_uvzs_masked: bad arguments"),
                                  "formed": NO_DEVICE},
    "camd_cell_first_index": {"null": (BAD, "camd_cell_first_index: a window of 0 x 0 cells is empty or beyond 2^28 cells"),
                              "formed": NO_DEVICE, "empty": NO_DEVICE},
    "camd_cell_first_index_batch": {"null": (BAD, "camd_cell_first_index_batch: 1 .. 65535 sets and both tables are required"),
                                    "formed": NO_DEVICE},
    "camd_cell_intersect_count": {"null": (BAD, "camd_cell_intersect_count: a window of 0 x 0 cells is empty or beyond 2^28 cells"),
                                  "formed": NO_DEVICE},
    "camd_cell_intersect_count_batch": {"null": (BAD, "camd_cell_intersect_count_batch: 1 .. 65535 triples and both tables are required"),
                                        "formed": NO_DEVICE},
    "camd_cell_intersect_emit": {"null": (BAD, "camd_cell_intersect_emit: a window of 0 x 0 cells is empty or beyond 2^28 cells"),
                                 "formed": NO_DEVICE},
    "camd_cell_intersect_emit_batch": {"null": (BAD, "camd_cell_intersect_emit_batch: 1 .. 65535 triples and both tables are required"),
                                       "formed": NO_DEVICE},
    "camd_cell_population": {"null": (BAD, "camd_cell_population: a window of 0 x 0 cells is empty or beyond 2^28 cells"),
                             "formed": NO_DEVICE, "empty": NO_DEVICE},
    "camd_column_scale": {"null": (BAD, "camd_column_scale: bad arguments"),
                          "formed": NO_DEVICE, "empty": (0, None)},
    "camd_column_sum": {"null": (BAD, "camd_column_sum: bad arguments"),
                        "formed": NO_DEVICE, "empty": (BAD, "camd_column_sum: bad arguments")},
    "camd_depth_to_point_cloud": {"null": (BAD, "camd_depth_to_point_cloud: bad size / interpolation rate"),
                                  "formed": NO_DEVICE},
    "camd_disp16_resized_to_depth": {"null": (BAD, "camd_disp16_resized_to_depth: bad arguments"),
                                     "formed": NO_DEVICE},
    "camd_disp_to_depth": {"null": (BAD, "camd_disp_to_depth: bad arguments"),
                           "formed": NO_DEVICE},
    "camd_distort_depth": {"null": (BAD, "camd_distort_depth: bad arguments (elem_bytes is 4 or 8; out must not alias depth; batch <= 2^19)"),
                           "formed": NO_DEVICE},
    "camd_distort_index_map": {"null": (BAD, "camd_distort_index_map: bad arguments"),
                               "formed": NO_DEVICE},
    "camd_epipolar_sums": {"null": (BAD, "camd_epipolar_sums: bad arguments"),
                           "formed": NO_DEVICE, "empty": (BAD, "camd_epipolar_sums: bad arguments")},
    "camd_filter_speckles_s16": {"null": (BAD, "camd_filter_speckles_s16: bad arguments")},
    "camd_flow_abs_to_normal": {"null": (BAD, "camd_flow_abs_to_normal: bad arguments"),
                                "formed": NO_DEVICE},
    "camd_flow_normal_to_abs": {"null": (BAD, "camd_flow_normal_to_abs: bad arguments"),
                                "formed": NO_DEVICE},
    "camd_flow_to_matched_uvs": {"null": (BAD, "camd_flow_to_matched_uvs: bad arguments"),
                                 "formed": NO_DEVICE},
    "camd_init_undistort_rectify_map": {"null": (BAD, "camd_init_undistort_rectify_map: bad arguments"),
                                        "formed": NO_DEVICE},
    "camd_matched_uvs_to_zs": {"null": (BAD, "camd_matched_uvs_to_zs: NULL argument"),
                               "formed": NO_DEVICE, "empty": (0, None)},
    "camd_median3_s16": {"null": (BAD, "camd_median3_s16: bad arguments (dst must differ from src)")},
    "camd_nearest_fill": {"null": (BAD, "camd_nearest_fill: bad grid size 0 x 0"),
                          "formed": NO_DEVICE},
    "camd_overlap_emit": {"null": (BAD, "camd_overlap_emit: bad arguments"),
                          "formed": NO_DEVICE, "empty": NO_DEVICE},
    "camd_overlap_keep": {"null": (BAD, "camd_overlap_keep: a window of 0 x 0 cells is empty or beyond 2^28 cells"),
                          "formed": NO_DEVICE, "empty": (0, None)},
    "camd_plane_eval": {"null": (BAD, "camd_plane_eval: bad arguments"),
                        "formed": NO_DEVICE},
    "camd_plane_sums": {"null": (BAD, "camd_plane_sums: bad arguments"),
                        "formed": NO_DEVICE, "empty": (BAD, "camd_plane_sums: bad arguments")},
    "camd_point_cloud_to_arr2d": {"null": (BAD, "camd_point_cloud_to_arr2d: bad arguments"),
                                  "formed": NO_DEVICE, "empty": NO_DEVICE},
    "camd_point_cloud_to_depth": {"null": (BAD, "camd_point_cloud_to_depth: bad arguments"),
                                  "formed": NO_DEVICE, "empty": NO_DEVICE},
    "camd_project_depth": {"null": (BAD, "camd_project_depth: bad size / interpolation rate"),
                           "formed": NO_DEVICE},
    "camd_project_points": {"null": (BAD, "camd_project_points: bad arguments (xyz / out: CAMD_VALUE_F64 or _F32, aligned to an element / a row"
                                          " of two; xyz_stride >= 3, got 0; n < 2^31; R, t: 9 and 3 host doubles)"),
                            "formed": NO_DEVICE, "empty": (0, None)},
    "camd_remap_fixed_bilinear_u8": {"null": (BAD, "camd_remap_fixed_bilinear_u8: bad arguments"),
                                     "formed": NO_DEVICE},
    "camd_remap_u8": {"null": (BAD, "camd_remap_u8: bad arguments"),
                      "formed": NO_DEVICE},
    "camd_reproject_remap": {"null": (BAD, "camd_reproject_remap: bad size / interpolation rate"),
                             "formed": NO_DEVICE},
    "camd_resize_linear_f32": {"null": (BAD, "camd_resize_linear_f32: bad arguments"),
                               "formed": NO_DEVICE},
    "camd_resize_linear_u8": {"null": (BAD, "camd_resize_linear_u8: bad arguments"),
                              "formed": NO_DEVICE},
    "camd_sparse_bin_count": {"null": (BAD, "camd_sparse_bin_count: bad grid size 0 x 0"),
                              "formed": NO_DEVICE, "empty": NO_DEVICE},
    "camd_sparse_bin_fill": {"null": (BAD, "camd_sparse_bin_fill: bad grid size 0 x 0"),
                             "formed": NO_DEVICE, "empty": (0, None)},
    "camd_undistort_maps": {"null": (BAD, "camd_undistort_maps: bad arguments"),
                            "formed": NO_DEVICE},
    "camd_undistort_points": {"null": (BAD, "camd_undistort_points: bad arguments (uv / out: CAMD_VALUE_F64 or _F32, aligned to an element / a "
                                            "row of two; uv_stride >= 2, got 0; n < 2^31; iters 1 .. 100, got 0)"),
                              "formed": NO_DEVICE, "empty": (0, None)},
    "camd_unrectify_depth": {"null": (BAD, "camd_unrectify_depth: bad arguments"),
                             "formed": NO_DEVICE},
    "camd_uv_bounds_batch": {"null": (BAD, "camd_uv_bounds_batch: 1 .. 65535 sets and both tables are required"),
                             "formed": NO_DEVICE},
    "camd_uvzi_pack": {"null": (BAD, "camd_uvzi_pack: bad arguments (rows 0 + 0 of 0)"),
                       "formed": NO_DEVICE, "empty": (0, None)},
    "camd_uvzs_to_arr2d": {"null": (BAD, "camd_uvzs_to_arr2d: bad arguments"),
                           "formed": NO_DEVICE, "empty": NO_DEVICE},
    "camd_vector_sum": {"null": (BAD, "camd_vector_sum: bad arguments"),
                        "formed": NO_DEVICE, "empty": (BAD, "camd_vector_sum: bad arguments")},
    "camd_vis_depth": {"null": (BAD, "camd_vis_depth: bad size: 0 pixels (1 .. 2^31 - 1), batch 0 (1 .. 65535)"),
                       "formed": NO_DEVICE},
    "camd_vis_depth_range": {"null": (BAD, "camd_vis_depth_range: bad size: 0 pixels (1 .. 2^31 - 1), batch 0 (1 .. 65535)"),
                             "formed": NO_DEVICE},
    "camd_vis_l1_bar": {"null": (BAD, "camd_vis_l1_bar: bad size 0 x 0, batch 0 (1 .. 65535)"),
                        "formed": NO_DEVICE, "empty": NO_DEVICE},
    "camd_vis_l1_colour": {"null": (BAD, "camd_vis_l1_colour: bad size: 0 pixels (1 .. 2^31 - 1), batch 0 (1 .. 65535)"),
                           "formed": NO_DEVICE},
    "camd_vis_l1_error": {"null": (BAD, "camd_vis_l1_error: bad size 0 x 0, batch 0 (1 .. 65535)"),
                          "formed": NO_DEVICE},
    "camd_vis_l1_limit": {"null": (BAD, "camd_vis_l1_limit: bad size: 0 pixels (1 .. 2^31 - 1), batch 0 (1 .. 65535)"),
                          "formed": NO_DEVICE},
    "camd_vis_lines": {"null": (BAD, "camd_vis_lines: bad size 0 x 0, batch 0 (1 .. 65535)"),
                       "formed": NO_DEVICE},
    "camd_warp_flow_backward_u8": {"null": (BAD, "camd_warp_flow_backward_u8: bad arguments"),
                                   "formed": NO_DEVICE},
    "camd_warp_flow_forward_u8": {"null": (BAD, "camd_warp_flow_forward_u8: bad arguments"),
                                  "formed": NO_DEVICE},
}


def test_every_stream_entry_point_is_in_the_table():
    src = open(os.path.join(ROOT, "include", "calibrating_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    streamed = set(re.findall(r"\b(camd_[A-Za-z0-9_]+)\s*\([^;{}]*\bvoid\*\s*stream\)", src))
    assert len(streamed) >= 60 and streamed <= set(_native.SIGNATURES)
    assert {s for s in streamed if not s.startswith("camd_sgbm_")} == set(CASES) == set(EXPECTED)


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_answers_as_recorded(name):
    got = {kind: answer(name, args) for kind, args in calls(name)}
    assert got == EXPECTED[name]
    if name not in NO_PROBE:
        assert got["formed"] == NO_DEVICE


def test_the_forward_warp_probes_before_it_looks_at_its_workspace():
    """camd_warp_flow_forward_u8 shares check_warp, probe included, with the backward warp and tests winner_ws after it"""
    args, _ = CASES["camd_warp_flow_forward_u8"]
    assert answer("camd_warp_flow_forward_u8", args[:15] + (None,) + args[16:] + (None,)) == NO_DEVICE
