"""ctypes binding of libcalibrating_amd.so (include/calibrating_amd.h).

The library holds the hand-written gfx950 kernels; there is no CPU fallback.  ``lib()`` raises
``RuntimeError`` when the shared object is missing (run ``python -c "import __graft_entry__ as g;
g.build()"`` or ``make -C calibrating_amd/csrc``) and every compute entry point returns
``CAMD_ERR_NO_DEVICE`` -> ``RuntimeError`` when no MI355X is visible.

Two ways into the library.  An entry point that queues work takes the stream as its last argument and is reached through
``call(name, device, *args, what=label)``: it enters ``device``, appends THAT device's current stream and maps the status
to an exception, so the device a launch runs on and the stream it is queued on cannot disagree.  The entry points without
a stream (``*_blocks``, ``*_workspace_bytes``, ``*_grid``, ``*_host``, the SGBM handle's create / destroy / query /
options / profile) are plain ``lib().fn(...)`` calls followed by ``check``.  ``_arrays`` holds the array side of a call.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (bench.py --lib, or CAMD_LIB in the environment of a test / measurement run, points this at an experimental build of
# the same ABI before the first call: A/B of kernel variants built by tools/build_dbg.sh.  Still a HIP library: there
# is no CPU fallback either way)
LIB_PATH = os.environ.get("CAMD_LIB") or os.path.join(_HERE, "lib", "libcalibrating_amd.so")
_lib = None

c_void_p, c_int, c_size_t, c_double = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_double

CAMD_OK = 0
CAMD_ERR_BAD_ARG = -1
CAMD_ERR_UNSUPPORTED = -2
CAMD_ERR_NO_DEVICE = -3
CAMD_ERR_HIP = -4
CAMD_ERR_NOMEM = -5

MODE_SGBM = 0
MODE_HH = 1
MODE_SGBM_3WAY = 2  # cv2's four-stripe, three-direction variant -- UNPINNED vs cv2: stripes, warm-up overlap and the SIMD
                    # tie rule are restated from recollection; tools/export_cv2_golden.py settles them
MODE_HH4 = 3
INTER_NEAREST = 0
INTER_LINEAR = 1
INTER_LANCZOS4 = 4
VALUE_F64, VALUE_F32, VALUE_U8 = 0, 1, 2  # value_type of camd_point_cloud_to_arr2d / camd_uvzs_to_arr2d
VALUE_U16 = 3  # a uint16 depth in millimetres: camd_vis_depth only
NEAREST_MAX_RADIUS = 32  # CAMD_NEAREST_MAX_RADIUS
SPLINE_MAX_POINTS = 1024  # CAMD_SPLINE_MAX_POINTS
POINTS_PIXELS = 0x100  # CAMD_POINTS_PIXELS, or-ed into camd_undistort_points' out_type
# camd_calib_*: the sizes and the places of the state (CAMD_CALIB_*)
CALIB_STATE_DOUBLES, CALIB_WORKSPACE_DOUBLES, CALIB_CANDIDATE_DOUBLES = 40, 136, 16
(CALIB_DONE, CALIB_ACCEPT, CALIB_LAMBDA, CALIB_COST, CALIB_EVALUATIONS, CALIB_ITERATIONS, CALIB_STATUS, CALIB_CONVERGED, CALIB_K,
 CALIB_DK, CALIB_MASK, CALIB_SOLVED, CALIB_PIVOT) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 17, 26, 35, 36
# camd_stereo_*: the same (CAMD_STEREO_*)
STEREO_STATE_DOUBLES, STEREO_WORKSPACE_DOUBLES, STEREO_CANDIDATE_DOUBLES, STEREO_PARTIAL_DOUBLES = 40, 91, 16, 36
(STEREO_DONE, STEREO_ACCEPT, STEREO_LAMBDA, STEREO_COST, STEREO_EVALUATIONS, STEREO_ITERATIONS, STEREO_STATUS, STEREO_CONVERGED,
 STEREO_RIG, STEREO_STEP, STEREO_CANDIDATE, STEREO_SOLVED, STEREO_PIVOT) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 20, 26, 38, 39
# camd_bundle_*: the sizes and the places of the state (CAMD_BUNDLE_*)
BUNDLE_MAX_VIEWS, BUNDLE_CHUNK, BUNDLE_SEGMENT, BUNDLE_PARTIAL_DOUBLES, BUNDLE_EVAL_DOUBLES, BUNDLE_STATE_DOUBLES = 16, 256, 1024, 104, 4, 576
(BUNDLE_DONE, BUNDLE_ACCEPT, BUNDLE_LAMBDA, BUNDLE_COST, BUNDLE_EVALUATIONS, BUNDLE_ITERATIONS, BUNDLE_STATUS, BUNDLE_CONVERGED,
 BUNDLE_SOLVED, BUNDLE_PIVOT, BUNDLE_FIXED, BUNDLE_ANCHOR, BUNDLE_AXIS, BUNDLE_COST0, BUNDLE_LABEL, BUNDLE_POSES, BUNDLE_CANDIDATE,
 BUNDLE_STEP, BUNDLE_K) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 32, 224, 416, 512


class SgbmParams(ctypes.Structure):
    FIELDS = ("minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff",
              "preFilterCap", "uniquenessRatio", "speckleWindowSize", "speckleRange", "mode")
    _fields_ = [(n, c_int) for n in FIELDS]


class CellSet(ctypes.Structure):  # camd_cell_set
    _fields_ = [("uv", c_void_p), ("n", ctypes.c_ulonglong), ("grid_offset", ctypes.c_ulonglong), ("uv_type", c_int),
                ("cu0", c_int), ("cv0", c_int), ("cells_w", c_int), ("cells_h", c_int), ("reserved", c_int)]


class CellTriple(ctypes.Structure):  # camd_cell_triple
    _fields_ = [("grid_offset1", ctypes.c_ulonglong), ("grid_offset2", ctypes.c_ulonglong), ("column_offset", ctypes.c_ulonglong),
                ("cells_w", c_int), ("cells_h", c_int)]


class PnpPoints(ctypes.Structure):  # camd_pnp_points
    _fields_ = [("object", c_void_p), ("image", c_void_p), ("start", c_void_p), ("object_rows", ctypes.c_ulonglong),
                ("image_rows", ctypes.c_ulonglong), ("object_type", c_int), ("image_type", c_int), ("object_stride", c_int),
                ("image_stride", c_int), ("object_shared", c_int), ("frames", c_int)]


class CharucoBoards(ctypes.Structure):  # camd_charuco_boards
    _fields_ = [("n", c_int), ("first_id", c_int * 8)]


class StereoRig(ctypes.Structure):  # camd_stereo_rig
    _fields_ = [("points1", PnpPoints), ("points2", PnpPoints), ("K1", c_void_p), ("dist1", c_void_p), ("K2", c_void_p),
                ("dist2", c_void_p), ("used", c_void_p), ("state", c_void_p), ("poses", c_void_p), ("candidate", c_void_p),
                ("workspace", c_void_p), ("partials", c_void_p), ("frame_error", c_void_p), ("ndist1", c_int), ("ndist2", c_int),
                ("used_n", c_int), ("reserved", c_int)]


class Bundle(ctypes.Structure):  # camd_bundle
    POINTERS = ("uv_a", "uv_b", "pair_views", "pair_start", "seg_first", "seg_n", "chunk_table", "pair_chunk", "status", "points",
                "rowoff", "rowcount", "uv_used_a", "uv_used_b", "X", "candidate", "src", "partials", "pair_blocks", "eval_partials",
                "eval_blocks", "state", "pair_error", "rows_a", "rows_b")
    _fields_ = [(n, c_void_p) for n in POINTERS] + [("threshold", c_double), ("matches", ctypes.c_longlong), ("used", ctypes.c_longlong)] + \
               [(n, c_int) for n in ("uv_type", "views", "pairs", "segments", "chunks", "reserved")]


# name -> (restype, argtypes); every symbol include/calibrating_amd.h declares
SIGNATURES = {
    "camd_last_error": (ctypes.c_char_p, []),
    "camd_version": (c_int, []),
    "camd_device_ok": (c_int, []),
    "camd_sgbm_workspace_bytes": (c_size_t, [ctypes.POINTER(SgbmParams), c_int, c_int, c_int, c_int]),
    "camd_sgbm_create": (c_int, [ctypes.POINTER(SgbmParams), c_int, c_int, c_int, c_int,
                                 ctypes.POINTER(c_void_p)]),
    "camd_sgbm_destroy": (c_int, [c_void_p]),
    "camd_sgbm_compute": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_size_t,
                                  c_size_t, c_int, c_void_p]),
    "camd_sgbm_query": (c_int, [c_void_p] + [ctypes.POINTER(c_int)] * 4),
    "camd_sgbm_debug_copy": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "camd_sgbm_set_option": (c_int, [c_void_p, c_int, c_int]),
    "camd_sgbm_status": (c_int, [c_void_p, c_void_p]),
    "camd_sgbm_set_profiling": (c_int, [c_void_p, c_int]),
    "camd_sgbm_num_stages": (c_int, []),
    "camd_sgbm_stage_name": (ctypes.c_char_p, [c_int]),
    "camd_sgbm_get_profile": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_float), c_int]),
    "camd_median3_s16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "camd_speckle_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "camd_filter_speckles_s16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                         c_void_p]),
    "camd_remap_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_size_t, c_size_t, c_void_p, c_void_p,
                              c_void_p, c_int, c_int, c_size_t, c_size_t, c_int, c_int, c_int, c_void_p]),
    "camd_remap_fixed_bilinear_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_size_t, c_size_t, c_void_p,
                                             c_void_p, c_void_p, c_int, c_int, c_size_t, c_size_t, c_int,
                                             c_void_p]),
    "camd_undistort_maps_host": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "camd_init_undistort_rectify_map": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                                c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "camd_undistort_maps": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "camd_point_cloud_grid": (c_int, [c_int, c_int, c_double, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "camd_point_cloud_workspace_bytes": (c_size_t, [c_int, c_int, c_double]),
    "camd_depth_to_point_cloud": (c_int, [c_void_p, c_int, c_int, c_void_p, c_double, c_void_p, c_void_p, c_size_t,
                                          c_void_p, c_void_p, c_void_p]),
    "camd_apply_T_to_point_cloud": (c_int, [c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "camd_point_cloud_to_depth": (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_int, c_int, c_double, c_void_p,
                                          c_void_p, c_void_p]),
    "camd_project_depth": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_double, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p]),
    "camd_reproject_remap": (c_int, [c_void_p, c_int, c_int, c_size_t, c_void_p, c_void_p, c_void_p, c_double, c_int, c_int,
                                     c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_int, c_void_p]),
    "camd_point_cloud_to_arr2d": (c_int, [c_void_p, c_size_t, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int,
                                          c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_uvzs_to_arr2d": (c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_int, c_int, c_double, c_int, c_void_p,
                                   c_void_p, c_void_p]),
    "camd_arr2d_to_uvzs": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "camd_arr2d_mask_workspace_bytes": (c_size_t, [c_int]),
    "camd_arr2d_to_uvzs_masked": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p,
                                          c_void_p]),
    "camd_sparse_bin_grid": (c_int, [c_int, c_int, c_double] + [ctypes.POINTER(c_int)] * 3),
    "camd_sparse_bin_count": (c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_double, c_void_p, c_void_p]),
    "camd_sparse_bin_fill": (c_int, [c_void_p, c_size_t, c_int, c_int, c_int, c_double, c_void_p, c_size_t, c_void_p,
                                     c_void_p, c_void_p]),
    "camd_nearest_fill": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_void_p, c_int,
                                  c_int, c_void_p]),
    "camd_plane_sums_blocks": (c_int, [c_size_t]),
    "camd_plane_sums": (c_int, [c_void_p, c_int, c_void_p, c_int, c_size_t, c_void_p, c_void_p, c_void_p]),
    "camd_plane_eval": (c_int, [c_double, c_double, c_double, c_int, c_int, c_void_p, c_void_p]),
    "camd_matched_uvs_to_zs": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "camd_cell_first_index": (c_int, [c_void_p, c_int, c_size_t, c_int, c_double, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                      c_void_p]),
    "camd_cell_population": (c_int, [c_void_p, c_int, c_size_t, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "camd_cell_intersect_count": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "camd_cell_intersect_emit": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
                                         c_void_p]),
    "camd_overlap_blocks": (c_int, [c_size_t]),
    "camd_overlap_keep": (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p]),
    "camd_overlap_emit": (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                  c_void_p, c_void_p]),
    "camd_epipolar_sums_blocks": (c_int, [c_size_t]),
    "camd_epipolar_sums": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_vector_sum_blocks": (c_int, [c_size_t]),
    "camd_vector_sum": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "camd_flow_to_matched_uvs": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p,
                                         c_void_p, c_void_p]),
    "camd_flow_abs_to_normal": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "camd_flow_normal_to_abs": (c_int, [c_void_p, c_int, c_int, c_int, c_double, c_double, c_void_p, c_void_p]),
    "camd_warp_flow_backward_u8": (c_int, [c_void_p, c_int, c_size_t, c_size_t, c_void_p, c_int, c_size_t, c_void_p, c_int, c_int,
                                           c_size_t, c_size_t, c_int, c_int, c_void_p]),
    "camd_warp_flow_forward_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_size_t, c_size_t, c_void_p, c_int, c_size_t, c_void_p,
                                          c_int, c_int, c_size_t, c_size_t, c_int, c_void_p, c_int, c_void_p]),
    "camd_vis_l1_error": (c_int, [c_void_p, c_void_p, c_double, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_vis_l1_limit_workspace_bytes": (c_size_t, [c_int]),
    "camd_vis_l1_limit": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_vis_l1_bar": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "camd_vis_l1_colour": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "camd_vis_depth_range": (c_int, [c_void_p, c_int, c_size_t, c_int, c_double, c_double, c_double, c_void_p, c_void_p]),
    "camd_vis_depth": (c_int, [c_void_p, c_int, c_size_t, c_int, c_double, c_double, c_double, c_double, c_double, c_void_p,
                               c_int, c_double, c_double, c_void_p, c_int, c_void_p, c_void_p]),
    "camd_vis_lines": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
                               c_size_t, c_size_t, c_size_t, c_void_p]),
    "camd_uv_bounds_blocks": (c_int, []),
    "camd_uv_bounds_batch": (c_int, [ctypes.POINTER(CellSet), c_int, c_void_p, c_void_p, c_void_p]),
    "camd_cell_first_index_batch": (c_int, [ctypes.POINTER(CellSet), c_int, c_void_p, c_double, c_void_p, c_size_t, c_void_p,
                                            c_void_p]),
    "camd_cell_intersect_count_batch": (c_int, [c_void_p, c_size_t, ctypes.POINTER(CellTriple), c_int, c_void_p, c_void_p,
                                                c_size_t, c_void_p]),
    "camd_cell_intersect_emit_batch": (c_int, [c_void_p, c_size_t, ctypes.POINTER(CellTriple), c_int, c_void_p, c_void_p,
                                               c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "camd_uvzi_pack": (c_int, [c_void_p, c_int, c_void_p, c_size_t, c_double, c_void_p, c_size_t, c_size_t, c_void_p]),
    "camd_column_sum_blocks": (c_int, [c_size_t]),
    "camd_column_sum": (c_int, [c_void_p, c_size_t, c_int, c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p]),
    "camd_column_scale": (c_int, [c_void_p, c_size_t, c_int, c_int, c_size_t, c_size_t, c_double, c_void_p]),
    "camd_set_global_option": (c_int, [c_int, c_int]),
    "camd_lanczos4_table_host": (c_int, [c_void_p]),
    "camd_bilinear_table_host": (c_int, [c_void_p]),
    "camd_resize_linear_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "camd_resize_linear_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "camd_disp_to_depth": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_double,
                                   c_double, c_void_p, c_void_p, c_int, c_void_p]),
    "camd_disp16_resized_to_depth": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                             c_double, c_double, c_void_p, c_void_p, c_int, c_void_p]),
    "camd_unrectify_depth": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int, c_int, c_int, c_void_p]),
    "camd_distort_index_map": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "camd_distort_depth": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "camd_undistort_points": (c_int, [c_void_p, c_int, c_size_t, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int,
                                      c_void_p]),
    "camd_project_points": (c_int, [c_void_p, c_int, c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                    c_void_p]),
    "camd_pnp_init": (c_int, [ctypes.POINTER(PnpPoints), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "camd_pnp_refine": (c_int, [ctypes.POINTER(PnpPoints), c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    "camd_calib_homography": (c_int, [ctypes.POINTER(PnpPoints), c_void_p, c_void_p, c_void_p]),
    "camd_calib_linearise": (c_int, [ctypes.POINTER(PnpPoints), c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_calib_step": (c_int, [ctypes.POINTER(PnpPoints), c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_calib_finish": (c_int, [ctypes.POINTER(PnpPoints), c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_calib_read": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "camd_stereo_linearise": (c_int, [ctypes.POINTER(StereoRig), c_void_p]),
    "camd_stereo_step": (c_int, [ctypes.POINTER(StereoRig), c_void_p]),
    "camd_stereo_finish": (c_int, [ctypes.POINTER(StereoRig), c_void_p]),
    "camd_bundle_start": (c_int, [ctypes.POINTER(Bundle), ctypes.c_longlong, c_void_p]),
    "camd_bundle_emit": (c_int, [ctypes.POINTER(Bundle), c_void_p]),
    "camd_bundle_step": (c_int, [ctypes.POINTER(Bundle), c_void_p]),
    "camd_bundle_finish": (c_int, [ctypes.POINTER(Bundle), c_void_p]),
    "camd_corner_sub_pix": (c_int, [c_void_p, c_int, c_int, c_size_t, c_size_t, c_int, c_void_p, c_int, c_size_t, c_void_p, c_int,
                                    c_int, c_void_p, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_bgr_to_gray_u8": (c_int, [c_void_p, c_int, c_int, c_size_t, c_size_t, c_void_p, c_size_t, c_size_t, c_int, c_int, c_int,
                                    c_int, c_int, c_void_p]),
    "camd_chess_response": (c_int, [c_void_p, c_int, c_int, c_size_t, c_size_t, c_int, c_void_p, c_void_p, c_void_p]),
    "camd_chess_peaks_workspace_bytes": (c_size_t, [c_int, c_int]),
    "camd_chess_peaks": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_chess_lattice": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "camd_charuco_detect": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_size_t, c_size_t, c_int, c_int, c_int, c_int, c_int,
                                    c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_charuco_detect_multi": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_size_t, c_size_t, c_int, c_int, c_int, c_int,
                                          c_int, c_void_p, c_int, c_int, ctypes.POINTER(CharucoBoards), c_int, c_int, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    "camd_dark_mask": (c_int, [c_void_p, c_int, c_int, c_size_t, c_size_t, c_int, c_int, c_int, c_void_p, c_void_p]),
    "camd_label_components": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "camd_marker_candidates_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "camd_marker_candidates": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_marker_decode": (c_int, [c_void_p, c_int, c_int, c_size_t, c_size_t, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                   c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_laplacian_sums": (c_int, [c_void_p, c_int, c_int, c_size_t, c_size_t, c_int, c_void_p, c_void_p]),
    "camd_hull_fit": (c_int, [c_void_p, c_int, c_void_p, c_int, c_size_t, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_hull_fill": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "camd_hull_mask": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "camd_spline_assemble": (c_int, [c_void_p, c_int, c_size_t, c_void_p, c_int, c_int, c_double, c_void_p, c_void_p]),
    "camd_spline_solve": (c_int, [c_void_p, c_int, c_size_t, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_spline_eval": (c_int, [c_void_p, c_int, c_size_t, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                 c_void_p]),
    "camd_spline_upsize": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "camd_cloud_workspace_bytes": (c_size_t, [c_size_t]),
    "camd_cloud_to_uvzs": (c_int, [c_void_p, c_int, c_size_t, c_int, c_void_p, c_void_p, c_int, c_int, c_double, c_int, c_void_p,
                                   c_size_t, c_void_p, c_void_p, c_void_p]),
    "camd_hull_row_range": (c_int, [c_void_p, c_int, c_size_t, c_void_p, c_void_p]),
    "camd_hull_extremes": (c_int, [c_void_p, c_int, c_size_t, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_nearest_fill_in_hull": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_size_t, c_int, c_int, c_double, c_void_p,
                                          c_void_p, c_int, c_void_p, c_void_p]),
    "camd_essential_hypotheses": (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_int, c_int, c_void_p, c_void_p, ctypes.c_ulonglong,
                                          c_int, c_void_p, c_void_p, c_void_p]),
    "camd_essential_score": (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_double,
                                     c_void_p, c_void_p, c_void_p]),
    "camd_essential_moments_blocks": (c_int, [c_size_t]),
    "camd_essential_moments": (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_int, c_int, c_void_p, c_void_p, c_void_p, c_double,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_essential_batch_hypotheses": (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_int, c_int, c_void_p, c_int, ctypes.c_ulonglong,
                                                c_int, c_void_p, c_void_p, c_void_p]),
    "camd_essential_batch_score": (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                           c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "camd_essential_batch_moments": (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                             c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_feature_score": (c_int, [c_void_p, c_int, c_int, c_size_t, c_size_t, c_int, c_int, c_void_p, c_void_p]),
    "camd_feature_keypoints_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "camd_feature_keypoints": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_feature_describe": (c_int, [c_void_p, c_int, c_int, c_size_t, c_size_t, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
    "camd_feature_search": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "camd_feature_filter_workspace_bytes": (c_size_t, [c_int]),
    "camd_feature_filter": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                    c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# include/calibrating_amd_experimental.h: measurement hooks without a counterpart in the reference's interface (CU-masked
# streams; with them goes set_option's CAMD_OPT_PHASES = 6).  Bound so that tools/ and one parity test can reach them;
# nothing in this package calls them.
EXPERIMENTAL_SIGNATURES = {
    "camd_stream_create_cu_mask": (c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p)]),
    "camd_stream_destroy": (c_int, [c_void_p]),
}


def lib():
    """The loaded library (declares every signature on first use)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "calibrating_amd: %s is missing -- build the HIP extension first "
                "(make -C calibrating_amd/csrc). There is no CPU fallback." % LIB_PATH)
        # torch first: it bundles its own libamdhip64.so.7; loading ours afterwards binds to that same
        # HIP runtime instance, so device pointers and streams are shared with torch
        import torch  # noqa: F401
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(EXPERIMENTAL_SIGNATURES.items()):
            fn = getattr(l, name)  # AttributeError here = header and library disagree
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def last_error():
    msg = lib().camd_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, what=""):
    """Map a camd_status to the exception the reference would raise at that point."""
    if rc == CAMD_OK:
        return
    msg = "%s%s" % (what + ": " if what else "", last_error())
    if rc in (CAMD_ERR_BAD_ARG, CAMD_ERR_UNSUPPORTED):
        raise ValueError(msg)
    if rc == CAMD_ERR_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def require_device():
    check(lib().camd_device_ok(), "calibrating_amd")


def current_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, device, *args, what=None):
    """``lib().<name>(*args, stream)`` on ``device`` and on the current stream OF THAT DEVICE, then ``check`` under the
    label ``what`` (default: the entry point's name).  For every entry point whose last parameter is the stream."""
    import torch
    with torch.cuda.device(device):
        rc = getattr(lib(), name)(*args, current_stream())
    check(rc, name if what is None else what)
