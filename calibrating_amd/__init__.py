"""calibrating_amd -- MI355X-native stereo depth path of DIYer22/calibrating.

Drop-in for the ``Stereo.get_depth`` hot path of the reference behind its own plugin surface
(calibrating/__init__.py:3-14 exports these names): ``MetaStereoMatching``,
``SemiGlobalBlockMatching``, ``Stereo``, ``Cam``.  The per-pair work runs in hand-written gfx950
kernels (calibrating_amd/csrc, C ABI in include/calibrating_amd.h); importing the package needs no
GPU, computing does.
"""
from .__info__ import __version__
from .camera import Cam
from .sgbm import MODE_HH, MODE_HH4, MODE_SGBM, MODE_SGBM_3WAY, StereoSGBM, StereoSGBM_create
from .stereo_matching import FeatureMatchingAsStereoMatching, MatchingByBoard, MetaStereoMatching, SemiGlobalBlockMatching
from .stereo_camera import Stereo
from .epipolar_geometry import (EssentialMatrixStereo, build_set2ds_by_flowds, filter_overlap_uvs, find_essential_matrices, find_essential_matrix,
                                flow_abs_to_normal, flow_normal_to_abs, flow_to_matched_uvs, matching_uvs_in_one_img,
                                matching_uvs_in_one_img_batch)
from .reconstruction_epipolar_geometry import ReconstructionExtrinsics
from .bundle import bundle_adjust_pairs
from .flow_utils import warp_flow
from .geometry import mean_Ts
from .pnp import solve_pnp_batch
from .calibrate import (CALIB_FIX_FOCAL_LENGTH, CALIB_FIX_K1, CALIB_FIX_K2, CALIB_FIX_K3, CALIB_FIX_K4, CALIB_FIX_K5, CALIB_FIX_K6,
                        CALIB_FIX_PRINCIPAL_POINT, CALIB_USE_INTRINSIC_GUESS, CALIB_ZERO_TANGENT_DIST, calibrate_camera)
from .stereo_calibrate import CALIB_FIX_INTRINSIC, CALIB_USE_EXTRINSIC_GUESS, stereo_calibrate
from .vis import resolve_max_l1, vis_align, vis_depth, vis_depth_l1, vis_stereo
from .boards import ArucoGridBoard, BaseBoard, CharucoBoard, Chessboard, MarkerBoard, MultiBoards
from .multi_boards import MultiBoardsCam
from .reconstruction_with_board import convert_cam_to_nerf_json, get_sharpness
from .features import BinaryFeatureMatching, detect_and_describe, match_descriptors, match_images, match_views
from .lidar import calibrate_lidar2cam, uvs_on_depth_to_xyzs, xyzs_to_dense_depth

__all__ = ["Cam", "Stereo", "MetaStereoMatching", "SemiGlobalBlockMatching", "StereoSGBM",
           "StereoSGBM_create", "MODE_SGBM", "MODE_HH", "MODE_SGBM_3WAY", "MODE_HH4", "__version__",
           "FeatureMatchingAsStereoMatching", "EssentialMatrixStereo", "filter_overlap_uvs", "matching_uvs_in_one_img",
           "flow_abs_to_normal", "flow_normal_to_abs", "flow_to_matched_uvs", "build_set2ds_by_flowds",
           "matching_uvs_in_one_img_batch", "ReconstructionExtrinsics", "warp_flow", "vis_depth", "vis_depth_l1",
           "resolve_max_l1", "vis_stereo", "vis_align", "solve_pnp_batch", "mean_Ts",
           "calibrate_camera", "CALIB_USE_INTRINSIC_GUESS", "CALIB_FIX_PRINCIPAL_POINT", "CALIB_FIX_FOCAL_LENGTH",
           "CALIB_ZERO_TANGENT_DIST", "CALIB_FIX_K1", "CALIB_FIX_K2", "CALIB_FIX_K3", "CALIB_FIX_K4", "CALIB_FIX_K5", "CALIB_FIX_K6",
           "stereo_calibrate", "CALIB_FIX_INTRINSIC", "CALIB_USE_EXTRINSIC_GUESS", "BaseBoard", "Chessboard", "CharucoBoard", "MarkerBoard", "ArucoGridBoard",
           "MatchingByBoard", "MultiBoards", "MultiBoardsCam", "convert_cam_to_nerf_json", "get_sharpness", "find_essential_matrix", "find_essential_matrices",
           "BinaryFeatureMatching", "detect_and_describe", "match_descriptors", "match_images", "match_views", "bundle_adjust_pairs",
           "xyzs_to_dense_depth", "uvs_on_depth_to_xyzs", "calibrate_lidar2cam"]
