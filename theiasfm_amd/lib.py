"""Loader + thin ctypes wrapper of the C-ABI library (include/theia_mi355_ba.h).

The library is built in-tree by ``__graft_entry__.build()`` into
``theiasfm_amd/lib/libtheia_mi355_ba.so``.  There is no CPU fallback: if the
library is missing, or no HIP device is visible when a solve is requested, the
calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtheia_mi355_ba.so")
_lib = None

# every symbol include/theia_mi355_ba.h declares
EXPORTS = (
    "tmi_ba_version", "tmi_ba_device_count", "tmi_ba_status_string", "tmi_ba_last_error",
    "tmi_ba_options_init",
    "tmi_ba_intrinsics_size", "tmi_ba_intrinsics_constant_mask", "tmi_ba_solve",
    "tmi_ba_solver_create", "tmi_ba_solver_set_allreduce", "tmi_ba_solver_solve",
    "tmi_ba_solver_reset", "tmi_ba_solver_set_parameters", "tmi_ba_solver_download", "tmi_ba_solver_stream",
    "tmi_ba_solver_destroy", "tmi_ba_solver_evaluate", "tmi_ba_structure_stats", "tmi_ba_structure_stats_for",
    "tmi_ba_rccl_unique_id", "tmi_ba_solver_init_rccl", "tmi_ba_solver_debug_allreduce",
    "tmi_ba_solver_filter_outlier_tracks", "tmi_ba_filter_outlier_tracks",
    "tmi_ba_solver_adjust_tracks", "tmi_ba_adjust_tracks",
    "tmi_ba_solver_adjust_views", "tmi_ba_adjust_views",
    "tmi_ba_track_estimator_options_init", "tmi_ba_solver_estimate_tracks", "tmi_ba_estimate_tracks",
    "tmi_ba_solver_select_good_tracks", "tmi_ba_select_good_tracks",
    "tmi_ba_adjust_two_views", "tmi_ba_adjust_two_views_angular", "tmi_ba_optimize_relative_positions",
    "tmi_ba_two_view_verification_options_init", "tmi_ba_verify_two_views",
    "tmi_ba_translation_filter_options_init", "tmi_ba_filter_view_pairs_from_relative_translation",
    "tmi_ba_filter_view_pairs_from_orientation",
    "tmi_ba_largest_connected_component", "tmi_ba_orientations_from_maximum_spanning_tree",
    "tmi_ba_robust_rotation_options_init", "tmi_ba_estimate_global_rotations_robust",
    "tmi_ba_lud_position_options_init", "tmi_ba_estimate_global_positions_lud",
    "tmi_ba_nonlinear_position_options_init", "tmi_ba_estimate_global_positions_nonlinear",
    "tmi_ba_nonlinear_rotation_options_init", "tmi_ba_estimate_global_rotations_nonlinear",
    "tmi_ba_linear_rotation_options_init", "tmi_ba_estimate_global_rotations_linear",
    "tmi_ba_rigid_subgraph_options_init", "tmi_ba_extract_parallel_rigid_subgraph",
    "tmi_ba_linear_position_options_init", "tmi_ba_estimate_global_positions_linear",
    "tmi_ba_localization_options_init", "tmi_ba_localize_views",
    "tmi_ba_match_options_init", "tmi_ba_match_features",
    "tmi_ba_cascade_match_options_init", "tmi_ba_match_features_cascade",
    "tmi_ba_guided_match_options_init", "tmi_ba_guided_epipolar_match",
    "tmi_ba_track_build_options_init", "tmi_ba_build_tracks",
    "tmi_ba_two_view_ransac_options_init", "tmi_ba_estimate_uncalibrated_relative_poses",
    "tmi_ba_estimate_calibrated_relative_poses",
    "tmi_ba_homography_ransac_options_init", "tmi_ba_estimate_homographies",
    "tmi_ba_estimate_positions_known_orientation", "tmi_ba_estimate_relative_positions_known_orientation",
    "tmi_ba_solver_structure_checksums",
    "tmi_ba_solver_operator_info",
)

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)


class LibraryMissing(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP engine has no CPU fallback)")
    # Load order matters: torch bundles its own libamdhip64.so (SONAME
    # libamdhip64.so.7, the same as /opt/rocm's).  Imported first, the loader
    # resolves the engine's NEEDED libamdhip64.so.7 to torch's already loaded
    # runtime, so the engine and torch share ONE HIP runtime and streams / device
    # pointers are interchangeable (needed by the all-reduce hook).  Loaded the
    # other way round the process ends up with two runtimes and torch sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    P, O, S = C.POINTER(abi.CProblem), C.POINTER(abi.COptions), C.POINTER(abi.CSummary)
    L.tmi_ba_version.restype = C.c_int32
    L.tmi_ba_device_count.restype = C.c_int32
    L.tmi_ba_status_string.restype = C.c_char_p
    L.tmi_ba_status_string.argtypes = [C.c_int32]
    L.tmi_ba_last_error.restype = C.c_char_p
    L.tmi_ba_options_init.argtypes = [O]
    L.tmi_ba_options_init.restype = None
    L.tmi_ba_intrinsics_size.argtypes = [C.c_int32]
    L.tmi_ba_intrinsics_size.restype = C.c_int32
    L.tmi_ba_intrinsics_constant_mask.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
    L.tmi_ba_intrinsics_constant_mask.restype = C.c_int32
    L.tmi_ba_solve.argtypes = [P, O, S]
    L.tmi_ba_solve.restype = C.c_int32
    L.tmi_ba_solver_create.argtypes = [P, O, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.tmi_ba_solver_create.restype = C.c_int32
    L.tmi_ba_solver_set_allreduce.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p]
    L.tmi_ba_solver_set_allreduce.restype = C.c_int32
    L.tmi_ba_solver_solve.argtypes = [C.c_void_p, O, S]
    L.tmi_ba_solver_solve.restype = C.c_int32
    L.tmi_ba_solver_reset.argtypes = [C.c_void_p]
    L.tmi_ba_solver_reset.restype = C.c_int32
    L.tmi_ba_solver_set_parameters.argtypes = [C.c_void_p, C.c_void_p]
    L.tmi_ba_solver_set_parameters.restype = C.c_int32
    L.tmi_ba_solver_download.argtypes = [C.c_void_p, P]
    L.tmi_ba_solver_download.restype = C.c_int32
    L.tmi_ba_solver_stream.argtypes = [C.c_void_p]
    L.tmi_ba_solver_stream.restype = C.c_void_p
    L.tmi_ba_solver_destroy.argtypes = [C.c_void_p]
    L.tmi_ba_solver_destroy.restype = None
    L.tmi_ba_solver_evaluate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_int32)]
    L.tmi_ba_solver_evaluate.restype = C.c_int32
    L.tmi_ba_rccl_unique_id.argtypes = [C.c_void_p]
    L.tmi_ba_rccl_unique_id.restype = C.c_int32
    L.tmi_ba_solver_init_rccl.argtypes = [C.c_void_p, C.c_void_p]
    L.tmi_ba_solver_init_rccl.restype = C.c_int32
    L.tmi_ba_solver_debug_allreduce.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_double)]
    L.tmi_ba_solver_debug_allreduce.restype = C.c_int32
    L.tmi_ba_structure_stats.argtypes = [P, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    L.tmi_ba_structure_stats.restype = C.c_int32
    L.tmi_ba_structure_stats_for.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    L.tmi_ba_structure_stats_for.restype = C.c_int32
    FS, TS = C.POINTER(abi.CFilterSummary), C.POINTER(abi.CTrackBatchSummary)
    L.tmi_ba_solver_filter_outlier_tracks.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                                      C.c_void_p, FS]
    L.tmi_ba_solver_filter_outlier_tracks.restype = C.c_int32
    L.tmi_ba_filter_outlier_tracks.argtypes = [P, C.c_int32, C.c_double, C.c_double, C.c_void_p,
                                               C.c_void_p, FS]
    L.tmi_ba_filter_outlier_tracks.restype = C.c_int32
    L.tmi_ba_solver_adjust_tracks.argtypes = [C.c_void_p, O, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, TS]
    L.tmi_ba_solver_adjust_tracks.restype = C.c_int32
    L.tmi_ba_adjust_tracks.argtypes = [P, O, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, TS]
    L.tmi_ba_adjust_tracks.restype = C.c_int32
    VS = C.POINTER(abi.CViewBatchSummary)
    L.tmi_ba_solver_adjust_views.argtypes = [C.c_void_p, O, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, VS]
    L.tmi_ba_solver_adjust_views.restype = C.c_int32
    L.tmi_ba_adjust_views.argtypes = [P, O, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, VS]
    L.tmi_ba_adjust_views.restype = C.c_int32
    EO, ES = C.POINTER(abi.CTrackEstimatorOptions), C.POINTER(abi.CTrackEstimateSummary)
    L.tmi_ba_track_estimator_options_init.argtypes = [EO]
    L.tmi_ba_track_estimator_options_init.restype = None
    L.tmi_ba_solver_estimate_tracks.argtypes = [C.c_void_p, EO, O, C.c_void_p, C.c_void_p, ES]
    L.tmi_ba_solver_estimate_tracks.restype = C.c_int32
    L.tmi_ba_estimate_tracks.argtypes = [P, EO, O, C.c_void_p, C.c_void_p, ES]
    L.tmi_ba_estimate_tracks.restype = C.c_int32
    L.tmi_ba_adjust_two_views.argtypes = [C.POINTER(abi.CTwoViewBatch), C.c_int32, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, TS]
    L.tmi_ba_adjust_two_views.restype = C.c_int32
    VO, VSUM = C.POINTER(abi.CTwoViewVerificationOptions), C.POINTER(abi.CTwoViewVerificationSummary)
    L.tmi_ba_two_view_verification_options_init.argtypes = [VO]
    L.tmi_ba_two_view_verification_options_init.restype = None
    L.tmi_ba_verify_two_views.argtypes = [C.POINTER(abi.CTwoViewBatch), VO, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, VSUM]
    L.tmi_ba_verify_two_views.restype = C.c_int32
    L.tmi_ba_adjust_two_views_angular.argtypes = [C.POINTER(abi.CTwoViewAngularBatch), C.c_int32, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(abi.CTrackBatchSummary)]
    L.tmi_ba_adjust_two_views_angular.restype = C.c_int32
    L.tmi_ba_optimize_relative_positions.argtypes = [C.POINTER(abi.CRelativePositionBatch), C.c_int32, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.POINTER(abi.CTrackBatchSummary)]
    L.tmi_ba_optimize_relative_positions.restype = C.c_int32
    PB, PFS = C.POINTER(abi.CViewPairBatch), C.POINTER(abi.CViewPairFilterSummary)
    L.tmi_ba_translation_filter_options_init.argtypes = [C.POINTER(abi.CTranslationFilterOptions)]
    L.tmi_ba_translation_filter_options_init.restype = None
    L.tmi_ba_filter_view_pairs_from_relative_translation.argtypes = [
        PB, C.POINTER(abi.CTranslationFilterOptions), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
        C.c_void_p, C.c_void_p, PFS]
    L.tmi_ba_filter_view_pairs_from_relative_translation.restype = C.c_int32
    L.tmi_ba_filter_view_pairs_from_orientation.argtypes = [PB, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, PFS]
    L.tmi_ba_filter_view_pairs_from_orientation.restype = C.c_int32
    L.tmi_ba_largest_connected_component.argtypes = [PB, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.POINTER(abi.CViewGraphComponentSummary)]
    L.tmi_ba_largest_connected_component.restype = C.c_int32
    L.tmi_ba_orientations_from_maximum_spanning_tree.argtypes = [
        PB, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.POINTER(abi.CSpanningTreeSummary)]
    L.tmi_ba_orientations_from_maximum_spanning_tree.restype = C.c_int32
    RO = C.POINTER(abi.CRobustRotationOptions)
    L.tmi_ba_robust_rotation_options_init.argtypes = [RO]
    L.tmi_ba_robust_rotation_options_init.restype = None
    L.tmi_ba_estimate_global_rotations_robust.argtypes = [
        C.POINTER(abi.CRelativeRotationBatch), RO, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(abi.CRobustRotationSummary)]
    L.tmi_ba_estimate_global_rotations_robust.restype = C.c_int32
    LO = C.POINTER(abi.CLudPositionOptions)
    L.tmi_ba_lud_position_options_init.argtypes = [LO]
    L.tmi_ba_lud_position_options_init.restype = None
    L.tmi_ba_estimate_global_positions_lud.argtypes = [
        PB, LO, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.POINTER(abi.CLudPositionSummary)]
    L.tmi_ba_estimate_global_positions_lud.restype = C.c_int32
    NO = C.POINTER(abi.CNonlinearPositionOptions)
    L.tmi_ba_nonlinear_position_options_init.argtypes = [NO]
    L.tmi_ba_nonlinear_position_options_init.restype = None
    L.tmi_ba_estimate_global_positions_nonlinear.argtypes = [
        PB, NO, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.POINTER(abi.CNonlinearPositionSummary)]
    L.tmi_ba_estimate_global_positions_nonlinear.restype = C.c_int32
    NR = C.POINTER(abi.CNonlinearRotationOptions)
    L.tmi_ba_nonlinear_rotation_options_init.argtypes = [NR]
    L.tmi_ba_nonlinear_rotation_options_init.restype = None
    L.tmi_ba_estimate_global_rotations_nonlinear.argtypes = [
        PB, NR, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.POINTER(abi.CNonlinearRotationSummary)]
    L.tmi_ba_estimate_global_rotations_nonlinear.restype = C.c_int32
    LR = C.POINTER(abi.CLinearRotationOptions)
    L.tmi_ba_linear_rotation_options_init.argtypes = [LR]
    L.tmi_ba_linear_rotation_options_init.restype = None
    L.tmi_ba_estimate_global_rotations_linear.argtypes = [
        PB, LR, C.c_int32, C.c_void_p, C.POINTER(abi.CLinearRotationSummary)]
    L.tmi_ba_estimate_global_rotations_linear.restype = C.c_int32
    RS = C.POINTER(abi.CRigidSubgraphOptions)
    L.tmi_ba_rigid_subgraph_options_init.argtypes = [RS]
    L.tmi_ba_rigid_subgraph_options_init.restype = None
    L.tmi_ba_extract_parallel_rigid_subgraph.argtypes = [
        PB, C.c_void_p, RS, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(abi.CRigidSubgraphSummary)]
    L.tmi_ba_extract_parallel_rigid_subgraph.restype = C.c_int32
    LP = C.POINTER(abi.CLinearPositionOptions)
    L.tmi_ba_linear_position_options_init.argtypes = [LP]
    L.tmi_ba_linear_position_options_init.restype = None
    L.tmi_ba_estimate_global_positions_linear.argtypes = [
        P, PB, LP, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [
        C.POINTER(abi.CLinearPositionSummary)]
    L.tmi_ba_estimate_global_positions_linear.restype = C.c_int32
    ZO =C.POINTER(abi.CLocalizationOptions)
    L.tmi_ba_localization_options_init.argtypes = [ZO]
    L.tmi_ba_localization_options_init.restype = None
    L.tmi_ba_localize_views.argtypes = [P, ZO, O, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 9 + [
        C.POINTER(abi.CLocalizationSummary)]
    L.tmi_ba_localize_views.restype = C.c_int32
    MO = C.POINTER(abi.CMatchOptions)
    L.tmi_ba_match_options_init.argtypes = [MO]
    L.tmi_ba_match_options_init.restype = None
    L.tmi_ba_match_features.argtypes = [MO, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_int64] + [C.c_void_p] * 6 + [C.POINTER(abi.CMatchSummary)]
    L.tmi_ba_match_features.restype = C.c_int32
    GO = C.POINTER(abi.CGuidedMatchOptions)
    L.tmi_ba_guided_match_options_init.argtypes = [GO]
    L.tmi_ba_guided_match_options_init.restype = None
    L.tmi_ba_guided_epipolar_match.argtypes = [GO, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [
        C.c_void_p] * 8 + [C.c_int64] + [C.c_void_p] * 9 + [C.POINTER(abi.CGuidedMatchSummary)]
    L.tmi_ba_guided_epipolar_match.restype = C.c_int32
    KO = C.POINTER(abi.CCascadeMatchOptions)
    L.tmi_ba_cascade_match_options_init.argtypes = [KO]
    L.tmi_ba_cascade_match_options_init.restype = None
    L.tmi_ba_match_features_cascade.argtypes = [KO, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 8 + [
        C.POINTER(abi.CCascadeMatchSummary)]
    L.tmi_ba_match_features_cascade.restype = C.c_int32
    TO = C.POINTER(abi.CTrackBuildOptions)
    L.tmi_ba_track_build_options_init.argtypes = [TO]
    L.tmi_ba_track_build_options_init.restype = None
    L.tmi_ba_build_tracks.argtypes = [TO, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 5 + [
        C.POINTER(abi.CTrackBuildSummary)]
    L.tmi_ba_build_tracks.restype = C.c_int32
    RO = C.POINTER(abi.CTwoViewRansacOptions)
    L.tmi_ba_two_view_ransac_options_init.argtypes = [RO]
    L.tmi_ba_two_view_ransac_options_init.restype = None
    L.tmi_ba_estimate_uncalibrated_relative_poses.argtypes = [RO, C.c_int32] + [C.c_void_p] * 7 + [C.c_int32] + [
        C.c_void_p] * 13 + [C.POINTER(abi.CTwoViewRansacSummary)]
    L.tmi_ba_estimate_uncalibrated_relative_poses.restype = C.c_int32
    L.tmi_ba_estimate_calibrated_relative_poses.argtypes = [RO, C.c_int32] + [C.c_void_p] * 7 + [C.c_int32] + [
        C.c_void_p] * 12 + [C.POINTER(abi.CTwoViewRansacSummary)]
    L.tmi_ba_estimate_calibrated_relative_poses.restype = C.c_int32
    HO = C.POINTER(abi.CHomographyRansacOptions)
    L.tmi_ba_homography_ransac_options_init.argtypes = [HO]
    L.tmi_ba_homography_ransac_options_init.restype = None
    L.tmi_ba_estimate_homographies.argtypes = [HO, C.c_int32] + [C.c_void_p] * 7 + [C.c_int32] + [
        C.c_void_p] * 10 + [C.POINTER(abi.CTwoViewRansacSummary)]
    L.tmi_ba_estimate_homographies.restype = C.c_int32
    L.tmi_ba_estimate_positions_known_orientation.argtypes = [HO, C.c_int32] + [C.c_void_p] * 8 + [C.c_int32] + [
        C.c_void_p] * 11 + [C.POINTER(abi.CTwoViewRansacSummary)]
    L.tmi_ba_estimate_positions_known_orientation.restype = C.c_int32
    L.tmi_ba_estimate_relative_positions_known_orientation.argtypes = [HO, C.c_int32] + [C.c_void_p] * 9 + [
        C.c_int32] + [C.c_void_p] * 12 + [C.POINTER(abi.CTwoViewRansacSummary)]
    L.tmi_ba_estimate_relative_positions_known_orientation.restype = C.c_int32
    L.tmi_ba_solver_structure_checksums.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.tmi_ba_solver_structure_checksums.restype = C.c_int32
    L.tmi_ba_solver_operator_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.tmi_ba_solver_operator_info.restype = C.c_int32
    SS = C.POINTER(abi.CSelectSummary)
    L.tmi_ba_solver_select_good_tracks.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, SS]
    L.tmi_ba_solver_select_good_tracks.restype = C.c_int32
    L.tmi_ba_select_good_tracks.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, SS]
    L.tmi_ba_select_good_tracks.restype = C.c_int32
    _lib = L
    return L


STRUCTURE_STAT_NAMES = ("tracks", "observations", "reduced_blocks", "block_dim", "upper_blocks",
                        "bsr_blocks", "pairs", "block_checksum", "slices", "padded_observations",
                        "observation_checksum", "pair_checksum")


def structure_stats(problem: abi.Problem, rank: int = 0, world: int = 1, forms_S: bool = True) -> dict:
    """Host-only statistics of the static structure for one rank (no GPU).  forms_S=False: the dealing of a handle whose
    operator is matrix-free (the default on several ranks) -- slices balanced by observations, not by Schur pairs."""
    L = load()
    cp = problem.as_c()
    out = (C.c_int64 * 12)()
    st = L.tmi_ba_structure_stats_for(C.byref(cp), rank, world, 1 if forms_S else 0, out)
    if st != 0:
        raise EngineError(st, "tmi_ba_structure_stats")
    return dict(zip(STRUCTURE_STAT_NAMES, list(out)))


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId through the engine's run-time RCCL binding (call on rank 0)."""
    L = load()
    buf = (C.c_uint8 * 128)()
    st = L.tmi_ba_rccl_unique_id(buf)
    if st != 0:
        raise EngineError(st, "tmi_ba_rccl_unique_id")
    return bytes(buf)


class EngineError(RuntimeError):
    def __init__(self, status, where, message=""):
        self.status = status
        name = abi.STATUS_NAMES.get(status, str(status))
        if not message and _lib is not None:
            message = (_lib.tmi_ba_last_error() or b"").decode("utf-8", "replace")
        super().__init__(f"{where}: status {status} ({name}) {message}")


def solve(problem: abi.Problem, options: abi.COptions):
    """One-shot tmi_ba_solve: upload, LM on the GPU, download into `problem`."""
    L = load()
    cp = problem.as_c()
    s = abi.CSummary()
    st = L.tmi_ba_solve(C.byref(cp), C.byref(options), C.byref(s))
    return st, s


def filter_outlier_tracks(problem: abi.Problem, max_inlier_reprojection_error: float,
                          min_triangulation_angle_degrees: float, device: int = -1):
    """One-shot SetOutlierTracksToUnestimated: (flag [Np] uint8, mean squared reprojection
    error [Np], CFilterSummary)."""
    L = load()
    cp = problem.as_c()
    n = problem.num_points
    flag = np.zeros(n, dtype=np.uint8)
    mean = np.zeros(n)
    fs = abi.CFilterSummary()
    st = L.tmi_ba_filter_outlier_tracks(C.byref(cp), device, float(max_inlier_reprojection_error),
                                        float(min_triangulation_angle_degrees), flag.ctypes.data,
                                        mean.ctypes.data, C.byref(fs))
    if st != 0:
        raise EngineError(st, "tmi_ba_filter_outlier_tracks")
    return flag, mean, fs


def select_good_tracks(problem: abi.Problem, long_track_length_threshold: int,
                       image_grid_cell_size_pixels: int, min_num_optimized_tracks_per_view: int,
                       view_mask=None, device: int = -1):
    """One-shot SelectGoodTracksForBundleAdjustment: (selected [Np] uint8, truncated length
    [Np] int32, mean squared error [Np], CSelectSummary)."""
    L = load()
    cp = problem.as_c()
    n = problem.num_points
    sel = np.zeros(n, dtype=np.uint8)
    ln = np.zeros(n, dtype=np.int32)
    err = np.zeros(n)
    ss = abi.CSelectSummary()
    vm = None if view_mask is None else np.ascontiguousarray(view_mask, dtype=np.uint8)
    st = L.tmi_ba_select_good_tracks(C.byref(cp), device, long_track_length_threshold,
                                     image_grid_cell_size_pixels, min_num_optimized_tracks_per_view,
                                     None if vm is None else vm.ctypes.data, sel.ctypes.data, ln.ctypes.data, err.ctypes.data, C.byref(ss))
    if st != 0:
        raise EngineError(st, "tmi_ba_select_good_tracks")
    return sel, ln, err, ss


def adjust_tracks(problem: abi.Problem, options: abi.COptions):
    """One-shot batched BundleAdjustTrack; problem.points is updated in place.  Returns
    (termination [Np] int8, iterations [Np] int32, initial cost [Np], final cost [Np],
    CTrackBatchSummary)."""
    L = load()
    cp = problem.as_c()
    n = problem.num_points
    term = np.full(n, -1, dtype=np.int8)
    iters = np.zeros(n, dtype=np.int32)
    c0 = np.zeros(n)
    c1 = np.zeros(n)
    ts = abi.CTrackBatchSummary()
    st = L.tmi_ba_adjust_tracks(C.byref(cp), C.byref(options), term.ctypes.data, iters.ctypes.data,
                                c0.ctypes.data, c1.ctypes.data, C.byref(ts))
    if st != 0:
        raise EngineError(st, "tmi_ba_adjust_tracks")
    return term, iters, c0, c1, ts


def _view_outputs(n, view_mask):
    vm = None if view_mask is None else np.ascontiguousarray(view_mask, dtype=np.uint8)
    if vm is not None and vm.shape != (n,):
        raise ValueError(f"view_mask must have num_cameras = {n} entries")
    return (vm, np.full(n, -1, dtype=np.int8), np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n),
            abi.CViewBatchSummary())


def adjust_views(problem: abi.Problem, options: abi.COptions, view_mask=None):
    """One-shot batched BundleAdjustView over the views view_mask selects (None = all); problem.extrinsics /
    intrinsics are updated in place for the usable views.  Returns (termination [Nc] int8, iterations [Nc] int32,
    initial cost [Nc], final cost [Nc], CViewBatchSummary)."""
    L = load()
    cp = problem.as_c()
    vm, term, iters, c0, c1, vs = _view_outputs(problem.num_cameras, view_mask)
    st = L.tmi_ba_adjust_views(C.byref(cp), C.byref(options), None if vm is None else vm.ctypes.data,
                               term.ctypes.data, iters.ctypes.data, c0.ctypes.data, c1.ctypes.data, C.byref(vs))
    if st != 0:
        raise EngineError(st, "tmi_ba_adjust_views")
    return term, iters, c0, c1, vs


def _track_mask(n, track_mask):
    tm = None if track_mask is None else np.ascontiguousarray(track_mask, dtype=np.uint8)
    if tm is not None and tm.shape != (n,):
        raise ValueError(f"track_mask must have num_points = {n} entries")
    return tm, np.full(n, -1, dtype=np.int8), abi.CTrackEstimateSummary()


def estimate_tracks(problem: abi.Problem, estimator_options: abi.CTrackEstimatorOptions, ba_options: abi.COptions,
                    track_mask=None):
    """One-shot batched TrackEstimator over the tracks track_mask selects (None = all); problem.points is updated in
    place for the statuses 0, 3 and 4.  Returns (status [Np] int8, CTrackEstimateSummary)."""
    L = load()
    cp = problem.as_c()
    tm, status, es = _track_mask(problem.num_points, track_mask)
    st = L.tmi_ba_estimate_tracks(C.byref(cp), C.byref(estimator_options), C.byref(ba_options),
                                  None if tm is None else tm.ctypes.data, status.ctypes.data, C.byref(es))
    if st != 0:
        raise EngineError(st, "tmi_ba_estimate_tracks")
    return status, es


def adjust_two_views(batch: abi.TwoViewBatch, point_dof: int = 4, max_num_iterations: int = 200, device: int = -1):
    """Batched BundleAdjustTwoViews; batch.extrinsics2 / intrinsics / points are updated in place
    for the usable pairs.  Returns (termination [P] int8, iterations [P] int32, initial cost [P],
    final cost [P], CTrackBatchSummary)."""
    L = load()
    cb = batch.as_c()
    n = batch.num_pairs
    term = np.full(n, -1, dtype=np.int8)
    iters = np.zeros(n, dtype=np.int32)
    c0 = np.zeros(n)
    c1 = np.zeros(n)
    ts = abi.CTrackBatchSummary()
    st = L.tmi_ba_adjust_two_views(C.byref(cb), int(point_dof), int(max_num_iterations), int(device),
                                   term.ctypes.data, iters.ctypes.data, c0.ctypes.data, c1.ctypes.data,
                                   C.byref(ts))
    if st != 0:
        raise EngineError(st, "tmi_ba_adjust_two_views")
    return term, iters, c0, c1, ts


def verify_two_views(batch: abi.TwoViewBatch, options: abi.CTwoViewVerificationOptions = None, point_dof: int = 4,
                     max_num_iterations: int = 200, device: int = -1):
    """Batched two-view verification BA (TwoViewMatchGeometricVerification::BundleAdjustRelativePose): triangulate,
    adjust, filter.  batch.points is an output only; batch.extrinsics2 / focal lengths are updated in place for the
    pairs of status 0 or 4, batch.points for the correspondences of status 0 or 4.  Returns a dict: correspondence_status
    [N] int8, pair_status [P] int8, pair_num_verified [P] int32, termination [P] int8, iterations [P] int32,
    initial_cost [P], final_cost [P], summary (CTwoViewVerificationSummary)."""
    L = load()
    if options is None:
        options = abi.two_view_verification_options()
    cb = batch.as_c()
    n = batch.num_pairs
    N = batch.features1.shape[0]
    out = {
        "correspondence_status": np.full(N, -1, dtype=np.int8),
        "pair_status": np.full(n, -1, dtype=np.int8),
        "pair_num_verified": np.zeros(n, dtype=np.int32),
        "termination": np.full(n, -1, dtype=np.int8),
        "iterations": np.zeros(n, dtype=np.int32),
        "initial_cost": np.zeros(n),
        "final_cost": np.zeros(n),
    }
    vs = abi.CTwoViewVerificationSummary()
    st = L.tmi_ba_verify_two_views(C.byref(cb), C.byref(options), int(point_dof), int(max_num_iterations), int(device),
                                   *[a.ctypes.data for a in out.values()], C.byref(vs))
    if st != 0:
        raise EngineError(st, "tmi_ba_verify_two_views")
    out["summary"] = vs
    return out


def adjust_two_views_angular(batch: abi.TwoViewAngularBatch, max_num_iterations: int = 200, device: int = -1):
    """Batched BundleAdjustTwoViewsAngular; batch.rotation2 / position2 are updated in place for the usable
    pairs.  Returns (termination [P] int8, iterations [P] int32, initial cost [P], final cost [P],
    CTrackBatchSummary)."""
    L = load()
    cb = batch.as_c()
    n = batch.num_pairs
    term = np.full(n, -1, dtype=np.int8)
    iters = np.zeros(n, dtype=np.int32)
    c0 = np.zeros(n)
    c1 = np.zeros(n)
    ts = abi.CTrackBatchSummary()
    st = L.tmi_ba_adjust_two_views_angular(C.byref(cb), int(max_num_iterations), int(device), term.ctypes.data,
                                           iters.ctypes.data, c0.ctypes.data, c1.ctypes.data, C.byref(ts))
    if st != 0:
        raise EngineError(st, "tmi_ba_adjust_two_views_angular")
    return term, iters, c0, c1, ts


def optimize_relative_positions(batch: abi.RelativePositionBatch, device: int = -1):
    """Batched OptimizeRelativePositionWithKnownRotation; batch.position2 is written for the pairs with status 0 or 1.
    Returns (status [P] int8, iterations [P] int32, cost [P], num_in_front [P] int32, CTrackBatchSummary)."""
    L = load()
    cb = batch.as_c()
    n = batch.num_pairs
    status = np.full(n, -1, dtype=np.int8)
    iters = np.zeros(n, dtype=np.int32)
    cost = np.zeros(n)
    front = np.zeros(n, dtype=np.int32)
    ts = abi.CTrackBatchSummary()
    st = L.tmi_ba_optimize_relative_positions(C.byref(cb), int(device), status.ctypes.data, iters.ctypes.data,
                                              cost.ctypes.data, front.ctypes.data, C.byref(ts))
    if st != 0:
        raise EngineError(st, "tmi_ba_optimize_relative_positions")
    return status, iters, cost, front, ts


def filter_view_pairs_from_relative_translation(batch: abi.ViewPairBatch, options=None, axes=None, device: int = -1):
    """The 1DSfM filter (FilterViewPairsFromRelativeTranslation) on the device.  options: a
    CTranslationFilterOptions (default: the reference's).  axes: [num_iterations, 3] projection axes to use as they
    are, or None: the engine draws them from options.seed.
    Returns (removed [P] uint8, bad_weight [P], rotated_translation [P, 3], iteration_order [iterations, V] int32,
    axes [iterations, 3] as used, CViewPairFilterSummary)."""
    L = load()
    o = options if options is not None else abi.translation_filter_options()
    K, n, V = max(int(o.num_iterations), 0), batch.num_pairs, batch.num_views
    given = axes is not None
    ax = np.ascontiguousarray(axes, dtype=np.float64).reshape(-1, 3).copy() if given else np.zeros((K, 3))
    if given and ax.shape[0] != K:
        raise ValueError("axes must hold options.num_iterations rows")
    cb = batch.as_c()
    removed = np.zeros(n, dtype=np.uint8)
    weight = np.zeros(n)
    rotated = np.zeros((n, 3))
    order = np.full((K, V), -1, dtype=np.int32)
    fs = abi.CViewPairFilterSummary()
    st = L.tmi_ba_filter_view_pairs_from_relative_translation(
        C.byref(cb), C.byref(o), ax.ctypes.data, 1 if given else 0, int(device), removed.ctypes.data,
        weight.ctypes.data, rotated.ctypes.data, order.ctypes.data, C.byref(fs))
    if st != 0:
        raise EngineError(st, "tmi_ba_filter_view_pairs_from_relative_translation")
    return removed, weight, rotated, order, ax, fs


def filter_view_pairs_from_orientation(batch: abi.ViewPairBatch, max_relative_rotation_difference_degrees: float,
                                       device: int = -1):
    """FilterViewPairsFromOrientation on the device.
    Returns (removed [P] uint8, angle [P] in radians, CViewPairFilterSummary)."""
    L = load()
    cb = batch.as_c()
    n = batch.num_pairs
    removed = np.zeros(n, dtype=np.uint8)
    angle = np.zeros(n)
    fs = abi.CViewPairFilterSummary()
    st = L.tmi_ba_filter_view_pairs_from_orientation(C.byref(cb), float(max_relative_rotation_difference_degrees),
                                                     int(device), removed.ctypes.data, angle.ctypes.data,
                                                     C.byref(fs))
    if st != 0:
        raise EngineError(st, "tmi_ba_filter_view_pairs_from_orientation")
    return removed, angle, fs


def _mask_pointer(pair_mask, n):
    if pair_mask is None:
        return None, None
    m = np.ascontiguousarray(pair_mask, dtype=np.uint8)
    if m.shape != (n,):
        raise ValueError("pair_mask must hold one entry per pair")
    return m, m.ctypes.data


def largest_connected_component(batch: abi.ViewPairBatch, pair_mask=None, device: int = -1):
    """The component step of RemoveDisconnectedViewPairs on the device.  pair_mask [P]: 0 = the edge is not there.
    Returns (view_label [V] int32, view_in_largest [V] uint8, pair_keep [P] uint8, CViewGraphComponentSummary)."""
    L = load()
    cb = batch.as_c()
    n, V = batch.num_pairs, batch.num_views
    mask, mask_p = _mask_pointer(pair_mask, n)
    label = np.full(V, -1, dtype=np.int32)
    in_largest = np.zeros(V, dtype=np.uint8)
    keep = np.zeros(n, dtype=np.uint8)
    cs = abi.CViewGraphComponentSummary()
    st = L.tmi_ba_largest_connected_component(C.byref(cb), mask_p, int(device), label.ctypes.data,
                                              in_largest.ctypes.data, keep.ctypes.data, C.byref(cs))
    if st != 0:
        raise EngineError(st, "tmi_ba_largest_connected_component")
    return label, in_largest, keep, cs


def orientations_from_maximum_spanning_tree(batch: abi.ViewPairBatch, pair_num_verified_matches, pair_mask=None,
                                            root_view: int = -1, device: int = -1, view_orientation=None):
    """OrientationsFromMaximumSpanningTree on the device (batch.pair_rotation2 holds the relative rotations).
    view_orientation [V, 3]: the values the views outside the tree keep (default: NaN).
    Returns a dict: orientation [V, 3], parent, parent_pair, depth [V] int32, in_tree [P] uint8, summary
    (CSpanningTreeSummary).  Raises EngineError on any failure."""
    L = load()
    cb = batch.as_c()
    n, V = batch.num_pairs, batch.num_views
    mask, mask_p = _mask_pointer(pair_mask, n)
    w = np.ascontiguousarray(pair_num_verified_matches, dtype=np.int32)
    if w.shape != (n,):
        raise ValueError("pair_num_verified_matches must hold one entry per pair")
    o = np.full((V, 3), np.nan) if view_orientation is None else \
        np.ascontiguousarray(view_orientation, dtype=np.float64).reshape(V, 3).copy()
    parent = np.full(V, -1, dtype=np.int32)
    parent_pair = np.full(V, -1, dtype=np.int32)
    depth = np.full(V, -1, dtype=np.int32)
    in_tree = np.zeros(n, dtype=np.uint8)
    ts = abi.CSpanningTreeSummary()
    st = L.tmi_ba_orientations_from_maximum_spanning_tree(
        C.byref(cb), w.ctypes.data, mask_p, int(root_view), int(device), o.ctypes.data, parent.ctypes.data,
        parent_pair.ctypes.data, depth.ctypes.data, in_tree.ctypes.data, C.byref(ts))
    if st != 0:
        raise EngineError(st, "tmi_ba_orientations_from_maximum_spanning_tree")
    return dict(orientation=o, parent=parent, parent_pair=parent_pair, depth=depth, in_tree=in_tree, summary=ts)


def estimate_global_rotations_robust(batch: abi.RelativeRotationBatch, view_rotation, fixed_view: int = 0, options=None,
                                     device: int = -1):
    """RobustRotationEstimator::EstimateRotations on the device.  view_rotation [V, 3]: the initial orientations (not
    modified).  options: a CRobustRotationOptions (default: the reference's).
    Returns a dict: rotations [V, 3], residuals [P, 3], admm_iterations (per outer L1 iteration run), l1_steps,
    irls_steps, irls_sq_residuals, summary (CRobustRotationSummary).  Raises EngineError on any failure."""
    L = load()
    o = options if options is not None else abi.robust_rotation_options()
    rot = np.array(view_rotation, dtype=np.float64).reshape(-1, 3)
    if rot.shape[0] != batch.num_views:
        raise ValueError("view_rotation must hold batch.num_views rows")
    n1, n2 = max(int(o.max_num_l1_iterations), 0), max(int(o.max_num_irls_iterations), 0)
    res = np.zeros((batch.num_pairs, 3))
    admm = np.zeros(max(n1, 1), dtype=np.int32)
    l1_steps, irls_steps, irls_sq = np.zeros(max(n1, 1)), np.zeros(max(n2, 1)), np.zeros(max(n2, 1))
    cb = batch.as_c()
    rs = abi.CRobustRotationSummary()
    st = L.tmi_ba_estimate_global_rotations_robust(
        C.byref(cb), C.byref(o), int(fixed_view), int(device), rot.ctypes.data, res.ctypes.data, admm.ctypes.data,
        l1_steps.ctypes.data, irls_steps.ctypes.data, irls_sq.ctypes.data, C.byref(rs))
    if st != 0:
        raise EngineError(st, "tmi_ba_estimate_global_rotations_robust")
    k1, k2 = rs.num_l1_iterations, rs.num_irls_iterations
    return dict(rotations=rot, residuals=res, admm_iterations=[int(x) for x in admm[:k1]], l1_steps=list(l1_steps[:k1]),
                irls_steps=list(irls_steps[:k2]), irls_sq_residuals=list(irls_sq[:k2]), summary=rs)


def estimate_global_positions_lud(batch: abi.ViewPairBatch, fixed_view: int = 0, options=None, device: int = -1):
    """LeastUnsquaredDeviationPositionEstimator::EstimatePositions on the device.  batch.view_rotation None:
    batch.pair_position2 is already in the global frame.  options: a CLudPositionOptions (default: the reference's).
    Returns a dict: positions [V, 3] (the fixed view at 0), scales [P], residuals [P, 3] (the final A x of the L1 rows),
    r_norms, s_norms (per ADMM iteration run), summary (CLudPositionSummary).  Raises EngineError on any failure."""
    L = load()
    o = options if options is not None else abi.lud_position_options()
    k = max(int(o.max_num_iterations), 1)
    pos = np.zeros((batch.num_views, 3))
    scales = np.zeros(batch.num_pairs)
    res = np.zeros((batch.num_pairs, 3))
    r_norms, s_norms = np.zeros(k), np.zeros(k)
    cb = batch.as_c()
    ps = abi.CLudPositionSummary()
    st = L.tmi_ba_estimate_global_positions_lud(
        C.byref(cb), C.byref(o), int(fixed_view), int(device), pos.ctypes.data, scales.ctypes.data, res.ctypes.data,
        r_norms.ctypes.data, s_norms.ctypes.data, C.byref(ps))
    if st != 0:
        raise EngineError(st, "tmi_ba_estimate_global_positions_lud")
    ran = ps.num_admm_iterations
    return dict(positions=pos, scales=scales, residuals=res, r_norms=r_norms[:ran].copy(), s_norms=s_norms[:ran].copy(),
                summary=ps)


def estimate_global_positions_nonlinear(batch: abi.ViewPairBatch, fixed_view: int = 0, options=None, device: int = -1,
                                        start=None):
    """NonlinearPositionEstimator::EstimatePositions on the device.  batch.view_rotation None: batch.pair_position2 is
    already in the global frame.  options: a CNonlinearPositionOptions (default: the reference's).  start [V, 3]: the
    positions to start from, required exactly when options.positions_given (not modified).
    Returns a dict: positions [V, 3] (the fixed view at 0), initial_positions [V, 3], residuals [P, 3], costs, radii and
    outcomes (entry 0 the start, then one per iteration run: 1 accepted, 0 rejected, -1 invalid, 2 / 3 ended by the
    parameter / function tolerance), summary (CNonlinearPositionSummary).  Raises EngineError on any failure."""
    L = load()
    o = options if options is not None else abi.nonlinear_position_options()
    if bool(o.positions_given) != (start is not None):
        raise ValueError("start goes with options.positions_given")
    k = max(int(o.max_num_iterations), 0) + 1
    pos = np.zeros((batch.num_views, 3)) if start is None else np.array(start, dtype=np.float64).reshape(-1, 3)
    if pos.shape[0] != batch.num_views:
        raise ValueError("start must hold batch.num_views rows")
    initial = np.zeros((batch.num_views, 3))
    res = np.zeros((batch.num_pairs, 3))
    costs, radii, outcomes = np.zeros(k), np.zeros(k), np.zeros(k, dtype=np.int32)
    cb = batch.as_c()
    ps = abi.CNonlinearPositionSummary()
    st = L.tmi_ba_estimate_global_positions_nonlinear(
        C.byref(cb), C.byref(o), int(fixed_view), int(device), pos.ctypes.data, initial.ctypes.data, costs.ctypes.data,
        radii.ctypes.data, outcomes.ctypes.data, res.ctypes.data, C.byref(ps))
    if st != 0:
        raise EngineError(st, "tmi_ba_estimate_global_positions_nonlinear")
    ran = ps.num_iterations + 1
    return dict(positions=pos, initial_positions=initial, residuals=res, costs=costs[:ran].copy(),
                radii=radii[:ran].copy(), outcomes=outcomes[:ran].copy(), summary=ps)


def estimate_global_positions_linear(problem: abi.Problem, batch: abi.ViewPairBatch, options=None, device: int = -1,
                                      triplet_capacity=None, view_position=None, view_estimated=None):
    """LinearPositionEstimator::EstimatePositions on the device.  problem: the cameras of every view (camera i is view
    i) and all observations.  batch: the pairs (view1 < view2), pair_rotation2, pair_position2 and view_rotation, the
    global orientations.  options: a CLinearPositionOptions (default: tmi_ba_linear_position_options_init's).
    triplet_capacity: room of the optional triplet arrays (0: not asked for).  None runs the WHOLE call twice, once to
    learn summary.num_triplets and once with that capacity: convenient for tests, twice the cost; a caller who times
    the call or knows a bound passes a capacity.
    view_position [V, 3] / view_estimated [V]: what the arrays hold where the call writes nothing (default zeros).
    Returns a dict: positions [V, 3], estimated [V] uint8, summary (CLinearPositionSummary) and, where
    summary.triplets_written, triplet_view [T, 3], triplet_pair [T, 3], triplet_baseline [T, 3], triplet_num_common,
    triplet_num_used, triplet_component [T] (else None each).  Raises EngineError on any failure."""
    L = load()
    o = options if options is not None else abi.linear_position_options()
    V = batch.num_views
    cp, cb = problem.as_c(), batch.as_c()

    def call(capacity):
        pos = np.zeros((V, 3)) if view_position is None else np.array(view_position, dtype=np.float64).reshape(V, 3)
        est = np.zeros(V, dtype=np.uint8) if view_estimated is None else np.array(view_estimated, dtype=np.uint8).reshape(V)
        tv, tp = np.zeros((capacity, 3), dtype=np.int32), np.zeros((capacity, 3), dtype=np.int32)
        tb = np.zeros((capacity, 3))
        tc, tu, tl = (np.zeros(capacity, dtype=np.int32) for _ in range(3))
        ps = abi.CLinearPositionSummary()
        ptr = (lambda a: a.ctypes.data) if capacity > 0 else (lambda a: None)
        st = L.tmi_ba_estimate_global_positions_linear(
            C.byref(cp), C.byref(cb), C.byref(o), int(device), pos.ctypes.data, est.ctypes.data, int(capacity), ptr(tv),
            ptr(tp), ptr(tb), ptr(tc), ptr(tu), ptr(tl), C.byref(ps))
        if st != 0:
            raise EngineError(st, "tmi_ba_estimate_global_positions_linear")
        return pos, est, (tv, tp, tb, tc, tu, tl), ps

    pos, est, trip, ps = call(0 if triplet_capacity is None else int(triplet_capacity))
    if triplet_capacity is None and ps.num_triplets > 0:
        pos, est, trip, ps = call(ps.num_triplets)
    T = ps.num_triplets
    written = bool(ps.triplets_written) and (triplet_capacity is None or int(triplet_capacity) > 0)
    names = ("triplet_view", "triplet_pair", "triplet_baseline", "triplet_num_common", "triplet_num_used",
             "triplet_component")
    out = dict(positions=pos, estimated=est, summary=ps)
    out.update({k: (a[:T].copy() if written else None) for k, a in zip(names, trip)})
    return out


def estimate_global_rotations_nonlinear(batch: abi.ViewPairBatch, view_rotation, options=None, view_given=None,
                                        device: int = -1, want_outputs: bool = True):
    """NonlinearRotationEstimator::EstimateRotations on the device.  batch: num_views, the pairs and pair_rotation2 are
    read.  view_rotation [V, 3]: the start (not modified).  options: a CNonlinearRotationOptions (default: the
    reference's, fixed_view = -1).  view_given [V] (None: every view): the views that have an initialisation; the others
    come back as they were.  want_outputs False passes NULL for every optional output.
    Returns a dict: rotations [V, 3], summary (CNonlinearRotationSummary) and, with want_outputs, residuals [P, 3] (0 for
    a skipped edge), costs, radii and outcomes (entry 0 the start, then one per iteration run: 1 accepted, 0 rejected,
    -1 invalid, 2 / 3 ended by the parameter / function tolerance).  Raises EngineError on any failure."""
    L = load()
    o = options if options is not None else abi.nonlinear_rotation_options()
    rot = np.array(view_rotation, dtype=np.float64).reshape(-1, 3)
    if rot.shape[0] != batch.num_views:
        raise ValueError("view_rotation must hold batch.num_views rows")
    given = None if view_given is None else np.ascontiguousarray(view_given, dtype=np.uint8)
    if given is not None and given.shape != (batch.num_views,):
        raise ValueError("view_given must hold batch.num_views entries")
    k = max(int(o.max_num_iterations), 0) + 1
    res = np.zeros((batch.num_pairs, 3))
    costs, radii, outcomes = np.zeros(k), np.zeros(k), np.zeros(k, dtype=np.int32)
    cb = batch.as_c()
    rs = abi.CNonlinearRotationSummary()
    ptr = (lambda a: a.ctypes.data) if want_outputs else (lambda a: None)
    st = L.tmi_ba_estimate_global_rotations_nonlinear(
        C.byref(cb), C.byref(o), None if given is None else given.ctypes.data, int(device), rot.ctypes.data, ptr(costs),
        ptr(radii), ptr(outcomes), ptr(res), C.byref(rs))
    if st != 0:
        raise EngineError(st, "tmi_ba_estimate_global_rotations_nonlinear")
    out = dict(rotations=rot, summary=rs)
    if want_outputs:
        ran = rs.num_iterations + 1
        out.update(residuals=res, costs=costs[:ran].copy(), radii=radii[:ran].copy(), outcomes=outcomes[:ran].copy())
    return out


def estimate_global_rotations_linear(batch: abi.ViewPairBatch, options=None, device: int = -1, view_rotation=None):
    """LinearRotationEstimator::EstimateRotations on the device.  batch: num_views, the pairs and pair_rotation2 are
    read.  options: a CLinearRotationOptions (default: tmi_ba_linear_rotation_options_init's).  view_rotation [V, 3]
    (default zeros, not modified): what the views without an edge keep -- there is no start.
    Returns a dict: rotations [V, 3] and summary (CLinearRotationSummary); with summary.usable == 0 the rotations are
    as given.  Raises EngineError on any failure."""
    L = load()
    o = options if options is not None else abi.linear_rotation_options()
    rot = (np.zeros((batch.num_views, 3)) if view_rotation is None
           else np.array(view_rotation, dtype=np.float64).reshape(-1, 3))
    if rot.shape[0] != batch.num_views:
        raise ValueError("view_rotation must hold batch.num_views rows")
    cb = batch.as_c()
    rs = abi.CLinearRotationSummary()
    st = L.tmi_ba_estimate_global_rotations_linear(C.byref(cb), C.byref(o), int(device), rot.ctypes.data, C.byref(rs))
    if st != 0:
        raise EngineError(st, "tmi_ba_estimate_global_rotations_linear")
    return dict(rotations=rot, summary=rs)


def extract_parallel_rigid_subgraph(batch: abi.ViewPairBatch, options=None, view_mask=None,
                                    want_null_space: bool = False, outputs=None):
    """ExtractMaximallyParallelRigidSubgraph on the device.  batch: view_rotation (the orientations), the pairs and
    pair_position2 are read.  options: a CRigidSubgraphOptions (default: tmi_ba_rigid_subgraph_options_init's).
    view_mask [V]: 0 = the view and its edges are not there.  outputs: a dict with keep [V] uint8, component_size [V]
    int32 and (with want_null_space) null_space [3 V * max_null_dimension] float64 to write into (default: fresh
    zeros) -- a failure leaves them as they were.
    Returns a dict: keep [V] uint8, component_size [V] int32, null_space [n, k] (None unless asked for) and summary
    (CRigidSubgraphSummary).  Raises EngineError on any failure; the error carries .summary."""
    L = load()
    o = options if options is not None else abi.rigid_subgraph_options()
    V = batch.num_views
    if batch.view_rotation is None:
        raise ValueError("the batch needs view_rotation: the orientations")
    mask, mask_p = _mask_pointer(view_mask, V) if view_mask is not None else (None, None)
    out = outputs if outputs is not None else {}
    keep = out.get("keep", np.zeros(V, dtype=np.uint8))
    size = out.get("component_size", np.zeros(V, dtype=np.int32))
    null = out.get("null_space", np.zeros(3 * V * max(int(o.max_null_dimension), 1))) if want_null_space else None
    if keep.dtype != np.uint8 or keep.shape != (V,) or size.dtype != np.int32 or size.shape != (V,):
        raise ValueError("keep must be [V] uint8 and component_size [V] int32")
    cb = batch.as_c()
    rs = abi.CRigidSubgraphSummary()
    st = L.tmi_ba_extract_parallel_rigid_subgraph(C.byref(cb), mask_p, C.byref(o), keep.ctypes.data, size.ctypes.data,
                                                  null.ctypes.data if null is not None else None, C.byref(rs))
    if st != 0:
        err = EngineError(st, "tmi_ba_extract_parallel_rigid_subgraph")
        err.summary = rs
        raise err
    n, k = int(rs.order), int(rs.null_dimension)
    return dict(keep=keep, component_size=size, null_space=None if null is None else null[:n * k].reshape(n, k).copy(),
                summary=rs)


def localize_views(problem: abi.Problem, view_error_threshold, options=None, ba_options=None, view_mask=None,
                   samples=None, want_hypothesis_cost: bool = False):
    """Batched LocalizeViewToReconstruction (calibrated path: P3P RANSAC, then the batched BundleAdjustView) over the
    views view_mask selects (None = all).  view_error_threshold [Nc]: the squared threshold in normalised coordinates.
    samples: optional [Nc, max_iterations, 3] int32 sample table (otherwise drawn from options.seed).
    problem.extrinsics (and, with the adjustment, free intrinsics) are updated in place for the localised views.
    Returns a dict: status [Nc] int8, num_correspondences, num_inliers, num_iterations, best_iteration, best_solution
    [Nc] int32, confidence [Nc], obs_inlier [No] uint8, hypothesis_cost [num_selected, max_iterations, 4] int32 or
    None, summary (CLocalizationSummary).  Raises EngineError on any failure."""
    L = load()
    o = options if options is not None else abi.localization_options()
    bo = ba_options if ba_options is not None else abi.default_options()
    nc = problem.num_cameras
    vm = None if view_mask is None else np.ascontiguousarray(view_mask, dtype=np.uint8)
    if vm is not None and vm.shape != (nc,):
        raise ValueError(f"view_mask must have num_cameras = {nc} entries")
    th = None if view_error_threshold is None else np.ascontiguousarray(view_error_threshold, dtype=np.float64)
    if th is not None and th.shape != (nc,):
        raise ValueError(f"view_error_threshold must have num_cameras = {nc} entries")
    k = max(int(o.max_iterations), 0)
    sm = None
    if samples is not None:
        sm = np.ascontiguousarray(samples, dtype=np.int32)
        if sm.shape != (nc, k, 3):
            raise ValueError(f"samples must have shape (num_cameras, max_iterations, 3) = ({nc}, {k}, 3)")
    nsel = nc if vm is None else int(np.count_nonzero(vm))
    status = np.full(nc, -1, dtype=np.int8)
    i32 = [np.zeros(nc, dtype=np.int32) for _ in range(5)]
    conf = np.zeros(nc)
    inl = np.zeros(problem.num_observations, dtype=np.uint8)
    hyp = np.full((nsel, min(k, 1 << 20), 4), -1, dtype=np.int32) if want_hypothesis_cost else None
    cp = problem.as_c()
    zs = abi.CLocalizationSummary()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    st = L.tmi_ba_localize_views(C.byref(cp), C.byref(o), C.byref(bo), ptr(vm), ptr(th), ptr(sm),
                                 0 if sm is None else 1, status.ctypes.data, *[a.ctypes.data for a in i32],
                                 conf.ctypes.data, inl.ctypes.data, ptr(hyp), C.byref(zs))
    if st != 0:
        raise EngineError(st, "tmi_ba_localize_views")
    return dict(status=status, num_correspondences=i32[0], num_inliers=i32[1], num_iterations=i32[2],
                best_iteration=i32[3], best_solution=i32[4], confidence=conf, obs_inlier=inl, hypothesis_cost=hyp,
                summary=zs)


def _match_call(entry, summary_type, default_options, image_begin, descriptors, projections, pair_image1, pair_image2,
                options, match_capacity, want_hash):
    """The wrapper tmi_ba_match_features and tmi_ba_match_features_cascade share (projections is None for the first)."""
    L = load()
    o = options if options is not None else default_options()
    ib = np.ascontiguousarray(image_begin, dtype=np.int64)
    desc = np.ascontiguousarray(descriptors, dtype=np.float32)
    if ib.ndim != 1 or ib.shape[0] < 1:
        raise ValueError("image_begin must have num_images + 1 entries")
    if desc.ndim != 2:
        raise ValueError("descriptors must be [rows, dim]")
    p1 = np.ascontiguousarray(pair_image1, dtype=np.int32)
    p2 = np.ascontiguousarray(pair_image2, dtype=np.int32)
    if p1.ndim != 1 or p1.shape != p2.shape:
        raise ValueError("pair_image1 and pair_image2 must be one-dimensional and of one length")
    if desc.shape[0] != int(ib[-1]):
        raise ValueError("descriptors must have image_begin[-1] rows")
    num_images, num_pairs = ib.shape[0] - 1, p1.shape[0]
    if match_capacity is None:
        ok = (p1 >= 0) & (p1 < num_images)
        n1 = np.diff(ib)[p1[ok]] if num_images else np.zeros(0, np.int64)
        cap = int(np.maximum(n1, 0).sum())
    else:
        cap = int(match_capacity)
    status = np.zeros(num_pairs, dtype=np.int8)
    nfwd = np.zeros(num_pairs, dtype=np.int32)
    begin = np.zeros(num_pairs + 1, dtype=np.int64)
    f1 = np.zeros(max(cap, 0), dtype=np.int32)
    f2 = np.zeros(max(cap, 0), dtype=np.int32)
    dist = np.zeros(max(cap, 0), dtype=np.float32)
    ms = summary_type()
    extra = {}
    if projections is None:
        st = L.tmi_ba_match_features(C.byref(o), num_images, ib.ctypes.data, desc.ctypes.data, desc.shape[1], num_pairs,
                                     p1.ctypes.data, p2.ctypes.data, cap, status.ctypes.data, nfwd.ctypes.data,
                                     begin.ctypes.data, f1.ctypes.data, f2.ctypes.data, dist.ctypes.data, C.byref(ms))
    else:
        proj = np.ascontiguousarray(projections, dtype=np.float32)
        if proj.shape != (188, desc.shape[1]):
            raise ValueError("projections must be [188, dim]")
        code = np.zeros((desc.shape[0], 4), dtype=np.uint32) if want_hash else None
        ids = np.zeros((desc.shape[0], 6), dtype=np.uint16) if want_hash else None
        st = L.tmi_ba_match_features_cascade(
            C.byref(o), num_images, ib.ctypes.data, desc.ctypes.data, desc.shape[1], proj.ctypes.data, num_pairs,
            p1.ctypes.data, p2.ctypes.data, cap, status.ctypes.data, nfwd.ctypes.data, begin.ctypes.data, f1.ctypes.data,
            f2.ctypes.data, dist.ctypes.data, code.ctypes.data if want_hash else None,
            ids.ctypes.data if want_hash else None, C.byref(ms))
        extra = dict(image_hash=code, image_bucket_ids=ids)
    if st not in (0, abi.ERR_CAPACITY):
        raise EngineError(st, entry)
    n = 0 if st else int(begin[-1])
    return dict(status=st, pair_status=status, pair_num_forward=nfwd, pair_match_begin=begin, feature1=f1[:n],
                feature2=f2[:n], distance=dist[:n], summary=ms, **extra)


def match_features(image_begin, descriptors, pair_image1, pair_image2, options=None, match_capacity=None):
    """Batched BruteForceFeatureMatcher (exact fp32 squared-L2 matching, ratio test, symmetric intersection) over the
    image pairs (pair_image1[p], pair_image2[p]).  image_begin [num_images + 1] int64 row offsets into descriptors
    [rows, dim] float32.  match_capacity: None sizes the match arrays for the most the options allow (the rows of
    image 1 over the pairs); a number is passed through, and a capacity that is too small comes back as `status` ==
    abi.ERR_CAPACITY with the per-pair arrays filled and summary.num_matches the needed total.
    Returns a dict: status (the call's), pair_status [P] int8, pair_num_forward [P] int32, pair_match_begin [P + 1]
    int64, feature1 / feature2 [total] int32, distance [total] float32, summary (CMatchSummary).  Raises EngineError
    on any other failure."""
    return _match_call("tmi_ba_match_features", abi.CMatchSummary, abi.match_options, image_begin, descriptors, None,
                       pair_image1, pair_image2, options, match_capacity, False)


def match_features_cascade(image_begin, descriptors, projections, pair_image1, pair_image2, options=None,
                           match_capacity=None, want_hash=False):
    """Batched CascadeHashingFeatureMatcher (tmi_ba_match_features_cascade): the arguments and the returned dict of
    match_features, plus projections [188, dim] float32 (rows 0..127 the primary projection, row 128 + 10 g + k bit k
    of bucket group g; synth.cascade_projections draws them) and options from abi.cascade_match_options().
    want_hash adds image_hash [rows, 4] uint32 and image_bucket_ids [rows, 6] uint16 (None otherwise).  summary is a
    CCascadeMatchSummary."""
    return _match_call("tmi_ba_match_features_cascade", abi.CCascadeMatchSummary, abi.cascade_match_options,
                       image_begin, descriptors, projections, pair_image1, pair_image2, options, match_capacity,
                       bool(want_hash))


def guided_epipolar_match(image_begin, descriptors, keypoints, pair_image1, pair_image2, fundamental_matrix,
                          pair_match_begin, match_feature1, match_feature2, options=None, pair_mask=None,
                          pair_stream=None, added_capacity=None, want_groups=False):
    """Batched GuidedEpipolarMatcher (tmi_ba_guided_epipolar_match): more matches along the epipolar lines of the pairs
    (pair_image1[p], pair_image2[p]).  image_begin [num_images + 1] int64 row offsets into descriptors [rows, dim]
    float32 and keypoints [rows, 2] float64; fundamental_matrix [P, 9] (row-major, image-1 point to image-2 line);
    the input matches of pair p are pair_match_begin[p] .. pair_match_begin[p + 1] - 1 of match_feature1 /
    match_feature2.  added_capacity: None sizes the arrays for the most there can be (the rows of image 1 over the
    pairs); a capacity that is too small comes back as `status` == abi.ERR_CAPACITY with summary.num_added the needed
    total.  want_groups adds the test outputs.
    Returns a dict: status, pair_status [P] int8, pair_num_groups [P] int32, pair_added_begin [P + 1] int64, feature1 /
    feature2 [total] int32, distance [total] float32, summary (CGuidedMatchSummary) and, with want_groups, pair_row
    [P + 1] int64 (row(p) of the header), feature_group, group_endpoints [rows, 4], group_num_candidates.  Raises
    EngineError on any other failure."""
    L = load()
    o = options if options is not None else abi.guided_match_options()
    ib = np.ascontiguousarray(image_begin, dtype=np.int64)
    desc = np.ascontiguousarray(descriptors, dtype=np.float32)
    keys = np.ascontiguousarray(keypoints, dtype=np.float64)
    if ib.ndim != 1 or ib.shape[0] < 1:
        raise ValueError("image_begin must have num_images + 1 entries")
    if desc.ndim != 2 or desc.shape[0] != int(ib[-1]):
        raise ValueError("descriptors must be [image_begin[-1], dim]")
    if keys.shape != (desc.shape[0], 2):
        raise ValueError("keypoints must be [rows, 2]")
    p1 = np.ascontiguousarray(pair_image1, dtype=np.int32)
    p2 = np.ascontiguousarray(pair_image2, dtype=np.int32)
    if p1.ndim != 1 or p1.shape != p2.shape:
        raise ValueError("pair_image1 and pair_image2 must be one-dimensional and of one length")
    num_images, num_pairs = ib.shape[0] - 1, p1.shape[0]
    F = np.ascontiguousarray(fundamental_matrix, dtype=np.float64).reshape(-1)
    if F.shape[0] != 9 * num_pairs:
        raise ValueError("fundamental_matrix must be [num_pairs, 9]")
    mb = np.ascontiguousarray(pair_match_begin, dtype=np.int64)
    m1 = np.ascontiguousarray(match_feature1, dtype=np.int32)
    m2 = np.ascontiguousarray(match_feature2, dtype=np.int32)
    if mb.shape != (num_pairs + 1,) or m1.ndim != 1 or m1.shape != m2.shape:
        raise ValueError("pair_match_begin must have num_pairs + 1 entries and the match arrays one length")
    if mb.shape[0] and int(mb.max()) > m1.shape[0]:
        raise ValueError("pair_match_begin points past the match arrays")
    mask = None if pair_mask is None else np.ascontiguousarray(pair_mask, dtype=np.uint8)
    strm = None if pair_stream is None else np.ascontiguousarray(pair_stream, dtype=np.uint32)
    for a in (mask, strm):
        if a is not None and a.shape != (num_pairs,):
            raise ValueError("pair_mask and pair_stream must have num_pairs entries")
    ok = (p1 >= 0) & (p1 < num_images)
    n1 = np.where(ok, np.diff(ib)[np.where(ok, p1, 0)], 0) if num_images else np.zeros(num_pairs, np.int64)
    pair_row = np.concatenate([[0], np.cumsum(np.maximum(n1, 0))]).astype(np.int64)
    rows = int(pair_row[-1])
    cap = rows if added_capacity is None else int(added_capacity)
    status = np.zeros(num_pairs, dtype=np.int8)
    ngroups = np.zeros(num_pairs, dtype=np.int32)
    begin = np.zeros(num_pairs + 1, dtype=np.int64)
    f1 = np.zeros(max(cap, 0), dtype=np.int32)
    f2 = np.zeros(max(cap, 0), dtype=np.int32)
    dist = np.zeros(max(cap, 0), dtype=np.float32)
    fg = np.zeros(rows, dtype=np.int32) if want_groups else None
    ge = np.zeros((rows, 4), dtype=np.float64) if want_groups else None
    gn = np.zeros(rows, dtype=np.int32) if want_groups else None
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    gs = abi.CGuidedMatchSummary()
    st = L.tmi_ba_guided_epipolar_match(
        C.byref(o), num_images, ib.ctypes.data, desc.ctypes.data, desc.shape[1], keys.ctypes.data, num_pairs,
        p1.ctypes.data, p2.ctypes.data, F.ctypes.data, mb.ctypes.data, m1.ctypes.data, m2.ctypes.data, ptr(mask),
        ptr(strm), cap, status.ctypes.data, ngroups.ctypes.data, begin.ctypes.data, f1.ctypes.data, f2.ctypes.data,
        dist.ctypes.data, ptr(fg), ptr(ge), ptr(gn), C.byref(gs))
    if st not in (0, abi.ERR_CAPACITY):
        raise EngineError(st, "tmi_ba_guided_epipolar_match")
    n = 0 if st else int(begin[-1])
    out = dict(status=st, pair_status=status, pair_num_groups=ngroups, pair_added_begin=begin, feature1=f1[:n],
               feature2=f2[:n], distance=dist[:n], summary=gs, added_arrays=(f1, f2, dist))
    if want_groups:
        out.update(pair_row=pair_row, feature_group=fg, group_endpoints=ge, group_num_candidates=gn)
    return out


def build_tracks(endpoint_view, endpoint_feature, options=None, track_capacity=None, obs_capacity=None,
                 want_nodes=False):
    """TrackBuilder on the device (tmi_ba_build_tracks): the tracks of the correspondences whose edge e joins the
    endpoints 2e and 2e + 1 of endpoint_view / endpoint_feature [2E] uint32 (a feature index is local to its view).
    options: abi.track_build_options().  track_capacity / obs_capacity: None sizes the outputs for the most there can
    be (E tracks, 2E observations); a number is passed through, and a capacity that is too small comes back as
    `status` == abi.ERR_CAPACITY with empty outputs and the needed totals in summary.num_tracks / num_observations.
    Returns a dict: status, track_begin [num_tracks + 1] int64, obs_view / obs_feature [num_observations] uint32,
    summary (CTrackBuildSummary) and, with want_nodes, endpoint_node / endpoint_label [2E] uint32 (None otherwise).
    Raises EngineError on any other failure."""
    L = load()
    o = options if options is not None else abi.track_build_options()
    ev = np.ascontiguousarray(endpoint_view, dtype=np.uint32)
    ef = np.ascontiguousarray(endpoint_feature, dtype=np.uint32)
    if ev.ndim != 1 or ev.shape != ef.shape or ev.shape[0] % 2:
        raise ValueError("endpoint_view and endpoint_feature must be [2E]")
    E = ev.shape[0] // 2
    tcap = E if track_capacity is None else int(track_capacity)
    ocap = 2 * E if obs_capacity is None else int(obs_capacity)
    begin = np.zeros(max(tcap, 0) + 1, dtype=np.int64)
    ov = np.zeros(max(ocap, 0), dtype=np.uint32)
    of = np.zeros(max(ocap, 0), dtype=np.uint32)
    node = np.zeros(2 * E, dtype=np.uint32) if want_nodes else None
    label = np.zeros(2 * E, dtype=np.uint32) if want_nodes else None
    ts = abi.CTrackBuildSummary()
    st = L.tmi_ba_build_tracks(C.byref(o), E, ev.ctypes.data, ef.ctypes.data, tcap, ocap, begin.ctypes.data,
                               ov.ctypes.data, of.ctypes.data, node.ctypes.data if want_nodes else None,
                               label.ctypes.data if want_nodes else None, C.byref(ts))
    if st not in (0, abi.ERR_CAPACITY):
        raise EngineError(st, "tmi_ba_build_tracks")
    nt = 0 if st else int(ts.num_tracks)
    no = 0 if st else int(ts.num_observations)
    return dict(status=st, track_begin=begin[:nt + 1], obs_view=ov[:no], obs_feature=of[:no], endpoint_node=node,
                endpoint_label=label, summary=ts)


def estimate_uncalibrated_relative_poses(pair_offset, feature1, feature2, pair_error_threshold, options=None,
                                         pair_mask=None, pair_stream=None, samples=None,
                                         want_hypothesis_cost: bool = False):
    """Batched EstimateUncalibratedRelativePose (the uncalibrated branch of EstimateTwoViewInfo: eight-point RANSAC, the
    focal lengths from F, the pose from E) over the pairs pair_mask selects (None = all).  pair_offset [P + 1] int64;
    feature1 / feature2 [N, 2] CENTRED pixels; pair_error_threshold [P] the squared threshold in pixels^2.
    pair_stream: optional [P] uint32 sample-stream ids (None: the pair index).  samples: optional
    [P, max_iterations, 8] int32 sample table (otherwise drawn from options.seed).
    Returns a dict: status [P] int8, num_correspondences, num_inliers, num_iterations, best_iteration [P] int32,
    confidence [P], fundamental_matrix [P, 9] (column-major), focal_length1 / focal_length2 [P], rotation / position
    [P, 3], corr_inlier [N] uint8, hypothesis_cost [num_selected, max_iterations] int32 or None, summary
    (CTwoViewRansacSummary).  Raises EngineError on any failure."""
    L = load()
    o = options if options is not None else abi.two_view_ransac_options()
    po = np.ascontiguousarray(pair_offset, dtype=np.int64)
    if po.ndim != 1 or po.shape[0] < 1:
        raise ValueError("pair_offset must have num_pairs + 1 entries")
    npair = po.shape[0] - 1
    f1 = np.ascontiguousarray(feature1, dtype=np.float64).reshape(-1, 2)
    f2 = np.ascontiguousarray(feature2, dtype=np.float64).reshape(-1, 2)
    total = max(int(po[-1]), 0)
    if f1.shape[0] != total or f2.shape[0] != total:
        raise ValueError(f"feature1 and feature2 must have pair_offset[-1] = {total} rows")
    th = None if pair_error_threshold is None else np.ascontiguousarray(pair_error_threshold, dtype=np.float64)
    if th is not None and th.shape != (npair,):
        raise ValueError(f"pair_error_threshold must have num_pairs = {npair} entries")
    pm = None if pair_mask is None else np.ascontiguousarray(pair_mask, dtype=np.uint8)
    if pm is not None and pm.shape != (npair,):
        raise ValueError(f"pair_mask must have num_pairs = {npair} entries")
    ps = None if pair_stream is None else np.ascontiguousarray(pair_stream, dtype=np.uint32)
    if ps is not None and ps.shape != (npair,):
        raise ValueError(f"pair_stream must have num_pairs = {npair} entries")
    k = max(int(o.max_iterations), 0)
    sm = None
    if samples is not None:
        sm = np.ascontiguousarray(samples, dtype=np.int32)
        if sm.shape != (npair, k, 8):
            raise ValueError(f"samples must have shape (num_pairs, max_iterations, 8) = ({npair}, {k}, 8)")
    nsel = npair if pm is None else int(np.count_nonzero(pm))
    status = np.full(npair, -1, dtype=np.int8)
    i32 = [np.zeros(npair, dtype=np.int32) for _ in range(4)]
    conf = np.zeros(npair)
    fm = np.zeros((npair, 9))
    fl1 = np.zeros(npair)
    fl2 = np.zeros(npair)
    rot = np.zeros((npair, 3))
    pos = np.zeros((npair, 3))
    inl = np.zeros(total, dtype=np.uint8)
    hyp = np.full((nsel, min(k, 1 << 20)), -1, dtype=np.int32) if want_hypothesis_cost else None
    rs = abi.CTwoViewRansacSummary()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    st = L.tmi_ba_estimate_uncalibrated_relative_poses(
        C.byref(o), npair, po.ctypes.data, f1.ctypes.data, f2.ctypes.data, ptr(th), ptr(pm), ptr(ps), ptr(sm),
        0 if sm is None else 1, status.ctypes.data, *[a.ctypes.data for a in i32], conf.ctypes.data, fm.ctypes.data,
        fl1.ctypes.data, fl2.ctypes.data, rot.ctypes.data, pos.ctypes.data, inl.ctypes.data, ptr(hyp), C.byref(rs))
    if st != 0:
        raise EngineError(st, "tmi_ba_estimate_uncalibrated_relative_poses")
    return dict(status=status, num_correspondences=i32[0], num_inliers=i32[1], num_iterations=i32[2],
                best_iteration=i32[3], confidence=conf, fundamental_matrix=fm, focal_length1=fl1, focal_length2=fl2,
                rotation=rot, position=pos, corr_inlier=inl, hypothesis_cost=hyp, summary=rs)


def estimate_calibrated_relative_poses(pair_offset, feature1, feature2, pair_error_threshold, options=None,
                                       pair_mask=None, pair_stream=None, samples=None,
                                       want_hypothesis_cost: bool = False):
    """Batched EstimateRelativePose (the calibrated branch of EstimateTwoViewInfo: five-point RANSAC, the pose from E)
    over the pairs pair_mask selects (None = all).  pair_offset [P + 1] int64; feature1 / feature2 [N, 2] NORMALISED
    coordinates (principal point removed, divided by the focal length); pair_error_threshold [P] the squared threshold in
    those units.  pair_stream: optional [P] uint32 sample-stream ids (None: the pair index).  samples: optional
    [P, max_iterations, 5] int32 sample table (otherwise drawn from options.seed).
    Returns a dict: status [P] int8, num_correspondences, num_inliers, num_iterations, best_iteration, best_solution [P]
    int32, confidence [P], essential_matrix [P, 9] (column-major, unit norm), rotation / position [P, 3], corr_inlier [N]
    uint8, hypothesis_cost [num_selected, max_iterations, 10] int32 or None, summary (CTwoViewRansacSummary).  Raises
    EngineError on any failure."""
    L = load()
    o = options if options is not None else abi.two_view_ransac_options()
    po = np.ascontiguousarray(pair_offset, dtype=np.int64)
    if po.ndim != 1 or po.shape[0] < 1:
        raise ValueError("pair_offset must have num_pairs + 1 entries")
    npair = po.shape[0] - 1
    f1 = np.ascontiguousarray(feature1, dtype=np.float64).reshape(-1, 2)
    f2 = np.ascontiguousarray(feature2, dtype=np.float64).reshape(-1, 2)
    total = max(int(po[-1]), 0)
    if f1.shape[0] != total or f2.shape[0] != total:
        raise ValueError(f"feature1 and feature2 must have pair_offset[-1] = {total} rows")
    th = None if pair_error_threshold is None else np.ascontiguousarray(pair_error_threshold, dtype=np.float64)
    if th is not None and th.shape != (npair,):
        raise ValueError(f"pair_error_threshold must have num_pairs = {npair} entries")
    pm = None if pair_mask is None else np.ascontiguousarray(pair_mask, dtype=np.uint8)
    if pm is not None and pm.shape != (npair,):
        raise ValueError(f"pair_mask must have num_pairs = {npair} entries")
    ps = None if pair_stream is None else np.ascontiguousarray(pair_stream, dtype=np.uint32)
    if ps is not None and ps.shape != (npair,):
        raise ValueError(f"pair_stream must have num_pairs = {npair} entries")
    k = max(int(o.max_iterations), 0)
    sm = None
    if samples is not None:
        sm = np.ascontiguousarray(samples, dtype=np.int32)
        if sm.shape != (npair, k, 5):
            raise ValueError(f"samples must have shape (num_pairs, max_iterations, 5) = ({npair}, {k}, 5)")
    nsel = npair if pm is None else int(np.count_nonzero(pm))
    status = np.full(npair, -1, dtype=np.int8)
    i32 = [np.zeros(npair, dtype=np.int32) for _ in range(5)]
    conf = np.zeros(npair)
    em = np.zeros((npair, 9))
    rot = np.zeros((npair, 3))
    pos = np.zeros((npair, 3))
    inl = np.zeros(total, dtype=np.uint8)
    hyp = np.full((nsel, min(k, 1 << 20), abi.CALIBRATED_SLOTS), -1, dtype=np.int32) if want_hypothesis_cost else None
    rs = abi.CTwoViewRansacSummary()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    st = L.tmi_ba_estimate_calibrated_relative_poses(
        C.byref(o), npair, po.ctypes.data, f1.ctypes.data, f2.ctypes.data, ptr(th), ptr(pm), ptr(ps), ptr(sm),
        0 if sm is None else 1, status.ctypes.data, *[a.ctypes.data for a in i32], conf.ctypes.data, em.ctypes.data,
        rot.ctypes.data, pos.ctypes.data, inl.ctypes.data, ptr(hyp), C.byref(rs))
    if st != 0:
        raise EngineError(st, "tmi_ba_estimate_calibrated_relative_poses")
    return dict(status=status, num_correspondences=i32[0], num_inliers=i32[1], num_iterations=i32[2],
                best_iteration=i32[3], best_solution=i32[4], confidence=conf, essential_matrix=em, rotation=rot,
                position=pos, corr_inlier=inl, hypothesis_cost=hyp, summary=rs)


class Solver:
    """Resident form: the problem stays in HBM across solve() calls."""

    def __init__(self, problem: abi.Problem, options: abi.COptions, rank: int = 0, world: int = 1):
        self._L = load()
        self.problem = problem
        self._cp = problem.as_c()
        self._h = C.c_void_p()
        self._cb = None
        st = self._L.tmi_ba_solver_create(C.byref(self._cp), C.byref(options), rank, world,
                                          C.byref(self._h))
        if st != 0:
            self._h = C.c_void_p()
            raise EngineError(st, "tmi_ba_solver_create")

    def set_allreduce(self, fn):
        """fn(device_ptr:int, count:int, hip_stream:int) -> 0 on success."""
        def tramp(buf, count, stream, user):
            try:
                return int(fn(buf, count, stream))
            except Exception as exc:  # never let an exception cross the C boundary
                print(f"[theiasfm_amd] all-reduce hook raised: {exc!r}", flush=True)
                return 1
        self._cb = ALLREDUCE_FN(tramp)
        st = self._L.tmi_ba_solver_set_allreduce(self._h, self._cb, None)
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_set_allreduce")

    def init_rccl(self, unique_id: bytes):
        """Native RCCL transport: every rank passes the 128-byte id rank 0 obtained from
        rccl_unique_id() (ship it with torch.distributed / MPI / a file)."""
        if unique_id is None:  # drop the communicator: the all-reduce hook applies again
            st = self._L.tmi_ba_solver_init_rccl(self._h, None)
            if st != 0:
                raise EngineError(st, "tmi_ba_solver_init_rccl")
            return
        if len(unique_id) != 128:
            raise ValueError("ncclUniqueId is 128 bytes")
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        st = self._L.tmi_ba_solver_init_rccl(self._h, buf)
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_init_rccl")

    def debug_allreduce(self, value: float) -> float:
        out = C.c_double(0.0)
        st = self._L.tmi_ba_solver_debug_allreduce(self._h, value, C.byref(out))
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_debug_allreduce")
        return out.value

    def solve(self, options: abi.COptions):
        s = abi.CSummary()
        st = self._L.tmi_ba_solver_solve(self._h, C.byref(options), C.byref(s))
        return st, s

    def reset(self):
        st = self._L.tmi_ba_solver_reset(self._h)
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_reset")

    def set_parameters(self, prob: abi.Problem):
        """new extrinsics / intrinsics / points for the resident structure (what reset() restores from then on)"""
        self._keep = prob  # the C view points into its arrays
        cp = prob.as_c()
        st = self._L.tmi_ba_solver_set_parameters(self._h, C.byref(cp))
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_set_parameters")

    def download(self):
        st = self._L.tmi_ba_solver_download(self._h, C.byref(self._cp))
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_download")
        return self.problem

    def filter_outlier_tracks(self, max_inlier_reprojection_error: float,
                              min_triangulation_angle_degrees: float):
        """SetOutlierTracksToUnestimated on the resident parameters (this rank's tracks)."""
        n = self.problem.num_points
        flag = np.full(n, 255, dtype=np.uint8)
        mean = np.full(n, np.nan)
        fs = abi.CFilterSummary()
        st = self._L.tmi_ba_solver_filter_outlier_tracks(
            self._h, float(max_inlier_reprojection_error), float(min_triangulation_angle_degrees),
            flag.ctypes.data, mean.ctypes.data, C.byref(fs))
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_filter_outlier_tracks")
        return flag, mean, fs

    def select_good_tracks(self, long_track_length_threshold: int, image_grid_cell_size_pixels: int,
                           min_num_optimized_tracks_per_view: int, view_mask=None):
        """SelectGoodTracksForBundleAdjustment on the resident parameters (unsharded handle)."""
        n = self.problem.num_points
        sel = np.zeros(n, dtype=np.uint8)
        ln = np.zeros(n, dtype=np.int32)
        err = np.zeros(n)
        ss = abi.CSelectSummary()
        vm = None if view_mask is None else np.ascontiguousarray(view_mask, dtype=np.uint8)
        st = self._L.tmi_ba_solver_select_good_tracks(
            self._h, long_track_length_threshold, image_grid_cell_size_pixels,
            min_num_optimized_tracks_per_view, None if vm is None else vm.ctypes.data, sel.ctypes.data, ln.ctypes.data, err.ctypes.data,
            C.byref(ss))
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_select_good_tracks")
        return sel, ln, err, ss

    def adjust_tracks(self, options: abi.COptions):
        """Batched BundleAdjustTrack on the resident parameters (this rank's tracks)."""
        n = self.problem.num_points
        term = np.full(n, -1, dtype=np.int8)
        iters = np.zeros(n, dtype=np.int32)
        c0 = np.zeros(n)
        c1 = np.zeros(n)
        ts = abi.CTrackBatchSummary()
        st = self._L.tmi_ba_solver_adjust_tracks(self._h, C.byref(options), term.ctypes.data,
                                                 iters.ctypes.data, c0.ctypes.data, c1.ctypes.data,
                                                 C.byref(ts))
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_adjust_tracks")
        return term, iters, c0, c1, ts

    def adjust_views(self, options: abi.COptions, view_mask=None):
        """Batched BundleAdjustView on the resident parameters (unsharded handle); a later solve() / download()
        sees the new cameras."""
        vm, term, iters, c0, c1, vs = _view_outputs(self.problem.num_cameras, view_mask)
        st = self._L.tmi_ba_solver_adjust_views(self._h, C.byref(options), None if vm is None else vm.ctypes.data,
                                                term.ctypes.data, iters.ctypes.data, c0.ctypes.data, c1.ctypes.data,
                                                C.byref(vs))
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_adjust_views")
        return term, iters, c0, c1, vs

    def estimate_tracks(self, estimator_options: abi.CTrackEstimatorOptions, ba_options: abi.COptions,
                        track_mask=None):
        """Batched TrackEstimator on the resident cameras (unsharded handle); a later solve() / download() sees the
        new points.  Returns (status [Np] int8, CTrackEstimateSummary)."""
        tm, status, es = _track_mask(self.problem.num_points, track_mask)
        st = self._L.tmi_ba_solver_estimate_tracks(self._h, C.byref(estimator_options), C.byref(ba_options),
                                                   None if tm is None else tm.ctypes.data, status.ctypes.data,
                                                   C.byref(es))
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_estimate_tracks")
        return status, es

    def structure_checksums(self):
        """Test hook: [24] uint64 checksums of the static structure arrays in HBM ([0] = built on the device)."""
        out = (C.c_uint64 * 24)()
        st = self._L.tmi_ba_solver_structure_checksums(self._h, out)
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_structure_checksums")
        return list(out)

    def operator_info(self) -> dict:
        """Which kernels this handle runs (tmi_ba_solver_operator_info)."""
        out = (C.c_int32 * 8)()
        st = self._L.tmi_ba_solver_operator_info(self._h, out)
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_operator_info")
        return dict(one_sweep_product=bool(out[0]), position_columns_formed=bool(out[1]), direct_camera_side=bool(out[2]),
                    adaptive=bool(out[3]), implicit=bool(out[4]), break_even=int(out[5]), cluster_handle=bool(out[6]),
                    compact_planes=bool(out[7] & 1), speculative_linearize=bool(out[7] & 2),
                    # back-substitution from the products' per-track sums (TMI_BA_BACKSUB_FROM_PRODUCTS): available to
                    # this handle / LM iterations of the last solve() that took it instead of the observation sweep
                    back_substitute_from_products=bool(out[7] & 4),
                    back_substitute_from_products_iterations=int(out[7]) >> 8)

    @property
    def stream(self) -> int:
        return int(self._L.tmi_ba_solver_stream(self._h) or 0)

    def evaluate(self, point_dof: int):
        """Device residuals [N,2], reduced camera Jacobians [N,2,D], shared-intrinsics
        Jacobians [N,2,D], point Jacobians [N,2,point_dof], valid [N] in the caller's
        observation order, and D."""
        n = self.problem.num_observations
        bd = C.c_int32(0)
        # D is not known before the call: allocate for the largest block (16)
        r = np.zeros((n, 2))
        A = np.zeros(n * 2 * 16)
        A1 = np.zeros(n * 2 * 16)
        Jp = np.zeros((n, 2, point_dof))
        valid = np.zeros(n, dtype=np.uint8)
        st = self._L.tmi_ba_solver_evaluate(self._h, r.ctypes.data, A.ctypes.data, A1.ctypes.data,
                                            Jp.ctypes.data, valid.ctypes.data, C.byref(bd))
        if st != 0:
            raise EngineError(st, "tmi_ba_solver_evaluate")
        D = bd.value
        return r, A[: n * 2 * D].reshape(n, 2, D), A1[: n * 2 * D].reshape(n, 2, D), Jp, valid, D

    def close(self):
        if self._h:
            self._L.tmi_ba_solver_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def estimate_homographies(pair_offset, feature1, feature2, pair_error_threshold, options=None, pair_mask=None,
                          pair_stream=None, samples=None, want_hypothesis_cost: bool = False,
                          want_hypothesis_cost_real: bool = False):
    """Batched EstimateHomography (the homography inlier count of the two-view geometric verification: four-point
    RANSAC with inlier-count or, options.use_mle, MLESAC scoring) over the pairs pair_mask selects (None = all).
    pair_offset [P + 1] int64; feature1 / feature2 [N, 2] in the caller's units; pair_error_threshold [P] the squared
    threshold in those units.  pair_stream: optional [P] uint32 sample-stream ids (None: the pair index).  samples:
    optional [P, max_iterations, 4] int32 sample table (otherwise drawn from options.seed).
    Returns a dict: status [P] int8, num_correspondences, num_inliers, num_iterations, best_iteration [P] int32,
    confidence [P], homography [P, 9] (column-major, no scale imposed), corr_inlier [N] uint8, hypothesis_cost
    [num_selected, max_iterations] int32 or None, hypothesis_cost_real [num_selected, max_iterations] float64 or None
    (an argument error without options.use_mle), summary (CTwoViewRansacSummary).  Raises EngineError on any failure."""
    L = load()
    o = options if options is not None else abi.homography_ransac_options()
    po = np.ascontiguousarray(pair_offset, dtype=np.int64)
    if po.ndim != 1 or po.shape[0] < 1:
        raise ValueError("pair_offset must have num_pairs + 1 entries")
    npair = po.shape[0] - 1
    f1 = np.ascontiguousarray(feature1, dtype=np.float64).reshape(-1, 2)
    f2 = np.ascontiguousarray(feature2, dtype=np.float64).reshape(-1, 2)
    total = max(int(po[-1]), 0)
    if f1.shape[0] != total or f2.shape[0] != total:
        raise ValueError(f"feature1 and feature2 must have pair_offset[-1] = {total} rows")
    th = None if pair_error_threshold is None else np.ascontiguousarray(pair_error_threshold, dtype=np.float64)
    if th is not None and th.shape != (npair,):
        raise ValueError(f"pair_error_threshold must have num_pairs = {npair} entries")
    pm = None if pair_mask is None else np.ascontiguousarray(pair_mask, dtype=np.uint8)
    if pm is not None and pm.shape != (npair,):
        raise ValueError(f"pair_mask must have num_pairs = {npair} entries")
    ps = None if pair_stream is None else np.ascontiguousarray(pair_stream, dtype=np.uint32)
    if ps is not None and ps.shape != (npair,):
        raise ValueError(f"pair_stream must have num_pairs = {npair} entries")
    k = max(int(o.max_iterations), 0)
    sm = None
    if samples is not None:
        sm = np.ascontiguousarray(samples, dtype=np.int32)
        if sm.shape != (npair, k, 4):
            raise ValueError(f"samples must have shape (num_pairs, max_iterations, 4) = ({npair}, {k}, 4)")
    nsel = npair if pm is None else int(np.count_nonzero(pm))
    status = np.full(npair, -1, dtype=np.int8)
    i32 = [np.zeros(npair, dtype=np.int32) for _ in range(4)]
    conf = np.zeros(npair)
    hm = np.zeros((npair, 9))
    inl = np.zeros(total, dtype=np.uint8)
    hyp = np.full((nsel, min(k, 1 << 20)), -1, dtype=np.int32) if want_hypothesis_cost else None
    hyr = np.full((nsel, min(k, 1 << 20)), np.nan) if want_hypothesis_cost_real else None
    rs = abi.CTwoViewRansacSummary()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    st = L.tmi_ba_estimate_homographies(
        C.byref(o), npair, po.ctypes.data, f1.ctypes.data, f2.ctypes.data, ptr(th), ptr(pm), ptr(ps), ptr(sm),
        0 if sm is None else 1, status.ctypes.data, *[a.ctypes.data for a in i32], conf.ctypes.data, hm.ctypes.data,
        inl.ctypes.data, ptr(hyp), ptr(hyr), C.byref(rs))
    if st != 0:
        raise EngineError(st, "tmi_ba_estimate_homographies")
    return dict(status=status, num_correspondences=i32[0], num_inliers=i32[1], num_iterations=i32[2],
                best_iteration=i32[3], confidence=conf, homography=hm, corr_inlier=inl, hypothesis_cost=hyp,
                hypothesis_cost_real=hyr, summary=rs)


def _known_orientation(symbol, item_offset, features, extra, orientations, item_error_threshold, options, item_mask,
                       item_stream, samples, want_hypothesis_cost, want_hypothesis_cost_real):
    """The shared body of the two known-orientation calls: `features` the one or two [N, 2] arrays, `extra` the
    [N, 3] world points or None, `orientations` one [P, 3] array per feature array."""
    L = load()
    o = options if options is not None else abi.homography_ransac_options()
    po = np.ascontiguousarray(item_offset, dtype=np.int64)
    if po.ndim != 1 or po.shape[0] < 1:
        raise ValueError("item_offset must have num_items + 1 entries")
    nitem = po.shape[0] - 1
    total = max(int(po[-1]), 0)
    fs = [np.ascontiguousarray(f, dtype=np.float64).reshape(-1, 2) for f in features]
    if any(f.shape[0] != total for f in fs):
        raise ValueError(f"every feature array must have item_offset[-1] = {total} rows")
    xs = []
    if extra is not None:
        xs = [np.ascontiguousarray(extra, dtype=np.float64).reshape(-1, 3)]
        if xs[0].shape[0] != total:
            raise ValueError(f"world_point must have item_offset[-1] = {total} rows")
    os_ = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3) for a in orientations]
    if any(a.shape[0] != nitem for a in os_):
        raise ValueError(f"every orientation array must have num_items = {nitem} rows")
    th = None if item_error_threshold is None else np.ascontiguousarray(item_error_threshold, dtype=np.float64)
    if th is not None and th.shape != (nitem,):
        raise ValueError(f"the error thresholds must have num_items = {nitem} entries")
    pm = None if item_mask is None else np.ascontiguousarray(item_mask, dtype=np.uint8)
    if pm is not None and pm.shape != (nitem,):
        raise ValueError(f"the mask must have num_items = {nitem} entries")
    ps = None if item_stream is None else np.ascontiguousarray(item_stream, dtype=np.uint32)
    if ps is not None and ps.shape != (nitem,):
        raise ValueError(f"the streams must have num_items = {nitem} entries")
    k = max(int(o.max_iterations), 0)
    sm = None
    if samples is not None:
        sm = np.ascontiguousarray(samples, dtype=np.int32)
        if sm.shape != (nitem, k, 2):
            raise ValueError(f"samples must have shape (num_items, max_iterations, 2) = ({nitem}, {k}, 2)")
    nsel = nitem if pm is None else int(np.count_nonzero(pm))
    status = np.full(nitem, -1, dtype=np.int8)
    i32 = [np.zeros(nitem, dtype=np.int32) for _ in range(4)]
    conf = np.zeros(nitem)
    pos = np.zeros((nitem, 3))
    inl = np.zeros(total, dtype=np.uint8)
    hyp = np.full((nsel, min(k, 1 << 20)), -1, dtype=np.int32) if want_hypothesis_cost else None
    hyr = np.full((nsel, min(k, 1 << 20)), np.nan) if want_hypothesis_cost_real else None
    rot = [np.zeros((total, 2)) for _ in fs]
    rs = abi.CTwoViewRansacSummary()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    st = getattr(L, symbol)(
        C.byref(o), nitem, po.ctypes.data, *[a.ctypes.data for a in fs + xs + os_], ptr(th), ptr(pm), ptr(ps), ptr(sm),
        0 if sm is None else 1, status.ctypes.data, *[a.ctypes.data for a in i32], conf.ctypes.data, pos.ctypes.data,
        inl.ctypes.data, ptr(hyp), ptr(hyr), *[a.ctypes.data for a in rot], C.byref(rs))
    if st != 0:
        raise EngineError(st, symbol)
    return dict(status=status, num_correspondences=i32[0], num_inliers=i32[1], num_iterations=i32[2],
                best_iteration=i32[3], confidence=conf, position=pos, corr_inlier=inl, hypothesis_cost=hyp,
                hypothesis_cost_real=hyr, rotated=rot, summary=rs)


def estimate_positions_known_orientation(item_offset, feature, world_point, item_orientation, item_error_threshold,
                                         options=None, item_mask=None, item_stream=None, samples=None,
                                         want_hypothesis_cost: bool = False, want_hypothesis_cost_real: bool = False):
    """Batched EstimateAbsolutePoseWithKnownOrientation (two-point position RANSAC with inlier-count or,
    options.use_mle, MLESAC scoring) over the views item_mask selects (None = all).  item_offset [P + 1] int64; feature
    [N, 2] normalised and NOT rotated; world_point [N, 3]; item_orientation [P, 3] angle-axis; item_error_threshold [P]
    squared, normalised units.  item_stream, samples ([P, max_iterations, 2]) as in estimate_homographies.
    Returns a dict: status [P] int8, num_correspondences, num_inliers, num_iterations, best_iteration [P] int32,
    confidence [P], position [P, 3], corr_inlier [N] uint8, hypothesis_cost / hypothesis_cost_real
    [num_selected, max_iterations] or None, rotated_feature [N, 2] (what the RANSAC saw; 0 for views not attempted),
    summary (CTwoViewRansacSummary).  Raises EngineError on any failure."""
    out = _known_orientation("tmi_ba_estimate_positions_known_orientation", item_offset, [feature], world_point,
                             [item_orientation], item_error_threshold, options, item_mask, item_stream, samples,
                             want_hypothesis_cost, want_hypothesis_cost_real)
    out["rotated_feature"] = out.pop("rotated")[0]
    return out


def estimate_relative_positions_known_orientation(pair_offset, feature1, feature2, pair_orientation1,
                                                  pair_orientation2, pair_error_threshold, options=None,
                                                  pair_mask=None, pair_stream=None, samples=None,
                                                  want_hypothesis_cost: bool = False,
                                                  want_hypothesis_cost_real: bool = False):
    """Batched EstimateRelativePoseWithKnownOrientation (two-point baseline-direction RANSAC, either scoring) over the
    pairs pair_mask selects.  feature1 / feature2 [N, 2] normalised and NOT rotated; pair_orientation1 /
    pair_orientation2 [P, 3] the two views' angle-axes (zeros: the features are taken as already rotated).  The other
    arguments and the returned dict are those of estimate_positions_known_orientation, with position [P, 3] the unit
    direction (its sign is not part of the estimate) and rotated_feature1 / rotated_feature2 [N, 2]."""
    out = _known_orientation("tmi_ba_estimate_relative_positions_known_orientation", pair_offset,
                             [feature1, feature2], None, [pair_orientation1, pair_orientation2], pair_error_threshold,
                             options, pair_mask, pair_stream, samples, want_hypothesis_cost, want_hypothesis_cost_real)
    out["rotated_feature1"], out["rotated_feature2"] = out.pop("rotated")
    return out
