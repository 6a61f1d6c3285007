"""ctypes binding of liboa_icp.so (include/oa_icp.h) -- the only way Python reaches the HIP kernels.

There is no fallback: if the shared library is missing or no GPU is usable the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liboa_icp.so")
LIB_EXP_PATH = os.path.join(_HERE, "liboa_icp_exp.so")      # the same library + the experiments (csrc/oa_families.hpp: OA_EXPERIMENTS)

OA_OK = 0
OA_E_BAD_ARG = -1
OA_E_HIP = -2
OA_E_TOO_FEW_PAIRS = -3
OA_E_SINGULAR = -4
OA_E_NO_DEVICE = -5
OA_E_STATE = -6
OA_E_BAD_THRESH = -7
OA_E_CAPACITY = -8
OA_E_RCCL = -9
OA_EXCHANGE_AUTO = -1
OA_EXCHANGE_MAILBOX = 0
OA_EXCHANGE_RCCL = 1
OA_NSUMS = 24
OA_METRIC_POINT = 0
OA_METRIC_PLANE = 1
OA_METRIC_GICP = 2
OA_METRIC_SYMMETRIC = 3
OA_LOSS_NONE = 0
OA_LOSS_HUBER = 1
OA_LOSS_TUKEY = 2
OA_LOSS_CAUCHY = 3
OA_POSE_NSCORE = 4
OA_ORIENT_NONE = 0
OA_ORIENT_TOWARD = 1
OA_ORIENT_AWAY = 2
OA_SEED_KEEP = 0
OA_SEED_TOWARD = 1
OA_SEED_AWAY = 2
OA_FPFH_DIM = 33
OA_FEAT_TOO_FEW_PAIRS = 1
OA_FEAT_NO_POSE = 2
OA_STAT_MESH_PSEUDONORMALS = 36
OA_STAT_RECIPROCAL = 37
OA_STAT_RECIPROCAL_RATIO = 38
OA_STAT_RECIP_REJECTED = 39
OA_STAT_TRIM = 40
OA_STAT_TRIM_CANDIDATES = 41
OA_STAT_TRIM_KEPT = 42
OA_STAT_TRIM_CUT = 43
OA_TRIM_AUTO = -1.0
OA_STAT_REJECT_BOUNDARY = 44
OA_STAT_BOUNDARY_REJECTED = 45
OA_STAT_TARGET_BOUNDARY = 46
OA_STAT_BOUNDARY_VERTICES = 47
OA_STAT_BOUNDARY_EDGES = 48
OA_STAT_ACC_PATH = 49
OA_STAT_ACC_ROWS = 50
OA_STAT_TARGET_CLEANED = 51
OA_OUTLIER_STATISTICAL = 0
OA_OUTLIER_RADIUS = 1
OA_CLUSTER_KEEP_CLUSTERED = 0
OA_CLUSTER_KEEP_LARGEST = 1
OA_CLUSTER_KEEP_MIN_SIZE = 2
(OA_ACC_CANON, OA_ACC_STRIDE, OA_ACC_WEIGHTED, OA_ACC_PLANE, OA_ACC_GICP, OA_ACC_FUSED_GRID, OA_ACC_FUSED_TRI_GRID, OA_ACC_FUSED_TREE,
 OA_ACC_FUSED_TRI_TREE, OA_ACC_DUAL) = range(1, 11)

# every symbol include/oa_icp.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "oa_device_count", "oa_create", "oa_create_multi", "oa_num_devices", "oa_set_exchange", "oa_release_cached_memory",
    "oa_destroy", "oa_last_error", "oa_version", "oa_set_stream",
    "oa_set_search_mode",
    "oa_set_target", "oa_set_target_mesh", "oa_set_source", "oa_set_normals", "oa_set_matrices", "oa_get_matrix_world", "oa_num_selected",
    "oa_reset_seeds", "oa_get_stat",
    "oa_make_pairs", "oa_nn_search", "oa_kabsch", "oa_affine_from_points", "oa_kabsch_from_sums", "oa_get_pivot",
    "oa_iterate", "oa_run", "oa_get_history", "oa_run_begin", "oa_iter_partial", "oa_iter_finish", "oa_run_end",
    "oa_get_search_ms", "oa_measure_valu_ceiling", "oa_exchange_note",
    "oa_set_metric", "oa_set_target_normals", "oa_point_to_plane",
    "oa_set_robust", "oa_set_source_weights", "oa_set_robust_auto",
    "oa_score_poses", "oa_coarse_candidates", "oa_coarse_align",
    "oa_target_knn", "oa_estimate_target_normals",
    "oa_set_gicp", "oa_set_source_normals",
    "oa_symmetric_step",
    "oa_coarse_align_poses", "oa_target_fpfh", "oa_match_features", "oa_feature_candidates",
    "oa_voxel_downsample",
    "oa_deviation", "oa_get_mesh_pseudonormals",
    "oa_set_reciprocal", "oa_set_trim",
    "oa_target_boundary", "oa_set_reject_boundary",
    "oa_normal_space_sample", "oa_stability",
    "oa_orient_target_normals",
    "oa_target_outliers", "oa_target_radius_count",
    "oa_target_clusters",
    "oa_set_neighbor_radius", "oa_get_neighbor_radius", "oa_target_spacing",
]


class Settings(C.Structure):
    _fields_ = [("iters", C.c_int32), ("use_target", C.c_int32), ("with_scale", C.c_int32),
                ("early_exit", C.c_int32), ("thresh", C.c_double), ("target_d", C.c_double)]


class Report(C.Structure):
    _fields_ = [("iters_done", C.c_int32), ("converged", C.c_int32), ("status", C.c_int32),
                ("reserved", C.c_int32), ("last_K", C.c_int64), ("last_translation", C.c_double),
                ("mean_dist", C.c_double), ("std_dist", C.c_double), ("mean_rot_angle", C.c_double),
                ("nn_ms_total", C.c_double), ("loop_ms", C.c_double)]


class CoarseSettings(C.Structure):
    _fields_ = [("n_rot", C.c_int32), ("n_refine", C.c_int32), ("refine_iters", C.c_int32), ("stride", C.c_int32),
                ("thresh", C.c_double)]


class CoarseReport(C.Structure):
    _fields_ = [("n_candidates", C.c_int32), ("best_candidate", C.c_int32), ("best_rank", C.c_int32), ("status", C.c_int32),
                ("cost_start", C.c_double), ("cost_best_candidate", C.c_double), ("cost_refined", C.c_double),
                ("K_refined", C.c_int64), ("score_ms", C.c_double), ("total_ms", C.c_double)]


class FeatureSettings(C.Structure):
    _fields_ = [("dim", C.c_int32), ("n_hyp", C.c_int32), ("mutual", C.c_int32), ("seed", C.c_uint32),
                ("ratio", C.c_double), ("edge_tol", C.c_double), ("min_edge", C.c_double)]


class FeatureReport(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("n_accepted", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32),
                ("match_ms", C.c_double), ("total_ms", C.c_double)]


class VoxelReport(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_finite", C.c_int64), ("n_voxels", C.c_int64), ("max_members", C.c_int64),
                ("dims", C.c_int32 * 3), ("reserved", C.c_int32), ("origin", C.c_double * 3), ("total_ms", C.c_double)]


class DeviationSettings(C.Structure):
    _fields_ = [("thresh", C.c_double), ("signed_mode", C.c_int32), ("n_quantiles", C.c_int32), ("quantiles", C.c_double * 8),
                ("n_bins", C.c_int32), ("reserved", C.c_int32), ("hist_lo", C.c_double), ("hist_hi", C.c_double)]


class DeviationReport(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_valid", C.c_int64), ("n_inlier", C.c_int64), ("n_inside", C.c_int64), ("n_unsigned", C.c_int64),
                ("max_index", C.c_int64), ("fitness", C.c_double), ("mean", C.c_double), ("rms", C.c_double), ("std", C.c_double),
                ("mean_signed", C.c_double), ("max_dist", C.c_double), ("quantile_values", C.c_double * 8), ("n_quantiles", C.c_int32),
                ("signed_used", C.c_int32), ("surface", C.c_int32), ("reserved", C.c_int32), ("search_ms", C.c_double),
                ("total_ms", C.c_double), ("pseudonormal_ms", C.c_double)]


class SampleReport(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_eligible", C.c_int64), ("bins_occupied", C.c_int64), ("level", C.c_int64),
                ("max_bin_count", C.c_int64), ("total_ms", C.c_double)]


class StabilityReport(C.Structure):
    _fields_ = [("n_used", C.c_int64), ("centroid", C.c_double * 3), ("scale", C.c_double), ("C", C.c_double * 36),
                ("eigenvalues", C.c_double * 6), ("eigenvectors", C.c_double * 36), ("rank", C.c_int32), ("reserved", C.c_int32),
                ("cond", C.c_double), ("total_ms", C.c_double)]


class OrientReport(C.Structure):
    _fields_ = [("n_components", C.c_int64), ("n_left_out", C.c_int64), ("n_flipped", C.c_int64), ("rounds", C.c_int32),
                ("reserved", C.c_int32)]


class OutlierSettings(C.Structure):
    _fields_ = [("method", C.c_int32), ("k", C.c_int32), ("std_ratio", C.c_double), ("radius", C.c_double),
                ("min_neighbors", C.c_int32), ("count_cap", C.c_int32)]


class OutlierReport(C.Structure):
    _fields_ = [("n_kept", C.c_int64), ("n_removed", C.c_int64), ("n_nonfinite", C.c_int64), ("mean", C.c_double),
                ("std", C.c_double), ("threshold", C.c_double)]


class ClusterSettings(C.Structure):
    _fields_ = [("eps", C.c_double), ("min_points", C.c_int32), ("keep", C.c_int32), ("min_size", C.c_int64)]


class ClusterReport(C.Structure):
    _fields_ = [("n_clusters", C.c_int64), ("n_core", C.c_int64), ("n_border", C.c_int64), ("n_noise", C.c_int64),
                ("n_nonfinite", C.c_int64), ("largest_label", C.c_int64), ("largest_size", C.c_int64), ("n_kept", C.c_int64),
                ("n_removed", C.c_int64)]


class SpacingReport(C.Structure):
    _fields_ = [("mean", C.c_double), ("std", C.c_double), ("n_finite", C.c_int64), ("n_nonfinite", C.c_int64)]


class OaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("oa_icp error %d: %s" % (code, msg))
        self.code = code
        self.msg = msg


_libs = {}


def load(experiments: bool = False):
    """Load liboa_icp.so (experiments=True: liboa_icp_exp.so, the flavour the A/B tests use).  Raises (loudly) when the HIP
    extension has not been built."""
    if experiments in _libs:
        return _libs[experiments]
    # One HIP runtime per process: PyTorch bundles its own libamdhip64.so.7.  If liboa_icp.so pulled in the
    # system copy first, torch would later fail with "No HIP GPUs are available"; importing torch first makes both
    # bind to the same runtime.  Without torch installed the system runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    # Another BUILD of the same library (the sanitizer pass, A/B experiments) -- only when OA_ICP_LIB_DEBUG=1 says that the
    # override is meant, and never silently: an environment variable alone does not redirect what a production import loads.
    path = LIB_EXP_PATH if experiments else LIB_PATH
    override = os.environ.get("OA_ICP_LIB")
    if override:
        if os.environ.get("OA_ICP_LIB_DEBUG") == "1":
            import sys
            print("object_alignment_amd: loading %s instead of %s (OA_ICP_LIB, OA_ICP_LIB_DEBUG=1)" % (override, LIB_PATH), file=sys.stderr)
            path = override
        else:
            import warnings
            warnings.warn("OA_ICP_LIB is set but ignored: set OA_ICP_LIB_DEBUG=1 as well to load another build of liboa_icp.so")
    if not os.path.exists(path):
        raise RuntimeError(
            "object_alignment_amd: %s is missing -- build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback" % path)
    L = C.CDLL(path)
    vp, fp, dp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    L.oa_device_count.restype = C.c_int
    L.oa_create.argtypes = [C.POINTER(vp), C.c_int]
    L.oa_create_multi.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]
    L.oa_num_devices.argtypes = [vp]
    L.oa_set_exchange.argtypes = [vp, C.c_int]
    L.oa_release_cached_memory.restype = None
    L.oa_destroy.argtypes = [vp]
    L.oa_destroy.restype = None
    L.oa_last_error.restype = C.c_char_p
    L.oa_version.restype = C.c_char_p
    L.oa_set_stream.argtypes = [vp, vp]
    L.oa_set_search_mode.argtypes = [vp, C.c_int]
    L.oa_set_target.argtypes = [vp, vp, C.c_int64, C.c_int]
    L.oa_set_target_mesh.argtypes = [vp, vp, C.c_int64, C.c_int, C.POINTER(C.c_int32), C.c_int64]
    L.oa_set_source.argtypes = [vp, vp, C.c_int64, C.c_int, ip, C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    L.oa_set_normals.argtypes = [vp, fp, C.c_int64, fp, C.c_int64, C.c_double]
    L.oa_set_matrices.argtypes = [vp, fp, fp]
    L.oa_get_matrix_world.argtypes = [vp, fp]
    L.oa_num_selected.argtypes = [vp]
    L.oa_reset_seeds.argtypes = [vp]
    L.oa_get_stat.argtypes = [vp, C.c_int, dp]
    L.oa_num_selected.restype = C.c_int64
    L.oa_make_pairs.argtypes = [vp, C.c_double, C.c_int, dp, dp, C.c_int64, ip, dp]
    L.oa_nn_search.argtypes = [vp, ip, fp, dp]
    L.oa_kabsch.argtypes = [vp, dp, dp, C.c_int64, C.c_int64, C.c_int, dp]
    L.oa_affine_from_points.argtypes = [vp, dp, dp, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, dp]
    L.oa_kabsch_from_sums.argtypes = [vp, dp, dp, C.c_int, dp]
    L.oa_get_pivot.argtypes = [vp, dp]
    L.oa_iterate.argtypes = [vp, C.POINTER(Settings), dp, dp]
    L.oa_run.argtypes = [vp, C.POINTER(Settings), C.POINTER(Report)]
    L.oa_get_history.argtypes = [vp, C.c_int32, dp, fp, ip, dp, dp]
    L.oa_exchange_note.argtypes = [vp]
    L.oa_exchange_note.restype = C.c_char_p
    L.oa_get_search_ms.argtypes = [vp, C.c_int32, dp]
    L.oa_measure_valu_ceiling.argtypes = [vp, C.c_double, dp]
    L.oa_run_begin.argtypes = [vp, C.POINTER(Settings)]
    L.oa_iter_partial.argtypes = [vp, vp]
    L.oa_iter_finish.argtypes = [vp, vp]
    L.oa_run_end.argtypes = [vp, C.POINTER(Report)]
    L.oa_set_metric.argtypes = [vp, C.c_int]
    L.oa_set_target_normals.argtypes = [vp, fp, C.c_int64]
    L.oa_set_gicp.argtypes = [vp, C.c_double]
    L.oa_set_source_normals.argtypes = [vp, fp, C.c_int64]
    L.oa_point_to_plane.argtypes = [vp, dp, dp, dp, C.c_int64, C.c_int64, dp]
    L.oa_symmetric_step.argtypes = [vp, dp, dp, dp, dp, C.c_int64, C.c_int64, dp]
    L.oa_set_robust.argtypes = [vp, C.c_int, C.c_double]
    L.oa_set_source_weights.argtypes = [vp, fp, C.c_int64]
    L.oa_set_robust_auto.argtypes = [vp, C.c_double, C.c_double]
    L.oa_score_poses.argtypes = [vp, fp, C.c_int32, C.c_double, C.c_int32, dp]
    L.oa_coarse_candidates.argtypes = [vp, C.c_int32, fp]
    L.oa_coarse_align.argtypes = [vp, C.POINTER(CoarseSettings), C.POINTER(CoarseReport)]
    L.oa_target_knn.argtypes = [vp, C.c_int, C.POINTER(C.c_int32), fp]
    L.oa_estimate_target_normals.argtypes = [vp, C.c_int, C.c_int, fp, C.c_int, fp, fp]
    i32p = C.POINTER(C.c_int32)
    L.oa_coarse_align_poses.argtypes = [vp, fp, C.c_int32, C.POINTER(CoarseSettings), C.POINTER(CoarseReport)]
    L.oa_target_fpfh.argtypes = [vp, C.c_int, fp, C.c_int]
    L.oa_match_features.argtypes = [vp, fp, C.c_int64, fp, C.c_int64, C.c_int32, i32p, fp, fp]
    L.oa_feature_candidates.argtypes = [vp, fp, C.c_int64, fp, C.POINTER(FeatureSettings), i32p, fp, i32p, C.POINTER(FeatureReport)]
    L.oa_voxel_downsample.argtypes = [vp, vp, C.c_int64, C.c_int, vp, C.c_double, dp, C.c_int64, fp, fp, i32p, ip, ip,
                                      C.POINTER(VoxelReport)]
    L.oa_deviation.argtypes = [vp, C.POINTER(DeviationSettings), dp, dp, fp, ip, C.POINTER(C.c_int8), ip, C.POINTER(DeviationReport)]
    L.oa_get_mesh_pseudonormals.argtypes = [vp, fp, fp]
    L.oa_set_reciprocal.argtypes = [vp, C.c_int, C.c_double]
    L.oa_target_boundary.argtypes = [vp, C.c_int, C.c_double, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]
    L.oa_set_reject_boundary.argtypes = [vp, C.c_int, C.c_int, C.c_double]
    L.oa_set_trim.argtypes = [vp, C.c_double, C.c_double, C.c_double]
    L.oa_normal_space_sample.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_uint32, C.c_int64, ip, i32p, ip,
                                         C.POINTER(SampleReport)]
    L.oa_stability.argtypes = [vp, vp, vp, C.c_int64, C.c_int, ip, C.c_int64, C.POINTER(StabilityReport)]
    L.oa_orient_target_normals.argtypes = [vp, C.c_int, C.c_double, C.c_int, fp, fp, C.c_int, fp, C.POINTER(C.c_uint8), i32p,
                                           C.POINTER(OrientReport)]
    L.oa_target_outliers.argtypes = [vp, C.POINTER(OutlierSettings), C.c_int, C.POINTER(C.c_uint8), dp, i32p, i32p,
                                     C.POINTER(OutlierReport)]
    L.oa_target_radius_count.argtypes = [vp, C.c_double, C.c_int32, i32p]
    L.oa_target_clusters.argtypes = [vp, C.POINTER(ClusterSettings), C.c_int, i32p, i32p, C.POINTER(C.c_uint8), i32p,
                                     C.POINTER(ClusterReport)]
    L.oa_set_neighbor_radius.argtypes = [vp, C.c_float]
    L.oa_get_neighbor_radius.argtypes = [vp, fp]
    L.oa_target_spacing.argtypes = [vp, C.POINTER(SpacingReport)]
    _libs[experiments] = L
    return L


def check(rc, lib=None):
    if rc != OA_OK:
        raise OaError(rc, (lib if lib is not None else load()).oa_last_error().decode("utf-8", "replace"))
    return rc


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def as_f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(shape) if shape is not None else a
