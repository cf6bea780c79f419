"""uvo -- MI355X-native ORB feature front-end (extract + match), Python plumbing over the C ABI.

The product is `libuvo.so` (hand-written HIP for gfx950 behind include/uvo/uvo.h).  This module only loads it with
ctypes and mirrors the reference's two entry classes (USLAM::ORBextractor, include/ORBextractor.h:47-95;
USLAM::ORBmatcher, include/ORBmatcher.h:41-88) so the parity tests and bench.py read like calls into the
reference.  There is no CPU fallback: importing fails loudly when the library is missing, and creating an
extractor / matcher fails when no HIP device is usable.

The package directory is not a valid Python identifier; import it with
    importlib.import_module("u-vip-slam_amd")
"""
import collections
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libuvo.so")

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                           ("class_id", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28

UVO_OK, UVO_E_BADARG, UVO_E_NODEVICE, UVO_E_HIP, UVO_E_CAPACITY, UVO_E_UNSUPPORTED, UVO_E_NOMEM = 0, -1, -2, -3, -4, -5, -6
UVO_TUNE_OCT_WIDE_MAX = 1
UVO_TUNE_FAST_MODE = 2
UVO_FAST_MODE_ADAPTIVE, UVO_FAST_MODE_TWO_PASS, UVO_FAST_MODE_SINGLE_PASS = 0, 1, 2
UVO_TUNE_BLUR_ROUNDING, UVO_BLUR_ROUNDING_SCALAR, UVO_BLUR_ROUNDING_SSE2 = 9, 0, 1
UVO_TUNE_LEVEL0_INPLACE = 11
# launch-shape knobs outside the public header (csrc/tune_internal.h): the parity tests force each shape through them
UVO_TUNE_FUSE_BLUR_TREE = 10
UVO_TUNE_PYR_RING = 12
UVO_TUNE_PYR_FORM, UVO_PYR_FORM_AUTO, UVO_PYR_FORM_LEVELS, UVO_PYR_FORM_TILES, UVO_PYR_FORM_ROWS = 13, 0, 1, 2, 3
UVO_TUNE_PYR_TILE_GROUP = 14
UVO_TUNE_FEW_FRAMES = 16
UVO_TUNE_ZERO_COPY_OUT, UVO_TUNE_SPIN_WAIT = 17, 18

# every symbol include/uvo/uvo.h declares
ABI_SYMBOLS = [
    "uvo_extractor_create", "uvo_extractor_destroy", "uvo_extractor_levels", "uvo_extractor_max_keypoints", "uvo_extractor_scale_factor", "uvo_extractor_tables",
    "uvo_extract", "uvo_extract_tracked", "uvo_extract_batch", "uvo_extract_batch_device", "uvo_host_alloc", "uvo_host_free", "uvo_host_register", "uvo_host_unregister", "uvo_host_bind_near_device", "uvo_host_bind_to_cpulist_file", "uvo_shard_plan_make", "uvo_sharder_create", "uvo_sharder_destroy", "uvo_sharder_max_keypoints", "uvo_sharder_run", "uvo_sharder_submit", "uvo_sharder_wait", "uvo_extract_batch_submit", "uvo_extract_batch_wait", "uvo_extractor_synchronize", "uvo_extractor_set_pipeline", "uvo_extractor_tune", "uvo_extractor_fast_state", "uvo_extractor_level_dims",
    "uvo_grider_fast", "uvo_clahe", "uvo_clahe_batch_device", "uvo_extractor_read_plane", "uvo_extractor_read_candidates", "uvo_extractor_octree_tap", "uvo_extractor_profile", "uvo_extractor_profile_only", "uvo_extractor_kernel_times",
    "uvo_matcher_create", "uvo_matcher_destroy", "uvo_matcher_synchronize", "uvo_hamming_knn2", "uvo_hamming_knn2_batch_device",
    "uvo_hamming_matrix", "uvo_distinctive_descriptors", "uvo_search_by_projection", "uvo_match_windows", "uvo_match_groups",
    "uvo_search_by_projection_kf", "uvo_search_by_bow", "uvo_search_for_triangulation", "uvo_search_for_triangulation_batch", "uvo_search_for_triangulation_next", "uvo_triangulate_matches", "uvo_create_new_map_points", "uvo_fuse", "uvo_fuse_batch", "uvo_project_points", "uvo_search_points_in_frustum", "uvo_sim3_decompose", "uvo_sim3_relative", "uvo_project_sim3", "uvo_search_by_projection_sim3", "uvo_search_by_sim3", "uvo_haloc_hash", "uvo_klt_create", "uvo_klt_destroy", "uvo_klt_build_pyramid", "uvo_klt_build_pyramid_from_extractor", "uvo_klt_read_level", "uvo_klt_track", "uvo_undistort_points", "uvo_klt_track_undistorted", "uvo_klt_find_fundamental", "uvo_klt_track_filtered", "uvo_klt_fm_hypotheses", "uvo_klt_solve_pnp_ransac", "uvo_klt_pnp_hypotheses", "uvo_vocabulary_create", "uvo_vocabulary_destroy", "uvo_bow_transform", "uvo_matcher_wait_extractor", "uvo_extractor_wait_matcher", "uvo_matcher_attach_extractor", "uvo_matcher_profile",
    "uvo_glibc_srand", "uvo_glibc_rand_next", "uvo_pnpsolver_set_create", "uvo_pnpsolver_set_destroy", "uvo_pnpsolver_set_clear", "uvo_pnpsolver_add",
    "uvo_pnpsolver_query", "uvo_pnpsolver_iterate", "uvo_pnpsolver_hypotheses",
    "uvo_pose_optimizer_create", "uvo_pose_optimizer_destroy", "uvo_pose_optimize", "uvo_pose_optimizer_trace",
    "uvo_nav_optimizer_create", "uvo_nav_optimizer_destroy", "uvo_nav_optimize", "uvo_nav_optimizer_trace",
    "uvo_sim3solver_set_create", "uvo_sim3solver_set_destroy", "uvo_sim3solver_set_clear", "uvo_sim3solver_add", "uvo_sim3solver_set_ransac_parameters",
    "uvo_sim3solver_query", "uvo_sim3solver_iterate", "uvo_sim3solver_find", "uvo_sim3solver_hypotheses",
    "uvo_sim3_optimizer_create", "uvo_sim3_optimizer_destroy", "uvo_sim3_optimize", "uvo_sim3_optimizer_trace",
    "uvo_bundle_adjuster_create", "uvo_bundle_adjuster_destroy", "uvo_bundle_adjust", "uvo_bundle_adjuster_trace",
    "uvo_nav_bundle_adjuster_create", "uvo_nav_bundle_adjuster_destroy", "uvo_nav_bundle_adjust", "uvo_nav_bundle_adjuster_trace",
    "uvo_essential_graph_create", "uvo_essential_graph_destroy", "uvo_essential_graph_optimize", "uvo_essential_graph_trace",
    "uvo_initializer_create", "uvo_initializer_destroy", "uvo_initializer_set_reference", "uvo_initializer_initialize", "uvo_initializer_hypotheses",
    "uvo_kfdb_create", "uvo_kfdb_destroy", "uvo_kfdb_add", "uvo_kfdb_erase", "uvo_kfdb_clear", "uvo_kfdb_set_covisibles", "uvo_kfdb_detect_reloc",
    "uvo_kfdb_detect_loop", "uvo_kfdb_detect_loop_haloc", "uvo_kfdb_last_query", "uvo_kfdb_last_haloc", "uvo_kfdb_state", "uvo_kfdb_size",
    "uvo_matcher_kernel_times", "uvo_last_error", "uvo_device_info",
]


class MatchRule(ctypes.Structure):
    """uvo_match_rule (include/uvo/uvo.h)."""
    _fields_ = [("rule", ctypes.c_int32), ("max_dist", ctypes.c_int32), ("nn_ratio", ctypes.c_float), ("exclusive", ctypes.c_int32),
                ("check_orientation", ctypes.c_int32)]


class FeatureVectorC(ctypes.Structure):
    """uvo_feature_vector: a DBoW2::FeatureVector in flat form."""
    _fields_ = [("node", ctypes.c_void_p), ("start", ctypes.c_void_p), ("feat", ctypes.c_void_p), ("n_nodes", ctypes.c_int32)]


class Epipolar(ctypes.Structure):
    """uvo_epipolar."""
    _fields_ = [("f12", ctypes.c_float * 9), ("q_x", ctypes.c_void_p), ("q_y", ctypes.c_void_p), ("t_x", ctypes.c_void_p), ("t_y", ctypes.c_void_p),
                ("sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int32)]


class CameraPose(ctypes.Structure):
    """uvo_camera_pose."""
    _fields_ = [("rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("ow", ctypes.c_float * 3), ("fx", ctypes.c_float), ("fy", ctypes.c_float),
                ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("min_x", ctypes.c_float), ("max_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("max_y", ctypes.c_float)]

    @classmethod
    def make(cls, Rcw, tcw, Ow, fx, fy, cx, cy, bounds):
        """bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY)"""
        c = cls()
        c.rcw[:] = [float(x) for x in np.asarray(Rcw, np.float32).reshape(9)]
        c.tcw[:] = [float(x) for x in np.asarray(tcw, np.float32).reshape(3)]
        c.ow[:] = [float(x) for x in np.asarray(Ow, np.float32).reshape(3)]
        c.fx, c.fy, c.cx, c.cy = float(fx), float(fy), float(cx), float(cy)
        c.min_x, c.min_y, c.max_x, c.max_y = [float(b) for b in bounds]
        return c

    def as_array(self):
        return np.frombuffer(bytes(self), np.float32).copy()


class TriangulationPairC(ctypes.Structure):
    """uvo_triangulation_pair."""
    _fields_ = [("fv2", ctypes.c_void_p), ("kp2", ctypes.c_void_p), ("n2", ctypes.c_int32), ("desc2", ctypes.c_void_p), ("has_mp2", ctypes.c_void_p),
                ("f12", ctypes.c_float * 9), ("sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int32)]


class TriangulationCameraC(ctypes.Structure):
    """uvo_triangulation_camera."""
    _fields_ = [("rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("ow", ctypes.c_float * 3), ("fx", ctypes.c_float), ("fy", ctypes.c_float),
                ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("scale_factors", ctypes.c_void_p), ("sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int32)]


class NewMapPointsC(ctypes.Structure):
    """uvo_new_map_points."""
    _fields_ = [("n_matches", ctypes.c_void_p), ("n_accepted", ctypes.c_void_p), ("idx1", ctypes.c_void_p), ("idx2", ctypes.c_void_p),
                ("verdict", ctypes.c_void_p), ("x3d", ctypes.c_void_p), ("has_mp1_out", ctypes.c_void_p)]


TRI_ACCEPTED, TRI_PARALLAX, TRI_W_ZERO, TRI_BEHIND_1, TRI_BEHIND_2, TRI_REPROJ_1, TRI_REPROJ_2, TRI_ZERO_DIST, TRI_SCALE = range(9)


class TriangulationCamera:
    """A key frame as the triangulation reads it (uvo_triangulation_camera): Rcw, tcw, Ow = GetCameraCenter(), intrinsics and the level
    tables GetScaleFactor(level) / GetSigma2(level).  Keeps the tables alive for the C struct."""

    def __init__(self, rcw, tcw, ow, fx, fy, cx, cy, scale_factors, sigma2):
        self.sf = np.ascontiguousarray(scale_factors, np.float32)
        self.sigma2 = np.ascontiguousarray(sigma2, np.float32)
        assert len(self.sf) == len(self.sigma2)
        c = self.c = TriangulationCameraC()
        c.rcw[:] = [float(x) for x in np.asarray(rcw, np.float32).reshape(9)]
        c.tcw[:] = [float(x) for x in np.asarray(tcw, np.float32).reshape(3)]
        c.ow[:] = [float(x) for x in np.asarray(ow, np.float32).reshape(3)]
        c.fx, c.fy, c.cx, c.cy = float(fx), float(fy), float(cx), float(cy)
        c.scale_factors, c.sigma2, c.nlevels = self.sf.ctypes.data, self.sigma2.ctypes.data, len(self.sf)


class FuseTargetC(ctypes.Structure):
    """uvo_fuse_target."""
    _fields_ = [("kp", ctypes.c_void_p), ("n", ctypes.c_int32), ("desc", ctypes.c_void_p), ("min_x", ctypes.c_int32), ("min_y", ctypes.c_int32),
                ("max_x", ctypes.c_int32), ("max_y", ctypes.c_int32), ("cam", CameraPose), ("scale_factors", ctypes.c_void_p), ("nlevels", ctypes.c_int32)]


PROJECT_FRUSTUM, PROJECT_KF_RELOC, PROJECT_FUSE, PROJECT_PIXEL_BOUNDED, PROJECT_PIXEL = range(5)
RULE_BEST_RATIO_SAME_LEVEL, RULE_BEST_ONLY, RULE_BEST_RATIO_LE, RULE_BEST_RATIO_LT, RULE_TRIANGULATION, RULE_BEST_RATIO_LEQ, RULE_INIT_STEAL = range(7)


class FeatureVector:
    """DBoW2::FeatureVector stand-in: {node id: [feature indices]} kept as the flat arrays the C ABI takes."""

    def __init__(self, groups):
        nodes = sorted(groups)
        self.node = np.asarray(nodes, np.uint32)
        self.start = np.zeros(len(nodes) + 1, np.int32)
        feats = []
        for j, k in enumerate(nodes):
            feats.extend(int(v) for v in groups[k])
            self.start[j + 1] = len(feats)
        self.feat = np.asarray(feats, np.int32)
        self.c = FeatureVectorC(_ptr(self.node), _ptr(self.start), _ptr(self.feat) if len(feats) else None, len(nodes))


class UvoError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        super().__init__("%s failed with code %d: %s" % (where, code, last_error()))


class ExtractorCfg(ctypes.Structure):
    _fields_ = [("nfeatures", ctypes.c_int32), ("scale_factor", ctypes.c_float), ("nlevels", ctypes.c_int32), ("score_type", ctypes.c_int32),
                ("fast_th", ctypes.c_int32), ("max_width", ctypes.c_int32), ("max_height", ctypes.c_int32), ("max_batch", ctypes.c_int32),
                ("max_input_keypoints", ctypes.c_int32), ("device", ctypes.c_int32)]


UVO_SHARD_MAX, UVO_SHARD_REMOTE = 64, -1


class SharderCfg(ctypes.Structure):
    _fields_ = [("extractor", ExtractorCfg), ("n_shards", ctypes.c_int32), ("devices", ctypes.c_int32 * UVO_SHARD_MAX), ("chunk_frames", ctypes.c_int32),
                ("match", ctypes.c_int32)]


class ShardPlan(ctypes.Structure):
    _fields_ = [("first_frame", ctypes.c_int32), ("n_frames", ctypes.c_int32), ("first_pair", ctypes.c_int32), ("n_pairs", ctypes.c_int32),
                ("halo_frame", ctypes.c_int32), ("n_chunks", ctypes.c_int32)]


class MatcherCfg(ctypes.Structure):
    _fields_ = [("max_query", ctypes.c_int32), ("max_train", ctypes.c_int32), ("max_batch", ctypes.c_int32), ("max_map_points", ctypes.c_int32),
                ("device", ctypes.c_int32)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("libuvo.so not built (%s); run `python u-vip-slam_amd/build.py` -- there is no CPU fallback" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    vp, ci, cf, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_ssize_t
    lib.uvo_last_error.restype = ctypes.c_char_p
    lib.uvo_device_info.argtypes = [ci, ctypes.c_char_p, ci]
    lib.uvo_extractor_create.argtypes = [ctypes.POINTER(ExtractorCfg), ctypes.POINTER(vp)]
    lib.uvo_extractor_destroy.argtypes = [vp]
    lib.uvo_extractor_destroy.restype = None
    lib.uvo_extractor_levels.argtypes = [vp]
    lib.uvo_extractor_max_keypoints.argtypes = [vp]
    lib.uvo_extractor_scale_factor.argtypes = [vp]
    lib.uvo_extractor_scale_factor.restype = cf
    lib.uvo_extractor_tables.argtypes = [vp, vp, vp, vp, vp]
    lib.uvo_extract.argtypes = [vp, vp, ci, ci, cl, vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, ci, vp]
    lib.uvo_extract_tracked.argtypes = [vp, vp, ci, ci, cl, vp, ci, ci, ci, vp, vp, ci, vp, vp]
    lib.uvo_extract_batch.argtypes = [vp, ci, vp, ci, ci, cl, cl, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, ci, vp]
    lib.uvo_extract_batch_device.argtypes = [vp, ci, vp, ci, ci, cl, cl, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, ci, vp]
    lib.uvo_host_alloc.argtypes = [vp, ctypes.c_size_t]
    lib.uvo_host_free.argtypes = [vp]
    lib.uvo_host_register.argtypes = [vp, ctypes.c_size_t]
    lib.uvo_host_unregister.argtypes = [vp]
    lib.uvo_host_bind_near_device.argtypes = [ci, vp]
    lib.uvo_host_bind_to_cpulist_file.argtypes = [ctypes.c_char_p]
    lib.uvo_shard_plan_make.argtypes = [ci, ci, ci, ci, ctypes.POINTER(ShardPlan)]
    lib.uvo_sharder_create.argtypes = [ctypes.POINTER(SharderCfg), ctypes.POINTER(vp)]
    lib.uvo_sharder_destroy.argtypes = [vp]
    lib.uvo_sharder_destroy.restype = None
    lib.uvo_sharder_max_keypoints.argtypes = [vp]
    lib.uvo_sharder_run.argtypes = [vp, vp, ci, ci, ci, ci, ci, cl, cl, vp, vp, ci, vp, vp, vp, vp, vp]
    lib.uvo_sharder_submit.argtypes = [vp, vp, ci, ci, ci, ci, ci, cl, cl, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    lib.uvo_sharder_wait.argtypes = [vp, ci]
    lib.uvo_extract_batch_submit.argtypes = [vp, ci, vp, ci, ci, cl, cl, vp, vp, ci, vp, vp]
    lib.uvo_extract_batch_wait.argtypes = [vp, ci]
    lib.uvo_extractor_synchronize.argtypes = [vp]
    lib.uvo_extractor_set_pipeline.argtypes = [vp, ci]
    lib.uvo_extractor_tune.argtypes = [vp, ci, ci]
    lib.uvo_extractor_level_dims.argtypes = [vp, ci, vp, vp]
    lib.uvo_extractor_fast_state.argtypes = [vp, vp, vp, vp]
    lib.uvo_clahe.argtypes = [vp, vp, ci, ci, cl, ctypes.c_double, ci, ci, vp, cl]
    lib.uvo_clahe_batch_device.argtypes = [vp, ci, vp, ci, ci, cl, cl, ctypes.c_double, ci, ci, vp, cl, cl]
    lib.uvo_grider_fast.argtypes = [vp, vp, ci, ci, cl, ci, ci, ci, ci, ci, vp, ci, vp]
    lib.uvo_extractor_read_plane.argtypes = [vp, ci, ci, ci, vp]
    lib.uvo_extractor_read_candidates.argtypes = [vp, ci, ci, vp, ci, vp]
    lib.uvo_extractor_octree_tap.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, vp, vp]
    lib.uvo_extractor_profile.argtypes = [vp, ci]
    lib.uvo_extractor_profile_only.argtypes = [vp, ctypes.c_char_p]
    lib.uvo_extractor_kernel_times.argtypes = [vp, ctypes.c_char_p, ci, vp, vp, ci, vp]
    lib.uvo_matcher_create.argtypes = [ctypes.POINTER(MatcherCfg), ctypes.POINTER(vp)]
    lib.uvo_matcher_destroy.argtypes = [vp]
    lib.uvo_matcher_destroy.restype = None
    lib.uvo_matcher_synchronize.argtypes = [vp]
    lib.uvo_hamming_knn2.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp, vp]
    lib.uvo_hamming_knn2_batch_device.argtypes = [vp, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp]
    lib.uvo_hamming_matrix.argtypes = [vp, vp, ci, vp, ci, vp]
    lib.uvo_distinctive_descriptors.argtypes = [vp, vp, vp, ci, vp, vp]
    lib.uvo_search_by_projection.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, cf, cf, vp]
    lib.uvo_match_windows.argtypes = [vp, vp, ci, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uvo_match_groups.argtypes = [vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uvo_search_by_projection_kf.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, cf, ci, ci, vp]
    lib.uvo_search_by_bow.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, cf, ci, vp, vp]
    lib.uvo_search_for_triangulation.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, vp, vp]
    lib.uvo_project_points.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, cf, cf, vp, vp, vp, vp, vp]
    lib.uvo_vocabulary_create.argtypes = [vp, ctypes.POINTER(vp)]
    lib.uvo_vocabulary_destroy.argtypes = [vp]
    lib.uvo_vocabulary_destroy.restype = None
    lib.uvo_bow_transform.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, vp]
    lib.uvo_haloc_hash.argtypes = [vp, vp, ci, ci, vp, ci, vp]
    lib.uvo_klt_create.argtypes = [vp, ctypes.POINTER(vp)]
    lib.uvo_klt_destroy.argtypes = [vp]
    lib.uvo_klt_destroy.restype = None
    lib.uvo_klt_build_pyramid.argtypes = [vp, ci, vp, ci, ci, cl, vp]
    lib.uvo_klt_build_pyramid_from_extractor.argtypes = [vp, ci, vp, vp]
    lib.uvo_klt_read_level.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    lib.uvo_klt_track.argtypes = [vp, ci, ci, vp, vp, ci, ci, ci, ctypes.c_double, ctypes.c_double, vp, vp]
    lib.uvo_undistort_points.argtypes = [vp, vp, vp, ci, vp]
    lib.uvo_klt_track_undistorted.argtypes = [vp, ci, ci, vp, vp, ci, ci, ci, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp, vp]
    lib.uvo_klt_find_fundamental.argtypes = [vp, vp, vp, ci, ctypes.c_double, ctypes.c_double, vp, vp, vp]
    lib.uvo_klt_track_filtered.argtypes = [vp, ci, ci, vp, vp, ci, ci, ci, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp, vp, ctypes.c_double,
                                           ctypes.c_double, vp, vp]
    lib.uvo_klt_fm_hypotheses.argtypes = [vp, vp, vp, vp, ci, vp]
    lib.uvo_klt_solve_pnp_ransac.argtypes = [vp, vp, vp, ci, vp, ci, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp, vp]
    lib.uvo_klt_pnp_hypotheses.argtypes = [vp, vp, vp, vp, ci, vp]
    lib.uvo_glibc_srand.argtypes = [vp, ctypes.c_uint32]
    lib.uvo_glibc_srand.restype = None
    lib.uvo_glibc_rand_next.argtypes = [vp]
    lib.uvo_glibc_rand_next.restype = ctypes.c_int32
    lib.uvo_pnpsolver_set_create.argtypes = [vp, ci, ci, vp]
    lib.uvo_pnpsolver_set_destroy.argtypes = [vp]
    lib.uvo_pnpsolver_set_destroy.restype = None
    lib.uvo_pnpsolver_set_clear.argtypes = [vp]
    lib.uvo_pnpsolver_add.argtypes = [vp, vp, vp, vp, vp, ci, ci, cf, cf, cf, cf, vp, vp]
    lib.uvo_pnpsolver_query.argtypes = [vp, ci, vp]
    lib.uvo_pnpsolver_iterate.argtypes = [vp, vp, ci, ci, vp, vp]
    lib.uvo_pnpsolver_hypotheses.argtypes = [vp, ci, vp, vp, vp, ci, vp]
    lib.uvo_pose_optimizer_create.argtypes = [vp, ci, ci, vp]
    lib.uvo_pose_optimizer_destroy.argtypes = [vp]
    lib.uvo_pose_optimizer_destroy.restype = None
    lib.uvo_pose_optimize.argtypes = [vp, vp, ci, vp]
    lib.uvo_pose_optimizer_trace.argtypes = [vp, ci, vp]
    lib.uvo_nav_optimizer_create.argtypes = [vp, ci, ci, vp]
    lib.uvo_nav_optimizer_destroy.argtypes = [vp]
    lib.uvo_nav_optimizer_destroy.restype = None
    lib.uvo_nav_optimize.argtypes = [vp, vp, ci, vp]
    lib.uvo_nav_optimizer_trace.argtypes = [vp, ci, vp]
    lib.uvo_sim3_optimizer_create.argtypes = [vp, ci, ci, vp]
    lib.uvo_sim3_optimizer_destroy.argtypes = [vp]
    lib.uvo_sim3_optimizer_destroy.restype = None
    lib.uvo_sim3_optimize.argtypes = [vp, vp, ci, vp]
    lib.uvo_sim3_optimizer_trace.argtypes = [vp, ci, vp]
    lib.uvo_bundle_adjuster_create.argtypes = [vp, ci, ci, ci, ci, vp]
    lib.uvo_bundle_adjuster_destroy.argtypes = [vp]
    lib.uvo_bundle_adjuster_destroy.restype = None
    lib.uvo_bundle_adjust.argtypes = [vp, vp, vp]
    lib.uvo_bundle_adjuster_trace.argtypes = [vp, vp]
    lib.uvo_nav_bundle_adjuster_create.argtypes = [vp, ci, ci, ci, ci, ci, vp]
    lib.uvo_nav_bundle_adjuster_destroy.argtypes = [vp]
    lib.uvo_nav_bundle_adjuster_destroy.restype = None
    lib.uvo_nav_bundle_adjust.argtypes = [vp, vp, vp]
    lib.uvo_nav_bundle_adjuster_trace.argtypes = [vp, vp]
    lib.uvo_essential_graph_create.argtypes = [vp, ci, ci, ci, ci, vp]
    lib.uvo_essential_graph_destroy.argtypes = [vp]
    lib.uvo_essential_graph_destroy.restype = None
    lib.uvo_essential_graph_optimize.argtypes = [vp, vp, vp]
    lib.uvo_essential_graph_trace.argtypes = [vp, vp]
    lib.uvo_sim3solver_set_create.argtypes = [vp, ci, ci, vp]
    lib.uvo_sim3solver_set_destroy.argtypes = [vp]
    lib.uvo_sim3solver_set_destroy.restype = None
    lib.uvo_sim3solver_set_clear.argtypes = [vp]
    lib.uvo_sim3solver_add.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp]
    lib.uvo_sim3solver_set_ransac_parameters.argtypes = [vp, ci, vp]
    lib.uvo_sim3solver_query.argtypes = [vp, ci, vp]
    lib.uvo_sim3solver_iterate.argtypes = [vp, vp, ci, ci, vp, vp]
    lib.uvo_sim3solver_find.argtypes = [vp, ci, vp, vp]
    lib.uvo_sim3solver_hypotheses.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp]
    lib.uvo_initializer_create.argtypes = [vp, ci, vp]
    lib.uvo_initializer_destroy.argtypes = [vp]
    lib.uvo_initializer_destroy.restype = None
    lib.uvo_initializer_set_reference.argtypes = [vp, vp, ci, vp, cf, ci]
    lib.uvo_initializer_initialize.argtypes = [vp, vp, ci, vp, vp, vp]
    lib.uvo_initializer_hypotheses.argtypes = [vp, vp, vp, vp, ci, vp]
    i64 = ctypes.c_int64
    lib.uvo_kfdb_create.argtypes = [ci, ci, ci, ci, vp]
    lib.uvo_kfdb_destroy.argtypes = [vp]
    lib.uvo_kfdb_destroy.restype = None
    lib.uvo_kfdb_add.argtypes = [vp, i64, vp, vp, ci, vp, vp]
    lib.uvo_kfdb_erase.argtypes = [vp, ci]
    lib.uvo_kfdb_clear.argtypes = [vp]
    lib.uvo_kfdb_set_covisibles.argtypes = [vp, ci, vp, ci]
    lib.uvo_kfdb_detect_reloc.argtypes = [vp, i64, vp, vp, ci, vp, ci, vp]
    lib.uvo_kfdb_detect_loop.argtypes = [vp, i64, vp, vp, ci, vp, ci, cf, vp, ci, vp]
    lib.uvo_kfdb_detect_loop_haloc.argtypes = [vp, i64, vp, vp, ci, cf, vp, vp]
    lib.uvo_kfdb_last_query.argtypes = [vp, vp, ci, vp, vp, vp]
    lib.uvo_kfdb_last_haloc.argtypes = [vp, vp, vp, ci, vp]
    lib.uvo_kfdb_state.argtypes = [vp, ci, ci, vp]
    lib.uvo_kfdb_size.argtypes = [vp]
    lib.uvo_fuse.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, cf, vp, vp]
    lib.uvo_search_for_triangulation_batch.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp]
    lib.uvo_search_for_triangulation_next.argtypes = [vp, ci, vp, ci, vp, vp]
    lib.uvo_triangulate_matches.argtypes = [vp, vp, vp, cf, vp, vp, ci, vp, vp]
    lib.uvo_create_new_map_points.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, cf, ci, vp]
    lib.uvo_fuse_batch.argtypes = [vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, cf, vp, vp]
    lib.uvo_search_points_in_frustum.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, cf, cf, cf, cf, vp, vp, vp, vp, vp, vp, vp]
    lib.uvo_sim3_decompose.argtypes = [vp, ci, vp]
    lib.uvo_sim3_relative.argtypes = [cf, vp, vp, vp, vp, vp]
    lib.uvo_project_sim3.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp]
    lib.uvo_search_by_projection_sim3.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, ci, ci, vp]
    lib.uvo_search_by_sim3.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, cf, vp, vp]
    lib.uvo_matcher_wait_extractor.argtypes = [vp, vp]
    lib.uvo_extractor_wait_matcher.argtypes = [vp, vp]
    lib.uvo_matcher_attach_extractor.argtypes = [vp, vp]
    lib.uvo_matcher_profile.argtypes = [vp, ci]
    lib.uvo_matcher_kernel_times.argtypes = [vp, ctypes.c_char_p, ci, vp, vp, ci, vp]
    return lib


lib = _load()


def last_error():
    return lib.uvo_last_error().decode("utf-8", "replace")


def device_info(device=0):
    buf = ctypes.create_string_buffer(256)
    rc = lib.uvo_device_info(device, buf, 256)
    if rc:
        raise UvoError(rc, "uvo_device_info")
    return buf.value.decode()


def _ptr(a):
    return None if a is None else a.ctypes.data


def pinned_empty(shape, dtype):
    """numpy array in page-locked host memory (uvo_host_alloc), for the asynchronous host-buffer form; freed with the array."""
    import weakref
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    p = ctypes.c_void_p()
    rc = lib.uvo_host_alloc(ctypes.byref(p), max(n, 1))
    if rc:
        raise UvoError(rc, "uvo_host_alloc")
    buf = (ctypes.c_uint8 * max(n, 1)).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
    weakref.finalize(buf, lib.uvo_host_free, p.value)
    return arr


def shard_plan(total_frames, n_shards, shard, chunk_frames):
    """uvo_shard_plan_make: the block of one shard (pure arithmetic, works without a GPU)."""
    p = ShardPlan()
    rc = lib.uvo_shard_plan_make(total_frames, n_shards, shard, chunk_frames, ctypes.byref(p))
    if rc:
        raise UvoError(rc, "uvo_shard_plan_make")
    return p


class Sharder:
    """uvo_sharder: one job of `total` frames over the GPUs of one node, results gathered by the device-to-host copies themselves
    (include/uvo/uvo.h "Sharder").  devices[i] = HIP ordinal of shard i, or UVO_SHARD_REMOTE for shards another process runs."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, fastTh=20, *, max_width=640, max_height=512, devices=(0,), chunk_frames=128,
                 match=True):
        self.cfg = SharderCfg()
        self.cfg.extractor = ExtractorCfg(nfeatures, scaleFactor, nlevels, 0, fastTh, max_width, max_height, 1, 0, 0)
        self.cfg.n_shards = len(devices)
        for i, d in enumerate(devices):
            self.cfg.devices[i] = d
        self.cfg.chunk_frames = chunk_frames
        self.cfg.match = 1 if match else 0
        self._h = ctypes.c_void_p()
        rc = lib.uvo_sharder_create(ctypes.byref(self.cfg), ctypes.byref(self._h))
        if rc:
            self._h = None
            raise UvoError(rc, "uvo_sharder_create")
        self.cap = lib.uvo_sharder_max_keypoints(self._h)
        self.n_shards, self.chunk_frames = len(devices), chunk_frames

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.uvo_sharder_destroy(self._h)
            self._h = None

    __del__ = close

    def plan(self, total_frames, shard):
        return shard_plan(total_frames, self.n_shards, shard, self.chunk_frames)

    def _check(self, imgs, total_frames, out_kp, out_desc, n_out, idx0, d0, idx1, d1):
        assert imgs.dtype == np.uint8 and imgs.ndim == 3 and imgs.flags.c_contiguous
        cap = out_kp.shape[1]
        assert out_kp.dtype == KEYPOINT_DTYPE and out_kp.shape[0] >= total_frames and out_kp.flags.c_contiguous
        assert out_desc.dtype == np.uint8 and out_desc.shape[1:] == (cap, 32) and out_desc.flags.c_contiguous
        assert n_out.dtype == np.int32 and len(n_out) >= total_frames
        if idx0 is not None:
            for a, dt in ((idx0, np.int32), (idx1, np.int32), (d0, np.uint16), (d1, np.uint16)):
                assert a.dtype == dt and a.shape[1] == cap and a.shape[0] >= total_frames - 1 and a.flags.c_contiguous
        return cap

    def submit(self, imgs, imgs_first_frame, total_frames, out_kp, out_desc, n_out, idx0=None, d0=None, idx1=None, d1=None):
        """uvo_sharder_submit: queue a job, return its ticket at once.  imgs: (n, H, W) uint8 C-contiguous holding frames
        imgs_first_frame .. ; outputs as uvo_sharder_submit documents them (untouched until wait(ticket) returns)."""
        cap = self._check(imgs, total_frames, out_kp, out_desc, n_out, idx0, d0, idx1, d1)
        _, h, w = imgs.shape
        t = ctypes.c_int()
        rc = lib.uvo_sharder_submit(self._h, imgs.ctypes.data, imgs.shape[0], imgs_first_frame, total_frames, w, h, w, w * h, out_kp.ctypes.data, out_desc.ctypes.data, cap,
                                    n_out.ctypes.data, _ptr(idx0), _ptr(d0), _ptr(idx1), _ptr(d1), ctypes.byref(t))
        if rc:
            raise UvoError(rc, "uvo_sharder_submit")
        return t.value

    def wait(self, ticket):
        rc = lib.uvo_sharder_wait(self._h, int(ticket))
        if rc:
            raise UvoError(rc, "uvo_sharder_wait")

    def run(self, imgs, imgs_first_frame, total_frames, out_kp, out_desc, n_out, idx0=None, d0=None, idx1=None, d1=None):
        """submit + wait."""
        self.wait(self.submit(imgs, imgs_first_frame, total_frames, out_kp, out_desc, n_out, idx0, d0, idx1, d1))


def host_register(arr):
    """Page-lock memory the caller owns (uvo_host_register), e.g. a mapping shared between processes."""
    rc = lib.uvo_host_register(arr.ctypes.data, arr.nbytes)
    if rc:
        raise UvoError(rc, "uvo_host_register")


def host_bind_near_device(device):
    """uvo_host_bind_near_device: binds the calling thread to the CPUs local to `device`; -> (bound, numa_node) -- (False, -1) where the
    platform says nothing (placement is speed, never correctness)."""
    node = ctypes.c_int32(-1)
    rc = lib.uvo_host_bind_near_device(int(device), ctypes.byref(node))
    if rc < 0:
        raise UvoError(rc, "uvo_host_bind_near_device")
    return rc == 1, int(node.value)


def host_bind_to_cpulist_file(path):
    rc = lib.uvo_host_bind_to_cpulist_file(str(path).encode())
    if rc < 0:
        raise UvoError(rc, "uvo_host_bind_to_cpulist_file")
    return rc == 1


def host_unregister(arr):
    rc = lib.uvo_host_unregister(arr.ctypes.data)
    if rc:
        raise UvoError(rc, "uvo_host_unregister")


def _spread_rows(names, ms):
    """the "kernel:stat" pseudo-rows of a uvo_*_kernel_times report -> {kernel: {stat: ms}}"""
    out = {}
    for i, nm in enumerate(names):
        if ":" in nm:
            k, stat = nm.split(":", 1)
            out.setdefault(k, {})[stat] = float(ms[i])
    return out


OctreeTap = collections.namedtuple("OctreeTap", "selected sel_count cand_count fcount threads residue")


class ORBextractor:
    """Mirror of USLAM::ORBextractor (include/ORBextractor.h:47-95).

    ctor args follow the reference (nfeatures, scaleFactor, nlevels, scoreType, fastTh); the extra keyword
    arguments size the device scratch the handle owns.
    """
    HARRIS_SCORE, FAST_SCORE = 0, 1

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, scoreType=0, fastTh=7, *, max_width=640, max_height=512, max_batch=1,
                 max_input_keypoints=0, device=0):
        self.cfg = ExtractorCfg(nfeatures, scaleFactor, nlevels, scoreType, fastTh, max_width, max_height, max_batch, max_input_keypoints,
                                device)
        self._h = ctypes.c_void_p()
        rc = lib.uvo_extractor_create(ctypes.byref(self.cfg), ctypes.byref(self._h))
        if rc:
            self._h = None
            raise UvoError(rc, "uvo_extractor_create")
        scale = np.zeros(nlevels, np.float32)
        inv = np.zeros(nlevels, np.float32)
        quota = np.zeros(nlevels, np.int32)
        umax = np.zeros(16, np.int32)
        lib.uvo_extractor_tables(self._h, _ptr(scale), _ptr(inv), _ptr(quota), _ptr(umax))
        self.mvScaleFactor, self.mvInvScaleFactor, self.mnFeaturesPerLevel, self.umax = scale, inv, quota, umax
        # upper bound of keypoints per frame: sum(quota + 4) + pass-through keypoints
        self.cap = lib.uvo_extractor_max_keypoints(self._h)
        if self.cap < 0:
            raise UvoError(self.cap, "uvo_extractor_max_keypoints")

    def close(self):
        if getattr(self, "_h", None) and lib is not None:  # `lib` is already gone when the interpreter tears the module down
            lib.uvo_extractor_destroy(self._h)
            self._h = None

    __del__ = close

    def GetLevels(self):
        return lib.uvo_extractor_levels(self._h)

    def GetScaleFactor(self):
        return lib.uvo_extractor_scale_factor(self._h)

    def __call__(self, image, keypoints=None, grid_2d=None, min_px_dist=20, FullDetect=True, num_featsneeded=0):
        """operator()(image, mask, keypoints, descriptors, grid_2d, min_px_dist, FullDetect, num_featsneeded).

        image: HxW uint8.  keypoints: KEYPOINT_DTYPE array (the reference's in/out vector on entry) or None.
        grid_2d: int32 array of shape (rows, cols) in Fortran (column-major) order, mutated in place like the
        reference's Eigen::MatrixXi&.  Returns (keypoints, descriptors).
        """
        if image is None:      # the handle's last clahe() result, already in HBM
            h, w = self._clahe_shape
        else:
            image = np.ascontiguousarray(image, dtype=np.uint8)
            h, w = image.shape
        n_in = 0 if keypoints is None else len(keypoints)
        kin = None if n_in == 0 else np.ascontiguousarray(keypoints, dtype=KEYPOINT_DTYPE)
        rows = cols = 0
        if grid_2d is not None:
            if not (grid_2d.dtype == np.int32 and grid_2d.flags.f_contiguous):
                raise ValueError("grid_2d must be int32 and column-major (np.asfortranarray)")
            rows, cols = grid_2d.shape
        out_kp = np.zeros(self.cap, KEYPOINT_DTYPE)
        out_desc = np.zeros((self.cap, 32), np.uint8)
        n_out = ctypes.c_int(0)
        rc = lib.uvo_extract(self._h, _ptr(image), w, h, w if image is None else image.strides[0], _ptr(kin), n_in, _ptr(grid_2d), rows, cols, int(min_px_dist),
                             1 if FullDetect else 0, int(num_featsneeded), out_kp.ctypes.data, out_desc.ctypes.data, self.cap,
                             ctypes.byref(n_out))
        if rc:
            raise UvoError(rc, "uvo_extract")
        n = n_out.value
        return out_kp[:n].copy(), out_desc[:n].copy()

    def extract_tracked(self, image, keypoints, min_px_dist, num_featsneeded, want_grid=False):
        """uvo_extract_tracked: src/Tracking.cc:896-946 as one call -- occupancy grid from the tracked keypoints on the device, then the
        top-up extraction.  image None = the last clahe() result.  Returns (keypoints, descriptors[, grid (rows, cols) int32 F-order])."""
        if image is None:
            h, w = self._clahe_shape
        else:
            image = np.ascontiguousarray(image, dtype=np.uint8)
            h, w = image.shape
        kin = np.ascontiguousarray(keypoints, dtype=KEYPOINT_DTYPE)
        out_kp, out_desc, n_out = np.zeros(self.cap, KEYPOINT_DTYPE), np.zeros((self.cap, 32), np.uint8), ctypes.c_int(0)
        grid = np.zeros((h // min_px_dist + 2, w // min_px_dist + 2), np.int32, order="F") if want_grid else None
        rc = lib.uvo_extract_tracked(self._h, _ptr(image), w, h, w if image is None else image.strides[0], _ptr(kin) if len(kin) else None, len(kin),
                                     int(min_px_dist), int(num_featsneeded), out_kp.ctypes.data, out_desc.ctypes.data, self.cap, ctypes.byref(n_out),
                                     _ptr(grid))
        if rc:
            raise UvoError(rc, "uvo_extract_tracked")
        n = n_out.value
        return (out_kp[:n].copy(), out_desc[:n].copy()) + ((grid,) if want_grid else ())

    def extract_batch(self, images):
        """FullDetect extraction of a (B, H, W) uint8 stack; returns list of (keypoints, descriptors)."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        b, h, w = images.shape
        out_kp = np.zeros((b, self.cap), KEYPOINT_DTYPE)
        out_desc = np.zeros((b, self.cap, 32), np.uint8)
        n_out = np.zeros(b, np.int32)
        rc = lib.uvo_extract_batch(self._h, b, images.ctypes.data, w, h, images.strides[1], images.strides[0], None, None, None, 0, 0, 0, 1,
                                   None, out_kp.ctypes.data, out_desc.ctypes.data, self.cap, n_out.ctypes.data)
        if rc:
            raise UvoError(rc, "uvo_extract_batch")
        return [(out_kp[i, :n_out[i]].copy(), out_desc[i, :n_out[i]].copy()) for i in range(b)]

    def submit(self, images, out_kp, out_desc, n_out):
        """Asynchronous FullDetect extraction of a (B, H, W) uint8 stack into caller arrays out_kp (B, cap) KEYPOINT_DTYPE,
        out_desc (B, cap, 32) uint8, n_out (B,) int32 -- ideally all from pinned_empty(); returns the ticket for wait()."""
        assert images.dtype == np.uint8 and images.ndim == 3 and images.strides[2] == 1   # rows contiguous; row / frame strides are free
        b, h, w = images.shape
        cap = out_kp.shape[1]
        assert out_kp.dtype == KEYPOINT_DTYPE and out_kp.flags.c_contiguous and out_kp.shape[0] >= b
        assert out_desc.dtype == np.uint8 and out_desc.flags.c_contiguous and out_desc.shape[1:] == (cap, 32)
        assert n_out.dtype == np.int32 and len(n_out) >= b
        t = ctypes.c_int()
        rc = lib.uvo_extract_batch_submit(self._h, b, images.ctypes.data, w, h, images.strides[1], images.strides[0], out_kp.ctypes.data,
                                          out_desc.ctypes.data, cap, n_out.ctypes.data, ctypes.byref(t))
        if rc:
            raise UvoError(rc, "uvo_extract_batch_submit")
        return t.value

    def wait(self, ticket):
        rc = lib.uvo_extract_batch_wait(self._h, int(ticket))
        if rc:
            raise UvoError(rc, "uvo_extract_batch_wait")

    def extract_batch_device(self, d_imgs, batch, width, height, d_out_kp, d_out_desc, d_n_out, cap=None, stride=None, frame_stride=None):
        """HBM-resident FullDetect extraction; all arguments are integer device addresses (rows `stride` bytes apart, frames `frame_stride`;
        tight by default).  Asynchronous: the images must stay as they are until the batch is complete."""
        stride = stride or width
        rc = lib.uvo_extract_batch_device(self._h, batch, d_imgs, width, height, stride, frame_stride or stride * height, None, None, None, 0, 0, 0, 1, None,
                                          d_out_kp, d_out_desc, cap or self.cap, d_n_out)
        if rc:
            raise UvoError(rc, "uvo_extract_batch_device")

    def grider_fast(self, image, num_features, grid_x, grid_y, threshold, nms=True):
        """Grider_FAST::perform_griding (include/Grider_FAST.h:81-137)."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = image.shape
        # what the call can return: the per-ROI quota times the ROIs, of which there can be more than grid cells (w % grid_x >= w // grid_x)
        size_x, size_y = w // max(grid_x, 1), h // max(grid_y, 1)
        rois = (w // size_x) * (h // size_y) if size_x > 0 and size_y > 0 else 0
        cap = max((max(num_features, 0) // max(grid_x * grid_y, 1) + 1) * rois, 1)   # (a call the library refuses still needs a buffer)
        out = np.zeros(cap, KEYPOINT_DTYPE)
        n = ctypes.c_int()
        rc = lib.uvo_grider_fast(self._h, image.ctypes.data, w, h, image.strides[0], num_features, grid_x, grid_y, threshold,
                                 1 if nms else 0, out.ctypes.data, cap, ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_grider_fast")
        return out[:n.value].copy()

    def synchronize(self):
        rc = lib.uvo_extractor_synchronize(self._h)
        if rc:
            raise UvoError(rc, "uvo_extractor_synchronize")

    def set_pipeline(self, depth):
        rc = lib.uvo_extractor_set_pipeline(self._h, depth)
        if rc:
            raise UvoError(rc, "uvo_extractor_set_pipeline")

    def tune(self, knob, value):
        rc = lib.uvo_extractor_tune(self._h, knob, value)
        if rc:
            raise UvoError(rc, "uvo_extractor_tune")

    def fast_state(self):
        """uvo_extractor_fast_state: per level (threshold the next batch of the current lane streams at, fall-back cells counted in the
        last batch, cells per frame)."""
        n = lib.uvo_extractor_levels(self._h)
        t, f, c = (np.zeros(n, np.int32) for _ in range(3))
        rc = lib.uvo_extractor_fast_state(self._h, t.ctypes.data, f.ctypes.data, c.ctypes.data)
        if rc:
            raise UvoError(rc, "uvo_extractor_fast_state")
        return t, f, c

    # ---- stage taps used by the parity tests ----
    def level_dims(self, level):
        w, h = ctypes.c_int(), ctypes.c_int()
        rc = lib.uvo_extractor_level_dims(self._h, level, ctypes.byref(w), ctypes.byref(h))
        if rc:
            raise UvoError(rc, "uvo_extractor_level_dims")
        return w.value, h.value

    def clahe(self, img, clip_limit=4.0, tiles=(12, 12), download=True):
        """cv::CLAHE::apply as set up at src/Tracking.cc:425-431 (clip limit 4, 12 x 12 tiles); returns the enhanced image.
        The result also stays in the handle's HBM: ex(None, ...) extracts from it, KLT.build_pyramid_from(slot, ex) builds the
        optical-flow pyramid from it; download=False skips the copy back (returns None)."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        self._clahe_shape = (h, w)
        out = np.empty_like(img) if download else None
        rc = lib.uvo_clahe(self._h, _ptr(img), w, h, img.strides[0], float(clip_limit), int(tiles[0]), int(tiles[1]), _ptr(out),
                           out.strides[0] if download else 0)
        if rc:
            raise UvoError(rc, "uvo_clahe")
        return out

    def clahe_batch_device(self, d_src, batch, w, h, d_dst, clip_limit=4.0, tiles=(12, 12)):
        """HBM-resident form on tight [batch][h][w] buffers (device pointers); enqueued ahead of the next extract_batch_device."""
        rc = lib.uvo_clahe_batch_device(self._h, batch, d_src, w, h, w, w * h, float(clip_limit), int(tiles[0]), int(tiles[1]), d_dst, w, w * h)
        if rc:
            raise UvoError(rc, "uvo_clahe_batch_device")

    def read_plane(self, level, blurred=False, frame=0):
        w, h = self.level_dims(level)
        out = np.zeros((h + 32, w + 32), np.uint8)
        rc = lib.uvo_extractor_read_plane(self._h, frame, level, 1 if blurred else 0, out.ctypes.data)
        if rc:
            raise UvoError(rc, "uvo_extractor_read_plane")
        return out

    def read_candidates(self, level, frame=0, cap=1 << 20):
        buf = np.zeros((cap, 3), np.int32)
        n = ctypes.c_int()
        rc = lib.uvo_extractor_read_candidates(self._h, frame, level, buf.ctypes.data, cap, ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_extractor_read_candidates")
        return buf[:min(n.value, cap)].copy()

    def octree_tap(self, problems, cell_flags, sel_cap=2048):
        """uvo_extractor_octree_tap: the quad-tree launch on caller-given lists.  problems[frame][level] = (high, low), each an (n, 3)
        array of (x, y, score) relative to the detection border; cell_flags (frames, flags_per_frame) uint8.  -> OctreeTap with, per
        (frame, level), selected (list of (x, y, score) in the kernel's order), sel_count, cand_count, fcount (arrays (frames, levels)),
        and threads, residue (cursor words, flag bytes left non-zero)."""
        nl = lib.uvo_extractor_levels(self._h)
        batch = len(problems)
        lists = [[np.asarray(p[k], np.int32).reshape(-1, 3) for fr in problems for p in fr] for k in (0, 1)]
        if any(len(fr) != nl for fr in problems):
            raise UvoError(UVO_E_BADARG, "octree_tap: one (high, low) pair per level")
        n_hi, n_lo = (np.array([len(a) for a in lists[k]], np.int32) for k in (0, 1))
        hi, lo = (np.ascontiguousarray(np.concatenate(lists[k] + [np.zeros((1, 3), np.int32)])) for k in (0, 1))   # (never an empty buffer)
        cell_flags = np.ascontiguousarray(cell_flags, np.uint8).reshape(max(batch, 1), -1)
        sel_count, cand_count, fcount = (np.zeros(max(batch, 1) * nl, np.int32) for _ in range(3))
        sel = np.zeros((max(batch, 1) * nl, sel_cap, 3), np.int32)
        threads, residue = ctypes.c_int32(), np.zeros(2, np.int32)
        rc = lib.uvo_extractor_octree_tap(self._h, batch, n_hi.ctypes.data, n_lo.ctypes.data, hi.ctypes.data, lo.ctypes.data, cell_flags.ctypes.data,
                                          cell_flags.shape[1], sel_count.ctypes.data, cand_count.ctypes.data, fcount.ctypes.data, sel.ctypes.data, sel_cap,
                                          ctypes.byref(threads), residue.ctypes.data)
        if rc:
            raise UvoError(rc, "uvo_extractor_octree_tap")
        selected = [[list(map(tuple, sel[f * nl + l, :min(int(sel_count[f * nl + l]), sel_cap)].tolist())) for l in range(nl)] for f in range(batch)]
        return OctreeTap(selected, sel_count.reshape(batch, nl), cand_count.reshape(batch, nl), fcount.reshape(batch, nl), threads.value,
                         tuple(int(v) for v in residue))

    def profile(self, enable=True, only=None):
        """Per-kernel HIP-event timing; only = a kernel name restricts it to that kernel (two event records per launch cost ~3 %)."""
        lib.uvo_extractor_profile_only(self._h, only.encode() if only else None)
        lib.uvo_extractor_profile(self._h, 1 if enable else 0)

    def kernel_times(self):
        """{kernel: (summed ms, launches)}; the per-launch spread rows of the same report ("name:min" ...) are kept in self.last_spread
        as {kernel: {"min" | "p50" | "max" | "period_min" | "period_p50" | "period_max": ms}}."""
        names = ctypes.create_string_buffer(16384)
        ms = np.zeros(256, np.float32)
        launches = np.zeros(256, np.int32)
        n = ctypes.c_int()
        rc = lib.uvo_extractor_kernel_times(self._h, names, 16384, ms.ctypes.data, launches.ctypes.data, 256, ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_extractor_kernel_times")
        nm = names.value.decode().split("\n")[:n.value]
        self.last_spread = _spread_rows(nm, ms)
        return {nm[i]: (float(ms[i]), int(launches[i])) for i in range(n.value) if ":" not in nm[i]}


class ORBmatcher:
    """Mirror of the USLAM::ORBmatcher surface on the hot path (include/ORBmatcher.h:41-88)."""
    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio=0.6, checkOri=True, *, max_query=4096, max_train=4096, max_batch=1, max_map_points=8192, device=0):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        self.cfg = MatcherCfg(max_query, max_train, max_batch, max_map_points, device)
        self._h = ctypes.c_void_p()
        rc = lib.uvo_matcher_create(ctypes.byref(self.cfg), ctypes.byref(self._h))
        if rc:
            self._h = None
            raise UvoError(rc, "uvo_matcher_create")

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.uvo_matcher_destroy(self._h)
            self._h = None

    __del__ = close

    def knn2(self, q, t, mask=None):
        """All-pairs knn-2 (include/utils.h:100-101).  Returns idx0, d0, idx1, d1."""
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        nq, nt = len(q), len(t)
        idx0 = np.full(nq, -1, np.int32)
        idx1 = np.full(nq, -1, np.int32)
        d0 = np.full(nq, 0xFFFF, np.uint16)
        d1 = np.full(nq, 0xFFFF, np.uint16)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        rc = lib.uvo_hamming_knn2(self._h, _ptr(q), nq, _ptr(t), nt, _ptr(m), _ptr(idx0), _ptr(d0), _ptr(idx1), _ptr(d1))
        if rc:
            raise UvoError(rc, "uvo_hamming_knn2")
        return idx0, d0, idx1, d1

    def ratio_matching(self, q, t, ratio, mask=None):
        """Utils::ratioMatching (include/utils.h:81-111): (queryIdx, trainIdx, distance) of accepted matches."""
        if len(q) == 0 or len(t) == 0:
            return np.zeros((0, 3), np.int32)
        idx0, d0, idx1, d1 = self.knn2(q, t, mask)
        ok = (idx1 >= 0) & (d0.astype(np.float32).astype(np.float64) <= d1.astype(np.float32).astype(np.float64) * float(ratio))
        qi = np.nonzero(ok)[0].astype(np.int32)
        return np.stack([qi, idx0[qi], d0[qi].astype(np.int32)], 1)

    def distance_matrix(self, q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        out = np.zeros((len(q), len(t)), np.uint16)
        rc = lib.uvo_hamming_matrix(self._h, _ptr(q), len(q), _ptr(t), len(t), _ptr(out))
        if rc:
            raise UvoError(rc, "uvo_hamming_matrix")
        return out

    def distinctive_descriptors(self, desc_lists):
        """MapPoint::ComputeDistinctiveDescriptors for a batch of map points (src/MapPoint.cc:197-270).
        desc_lists: list of (n_i, 32) uint8 arrays.  Returns (best_idx, best_median) int32 arrays."""
        offs = np.zeros(len(desc_lists) + 1, np.int32)
        offs[1:] = np.cumsum([len(d) for d in desc_lists])
        allv = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in desc_lists if len(d)]
        allv = np.concatenate(allv) if allv else np.zeros((0, 32), np.uint8)
        idx = np.zeros(len(desc_lists), np.int32)
        med = np.zeros(len(desc_lists), np.int32)
        rc = lib.uvo_distinctive_descriptors(self._h, _ptr(allv) if len(allv) else None, _ptr(offs), len(desc_lists), _ptr(idx), _ptr(med))
        if rc:
            raise UvoError(rc, "uvo_distinctive_descriptors")
        return idx, med

    def knn2_batch_device(self, pairs, d_q, d_nq, q_stride, d_t, d_nt, t_stride, d_idx0, d_d0, d_idx1, d_d1):
        rc = lib.uvo_hamming_knn2_batch_device(self._h, pairs, d_q, d_nq, q_stride, d_t, d_nt, t_stride, d_idx0, d_d0, d_idx1, d_d1)
        if rc:
            raise UvoError(rc, "uvo_hamming_knn2_batch_device")

    def synchronize(self):
        rc = lib.uvo_matcher_synchronize(self._h)
        if rc:
            raise UvoError(rc, "uvo_matcher_synchronize")

    def wait_extractor(self, ex):
        rc = lib.uvo_matcher_wait_extractor(self._h, ex._h)
        if rc:
            raise UvoError(rc, "uvo_matcher_wait_extractor")

    def attach(self, ex):
        """Enqueue the matcher's work in the stream of the extractor's current lane from now on (None: back to its own stream)."""
        rc = lib.uvo_matcher_attach_extractor(self._h, ex._h if ex is not None else None)
        if rc:
            raise UvoError(rc, "uvo_matcher_attach_extractor")

    def release_to_extractor(self, ex):
        rc = lib.uvo_extractor_wait_matcher(ex._h, self._h)
        if rc:
            raise UvoError(rc, "uvo_extractor_wait_matcher")

    def profile(self, enable=True):
        lib.uvo_matcher_profile(self._h, 1 if enable else 0)

    def kernel_times(self):
        """{kernel: (summed ms, launches)}; the per-launch spread rows of the same report ("name:min" ...) are kept in self.last_spread
        as {kernel: {"min" | "p50" | "max" | "period_min" | "period_p50" | "period_max": ms}}."""
        names = ctypes.create_string_buffer(16384)
        ms = np.zeros(256, np.float32)
        launches = np.zeros(256, np.int32)
        n = ctypes.c_int()
        rc = lib.uvo_matcher_kernel_times(self._h, names, 16384, ms.ctypes.data, launches.ctypes.data, 256, ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_matcher_kernel_times")
        nm = names.value.decode().split("\n")[:n.value]
        self.last_spread = _spread_rows(nm, ms)
        return {nm[i]: (float(ms[i]), int(launches[i])) for i in range(n.value) if ":" not in nm[i]}

    def SearchByProjection(self, kp, desc, bounds, assigned, proj_x, proj_y, level, view_cos, in_view, mp_desc, scale_factors, th=1.0):
        """SearchByProjection(FrameKTL&, vector<MapPoint*>&, th) (src/ORBmatcher.cc:49-125).

        kp/desc: frame keypoints (KEYPOINT_DTYPE) and descriptors; bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY);
        assigned: int32[n] in/out (-1 = F.mvpMapPoints[i] is NULL).  Returns nmatches.
        """
        kp = np.ascontiguousarray(kp, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        px, py = np.ascontiguousarray(proj_x, np.float32), np.ascontiguousarray(proj_y, np.float32)
        lv, vc = np.ascontiguousarray(level, np.int32), np.ascontiguousarray(view_cos, np.float32)
        iv, md = np.ascontiguousarray(in_view, np.uint8), np.ascontiguousarray(mp_desc, np.uint8)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        assert assigned.dtype == np.int32 and assigned.flags.c_contiguous
        nm = ctypes.c_int()
        rc = lib.uvo_search_by_projection(self._h, _ptr(kp), len(kp), _ptr(desc), int(bounds[0]), int(bounds[1]), int(bounds[2]), int(bounds[3]),
                                          _ptr(assigned), len(px), _ptr(px), _ptr(py), _ptr(lv), _ptr(vc), _ptr(iv), _ptr(md), _ptr(sf), len(sf),
                                          float(th), self.mfNNratio, ctypes.byref(nm))
        if rc:
            raise UvoError(rc, "uvo_search_by_projection")
        return nm.value


    # ---- the other search loops (generic engine + reference-named entry points) ----
    def match_windows(self, kp, desc, bounds, qx, qy, qr, qmin_level, qmax_level, qvalid, qdesc, rule, max_dist, *, blocked=None, qangle=None,
                      exclusive=True, check_orientation=False):
        """uvo_match_windows: candidates from 64x48 grid windows over kp; returns (match[nq], dist[nq], nmatches)."""
        kp = np.ascontiguousarray(kp, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        a = [np.ascontiguousarray(v, np.float32) for v in (qx, qy, qr)]
        lo, hi = np.ascontiguousarray(qmin_level, np.int32), np.ascontiguousarray(qmax_level, np.int32)
        qv, qd = np.ascontiguousarray(qvalid, np.uint8), np.ascontiguousarray(qdesc, np.uint8)
        bl = None if blocked is None else np.ascontiguousarray(blocked, np.uint8)
        qa = None if qangle is None else np.ascontiguousarray(qangle, np.float32)
        nq = len(a[0])
        match, dist, nm = np.full(nq, -1, np.int32), np.full(nq, -1, np.int32), ctypes.c_int()
        r = MatchRule(rule, max_dist, self.mfNNratio, 1 if exclusive else 0, 1 if check_orientation else 0)
        rc = lib.uvo_match_windows(self._h, _ptr(kp), len(kp), _ptr(desc), _ptr(bl), int(bounds[0]), int(bounds[1]), int(bounds[2]), int(bounds[3]),
                                   nq, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(lo), _ptr(hi), _ptr(qv), _ptr(qd), _ptr(qa), ctypes.byref(r),
                                   _ptr(match), _ptr(dist), ctypes.byref(nm))
        if rc:
            raise UvoError(rc, "uvo_match_windows")
        return match, dist, nm.value

    def SearchByProjectionKF(self, kp, desc, bounds, assigned, u, v, level, valid, mp_desc, kf_angle, scale_factors, th, ORBdist):
        """SearchByProjection(FrameKTL& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1622-1746),
        from the projected (u, v, level) of the key frame's map points.  assigned in/out; returns nmatches."""
        kp = np.ascontiguousarray(kp, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        uu, vv = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
        lv, va = np.ascontiguousarray(level, np.int32), np.ascontiguousarray(valid, np.uint8)
        md, ka = np.ascontiguousarray(mp_desc, np.uint8), np.ascontiguousarray(kf_angle, np.float32)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        assert assigned.dtype == np.int32 and assigned.flags.c_contiguous
        nm = ctypes.c_int()
        rc = lib.uvo_search_by_projection_kf(self._h, _ptr(kp), len(kp), _ptr(desc), int(bounds[0]), int(bounds[1]), int(bounds[2]), int(bounds[3]),
                                             _ptr(assigned), len(uu), _ptr(uu), _ptr(vv), _ptr(lv), _ptr(va), _ptr(md), _ptr(ka), _ptr(sf), len(sf),
                                             float(th), int(ORBdist), 1 if self.mbCheckOrientation else 0, ctypes.byref(nm))
        if rc:
            raise UvoError(rc, "uvo_search_by_projection_kf")
        return nm.value

    def SearchByBoW(self, fv1, desc1, angle1, usable1, fv2, desc2, angle2, usable2=None, kf_kf=False):
        """SearchByBoW(KeyFrame*, FrameKTL&, ...) (:155-284) / SearchByBoW(KeyFrame*, KeyFrame*, ...) (:715-850, kf_kf=True).
        Returns (match12[n1], nmatches)."""
        d1, d2 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(desc2, np.uint8)
        a1, a2 = np.ascontiguousarray(angle1, np.float32), np.ascontiguousarray(angle2, np.float32)
        u1 = np.ascontiguousarray(usable1, np.uint8)
        u2 = None if usable2 is None else np.ascontiguousarray(usable2, np.uint8)
        match = np.full(len(d1), -1, np.int32)
        nm = ctypes.c_int()
        rc = lib.uvo_search_by_bow(self._h, 1 if kf_kf else 0, ctypes.byref(fv1.c), len(d1), _ptr(d1), _ptr(a1), _ptr(u1), ctypes.byref(fv2.c), len(d2),
                                   _ptr(d2), _ptr(a2), _ptr(u2), self.mfNNratio, 1 if self.mbCheckOrientation else 0, _ptr(match), ctypes.byref(nm))
        if rc:
            raise UvoError(rc, "uvo_search_by_bow")
        return match, nm.value

    def SearchForTriangulation(self, fv1, kp1, desc1, has_mp1, fv2, kp2, desc2, has_mp2, F12, sigma2):
        """SearchForTriangulation(pKF1, pKF2, F12, ...) (:852-1014).  Returns (match12[n1], nmatches)."""
        kp1, kp2 = np.ascontiguousarray(kp1, KEYPOINT_DTYPE), np.ascontiguousarray(kp2, KEYPOINT_DTYPE)
        d1, d2 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(desc2, np.uint8)
        h1, h2 = np.ascontiguousarray(has_mp1, np.uint8), np.ascontiguousarray(has_mp2, np.uint8)
        f, s2 = np.ascontiguousarray(F12, np.float32).reshape(9), np.ascontiguousarray(sigma2, np.float32)
        match = np.full(len(kp1), -1, np.int32)
        nm = ctypes.c_int()
        rc = lib.uvo_search_for_triangulation(self._h, ctypes.byref(fv1.c), _ptr(kp1), len(kp1), _ptr(d1), _ptr(h1), ctypes.byref(fv2.c), _ptr(kp2),
                                              len(kp2), _ptr(d2), _ptr(h2), _ptr(f), _ptr(s2), len(s2), 1 if self.mbCheckOrientation else 0,
                                              _ptr(match), ctypes.byref(nm))
        if rc:
            raise UvoError(rc, "uvo_search_for_triangulation")
        return match, nm.value

    def SearchForTriangulationBatch(self, fv1, kp1, desc1, has_mp1, pairs):
        """uvo_search_for_triangulation_batch: the distances + epipolar tests of every (pKF1, pKF2_k) pair of CreateNewMapPoints' loop
        (src/LocalMapping.cc:1058-1080) in one launch.  pairs = [(fv2, kp2, desc2, has_mp2, F12, sigma2), ...].  Follow with
        SearchForTriangulationNext(k, has_mp1 as it is then) per pair."""
        kp1 = np.ascontiguousarray(kp1, KEYPOINT_DTYPE)
        d1, h1 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(has_mp1, np.uint8)
        keep = [kp1, d1, h1, fv1]
        arr = (TriangulationPairC * max(len(pairs), 1))()
        for k, (fv2, kp2, desc2, has_mp2, F12, sigma2) in enumerate(pairs):
            kp2 = np.ascontiguousarray(kp2, KEYPOINT_DTYPE)
            d2, h2 = np.ascontiguousarray(desc2, np.uint8), np.ascontiguousarray(has_mp2, np.uint8)
            s2 = np.ascontiguousarray(sigma2, np.float32)
            keep += [fv2, kp2, d2, h2, s2]
            arr[k].fv2, arr[k].kp2, arr[k].n2, arr[k].desc2, arr[k].has_mp2 = ctypes.addressof(fv2.c), _ptr(kp2), len(kp2), _ptr(d2), _ptr(h2)
            arr[k].f12[:] = [float(x) for x in np.asarray(F12, np.float32).reshape(9)]
            arr[k].sigma2, arr[k].nlevels = _ptr(s2), len(s2)
        rc = lib.uvo_search_for_triangulation_batch(self._h, ctypes.byref(fv1.c), _ptr(kp1), len(kp1), _ptr(d1), _ptr(h1), len(pairs), arr)
        if rc:
            raise UvoError(rc, "uvo_search_for_triangulation_batch")
        self._tri_n1 = len(kp1)

    def SearchForTriangulationNext(self, pair, has_mp1_now):
        """uvo_search_for_triangulation_next: the acceptance loop of src/ORBmatcher.cc:886-984 for one pair of the batch, on the host.
        Returns (match12[n1], nmatches)."""
        h1 = np.ascontiguousarray(has_mp1_now, np.uint8)
        match = np.full(self._tri_n1, -1, np.int32)
        nm = ctypes.c_int()
        rc = lib.uvo_search_for_triangulation_next(self._h, int(pair), _ptr(h1), 1 if self.mbCheckOrientation else 0, _ptr(match), ctypes.byref(nm))
        if rc:
            raise UvoError(rc, "uvo_search_for_triangulation_next")
        return match, nm.value

    def TriangulateMatches(self, cam1, cam2, ratio_factor, kp1, kp2):
        """uvo_triangulate_matches: the triangulation of src/LocalMapping.cc:1096-1180 for a list of matched undistorted key points
        (kp1[j] <-> kp2[j]).  cam1 / cam2: TriangulationCamera.  Returns (verdict[n] of TRI_*, x3d[n][3])."""
        kp1, kp2 = np.ascontiguousarray(kp1, KEYPOINT_DTYPE), np.ascontiguousarray(kp2, KEYPOINT_DTYPE)
        assert len(kp1) == len(kp2)
        n = len(kp1)
        verdict, x3d = np.full(n, -1, np.int32), np.zeros((n, 3), np.float32)
        rc = lib.uvo_triangulate_matches(self._h, ctypes.byref(cam1.c), ctypes.byref(cam2.c), float(ratio_factor), _ptr(kp1), _ptr(kp2), n, _ptr(verdict),
                                         _ptr(x3d))
        if rc:
            raise UvoError(rc, "uvo_triangulate_matches")
        return verdict, x3d

    def CreateNewMapPoints(self, fv1, kp1, desc1, has_mp1, pairs, cam1, cams2, ratio_factor):
        """uvo_create_new_map_points: the loop of src/LocalMapping.cc:1058-1199 in one call -- per pair, in order, on the device: the
        acceptance loop of SearchForTriangulation with key frame 1's map points as they are by then, the triangulation of the pair's
        matches, has_mp1 = 1 for the accepted ones.  pairs as in SearchForTriangulationBatch; cam1 and cams2[k]: TriangulationCamera.
        Returns (per_pair, has_mp1_after): per_pair[k] = dict(idx1, idx2, verdict, x3d, n_accepted), the matches in ascending idx1."""
        kp1 = np.ascontiguousarray(kp1, KEYPOINT_DTYPE)
        d1, h1 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(has_mp1, np.uint8)
        keep = [kp1, d1, h1, fv1]
        assert len(cams2) == len(pairs)
        arr = (TriangulationPairC * max(len(pairs), 1))()
        cams = (TriangulationCameraC * max(len(pairs), 1))()
        for k, (fv2, kp2, desc2, has_mp2, F12, sigma2) in enumerate(pairs):
            kp2 = np.ascontiguousarray(kp2, KEYPOINT_DTYPE)
            d2, h2 = np.ascontiguousarray(desc2, np.uint8), np.ascontiguousarray(has_mp2, np.uint8)
            s2 = np.ascontiguousarray(sigma2, np.float32)
            keep += [fv2, kp2, d2, h2, s2]
            arr[k].fv2, arr[k].kp2, arr[k].n2, arr[k].desc2, arr[k].has_mp2 = ctypes.addressof(fv2.c), _ptr(kp2), len(kp2), _ptr(d2), _ptr(h2)
            arr[k].f12[:] = [float(x) for x in np.asarray(F12, np.float32).reshape(9)]
            arr[k].sigma2, arr[k].nlevels = _ptr(s2), len(s2)
            cams[k] = cams2[k].c
        P, n1 = len(pairs), len(kp1)
        nm, na = np.zeros(max(P, 1), np.int32), np.zeros(max(P, 1), np.int32)
        idx1, idx2 = np.full((max(P, 1), max(n1, 1)), -1, np.int32), np.full((max(P, 1), max(n1, 1)), -1, np.int32)
        verdict, x3d = np.full((max(P, 1), max(n1, 1)), -1, np.int32), np.zeros((max(P, 1), max(n1, 1), 3), np.float32)
        h_out = np.zeros(max(n1, 1), np.uint8)
        out = NewMapPointsC(_ptr(nm), _ptr(na), _ptr(idx1), _ptr(idx2), _ptr(verdict), _ptr(x3d), _ptr(h_out))
        rc = lib.uvo_create_new_map_points(self._h, ctypes.byref(fv1.c), _ptr(kp1), n1, _ptr(d1), _ptr(h1), P, arr, ctypes.byref(cam1.c), cams,
                                           float(ratio_factor), 1 if self.mbCheckOrientation else 0, ctypes.byref(out))
        if rc:
            raise UvoError(rc, "uvo_create_new_map_points")
        per_pair = [dict(idx1=idx1[k, :nm[k]].copy(), idx2=idx2[k, :nm[k]].copy(), verdict=verdict[k, :nm[k]].copy(), x3d=x3d[k, :nm[k]].copy(),
                         n_accepted=int(na[k])) for k in range(P)]
        return per_pair, h_out[:n1].copy()

    def FuseBatch(self, targets, xyz, normal, min_distance, max_distance, usable, mp_desc, th=3.0):
        """uvo_fuse_batch: projection tests + search core of Fuse (:1037-1101) for every (target key frame, map point) in one pass.
        targets = [(kp, desc, cam (CameraPose), scale_factors), ...]; min_distance / max_distance = the map points' mfMinDistance /
        mfMaxDistance (the invariance bounds x 0.8f / x 1.2f are formed here, as in project_points).  Returns
        (best_idx[n_targets][nmp], best_dist[n_targets][nmp])."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        mn_inv = (np.float32(0.8) * np.ascontiguousarray(min_distance, np.float32)).astype(np.float32)
        mx_inv = (np.float32(1.2) * np.ascontiguousarray(max_distance, np.float32)).astype(np.float32)
        us = None if usable is None else np.ascontiguousarray(usable, np.uint8)
        md = np.ascontiguousarray(mp_desc, np.uint8)
        nmp = len(xyz)
        keep = []
        arr = (FuseTargetC * max(len(targets), 1))()
        for t, (kp, desc, cam, sf) in enumerate(targets):
            kp, desc, sf = np.ascontiguousarray(kp, KEYPOINT_DTYPE), np.ascontiguousarray(desc, np.uint8), np.ascontiguousarray(sf, np.float32)
            keep += [kp, desc, sf]
            arr[t].kp, arr[t].n, arr[t].desc = _ptr(kp), len(kp), _ptr(desc)
            arr[t].min_x, arr[t].min_y, arr[t].max_x, arr[t].max_y = int(cam.min_x), int(cam.min_y), int(cam.max_x), int(cam.max_y)
            arr[t].cam = cam
            arr[t].scale_factors, arr[t].nlevels = _ptr(sf), len(sf)
        bi, bd = np.full((len(targets), nmp), -1, np.int32), np.full((len(targets), nmp), -1, np.int32)
        rc = lib.uvo_fuse_batch(self._h, len(targets), arr, nmp, _ptr(xyz), _ptr(nrm), _ptr(mn_inv), _ptr(mx_inv), _ptr(us), _ptr(md), float(th), _ptr(bi), _ptr(bd))
        if rc:
            raise UvoError(rc, "uvo_fuse_batch")
        return bi, bd

    def project_points(self, mode, cam, xyz, normal, min_distance, max_distance, usable, scale_factors, scale_factor=1.2, viewing_cos_limit=0.5):
        """uvo_project_points: FrameKTL::isInFrustum (PROJECT_FRUSTUM), the projection prologue of SearchByProjection(F, pKF, ...)
        (PROJECT_KF_RELOC) or of Fuse (PROJECT_FUSE).  min_distance / max_distance are the map points' mfMinDistance / mfMaxDistance
        members; the invariance bounds (x 0.8f, x 1.2f: MapPoint::GetMin/MaxDistanceInvariance) are formed here in fp32.
        Returns (valid, u, v, level, view_cos)."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = None if normal is None else np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        mx = None if max_distance is None else np.ascontiguousarray(max_distance, np.float32)
        mn_inv = None if min_distance is None else (np.float32(0.8) * np.ascontiguousarray(min_distance, np.float32)).astype(np.float32)
        mx_inv = None if mx is None else (np.float32(1.2) * mx).astype(np.float32)
        us = None if usable is None else np.ascontiguousarray(usable, np.uint8)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        n = len(xyz)
        valid, u, v = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32)
        level, vc = np.zeros(n, np.int32), np.zeros(n, np.float32)
        rc = lib.uvo_project_points(self._h, int(mode), ctypes.byref(cam), n, _ptr(xyz), _ptr(nrm), _ptr(mn_inv), _ptr(mx_inv), _ptr(mx), _ptr(us), _ptr(sf), len(sf),
                                    float(scale_factor), float(viewing_cos_limit), _ptr(valid), _ptr(u), _ptr(v), _ptr(level), _ptr(vc))
        if rc:
            raise UvoError(rc, "uvo_project_points")
        return valid, u, v, level, vc

    # ---- the four members of the reference class that nothing in the reference calls (src/ORBmatcher.cc:409-713, :1507-1620) ----
    def WindowSearch(self, kp1, desc1, has_mp1, kp2, desc2, bounds2, windowSize, minScaleLevel=-1, maxScaleLevel=0x7fffffff):
        """WindowSearch(F1, F2, windowSize, vpMapPointMatches2, minScaleLevel, maxScaleLevel) (:409-516).  has_mp1[i1] = F1's keypoint
        holds a good map point.  Returns (match21[n2] = index into F1 or -1, nmatches)."""
        kp1 = np.ascontiguousarray(kp1, KEYPOINT_DTYPE)
        lv = kp1["octave"].astype(np.int32)
        valid = np.ascontiguousarray(has_mp1, np.uint8).copy()
        if minScaleLevel > 0:
            valid &= (lv >= minScaleLevel).astype(np.uint8)
        if maxScaleLevel < 0x7fffffff:
            valid &= (lv <= maxScaleLevel).astype(np.uint8)
        m12, _, nm = self.match_windows(kp2, desc2, bounds2, kp1["x"], kp1["y"], np.full(len(kp1), float(windowSize), np.float32), lv, lv, valid, desc1,
                                        RULE_BEST_RATIO_LEQ, 100, qangle=kp1["angle"], exclusive=True, check_orientation=self.mbCheckOrientation)
        m21 = np.full(len(kp2), -1, np.int32)
        sel = np.nonzero(m12 >= 0)[0]
        m21[m12[sel]] = sel
        return m21, nm

    def SearchByProjectionFrames(self, kp1, desc1, usable1, xyz1, cam2, kp2, desc2, assigned2, windowSize):
        """SearchByProjection(F1, F2, windowSize, vpMapPointMatches2) (:519-594).  usable1[i1]: F1's map point exists, is good and is not
        one of F2's already; cam2: F2's pose / intrinsics / bounds; assigned2 in/out (>= 0 = F2's keypoint holds a map point; new
        matches get the F1 index).  Returns nmatches."""
        kp1 = np.ascontiguousarray(kp1, KEYPOINT_DTYPE)
        n1 = len(kp1)
        valid, u, v, _, _ = self.project_points(PROJECT_PIXEL, cam2, xyz1, None, None, None, usable1, np.ones(1, np.float32))
        lv = kp1["octave"].astype(np.int32)
        bounds = (int(cam2.min_x), int(cam2.min_y), int(cam2.max_x), int(cam2.max_y))
        m12, _, nm = self.match_windows(kp2, desc2, bounds, u, v, np.full(n1, float(windowSize), np.float32), lv, lv, valid, desc1, RULE_BEST_RATIO_LEQ, 100,
                                        blocked=(assigned2 >= 0).astype(np.uint8), exclusive=True, check_orientation=False)
        sel = np.nonzero(m12 >= 0)[0]
        assigned2[m12[sel]] = sel
        return nm

    def SearchForInitialization(self, kp1, desc1, kp2, desc2, bounds2, prev_matched, windowSize=10):
        """SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (:598-713).  prev_matched: float32 [n1][2], updated in
        place for the matched keypoints (:705-708).  Returns (vnMatches12[n1], nmatches)."""
        kp1, kp2 = np.ascontiguousarray(kp1, KEYPOINT_DTYPE), np.ascontiguousarray(kp2, KEYPOINT_DTYPE)
        n1 = len(kp1)
        assert prev_matched.dtype == np.float32 and prev_matched.shape == (n1, 2)
        lv = kp1["octave"].astype(np.int32)
        valid = (lv <= 0).astype(np.uint8)                                   # :621-622: level 0 only
        m12, _, nm = self.match_windows(kp2, desc2, bounds2, prev_matched[:, 0].copy(), prev_matched[:, 1].copy(), np.full(n1, float(windowSize), np.float32),
                                        lv, lv, valid, desc1, RULE_INIT_STEAL, 50, qangle=kp1["angle"], exclusive=False,
                                        check_orientation=self.mbCheckOrientation)
        sel = np.nonzero(m12 >= 0)[0]
        prev_matched[sel, 0], prev_matched[sel, 1] = kp2["x"][m12[sel]], kp2["y"][m12[sel]]
        return m12, nm

    def SearchByProjectionLast(self, kp, desc, assigned, cam, usable_last, xyz_last, octave_last, angle_last, desc_last, scale_factors, th):
        """SearchByProjection(CurrentFrame, LastFrame, th) (:1507-1620): LastFrame's map points projected with the current pose, window
        th * scale[octave] on levels [octave-1, octave+1], best <= TH_HIGH, first come first served, rotation histogram.  assigned
        in/out (new matches hold the LastFrame index).  Returns nmatches."""
        valid, u, v, _, _ = self.project_points(PROJECT_PIXEL_BOUNDED, cam, xyz_last, None, None, None, usable_last, scale_factors)
        bounds = (int(cam.min_x), int(cam.min_y), int(cam.max_x), int(cam.max_y))
        return self.SearchByProjectionKF(kp, desc, bounds, assigned, u, v, np.ascontiguousarray(octave_last, np.int32), valid, desc_last, angle_last,
                                         scale_factors, th, 100)

    def haloc_hash(self, proj, desc):
        """haloc::Hash::getHash (src/hash.cpp:57-85): proj [num_proj][>= n] float32, desc [n][32] -> hash [num_proj * 32]."""
        proj = np.ascontiguousarray(proj, np.float32)
        desc = np.ascontiguousarray(desc, np.uint8)
        out = np.zeros(proj.shape[0] * 32, np.float32)
        rc = lib.uvo_haloc_hash(self._h, _ptr(proj), proj.shape[0], proj.shape[1], _ptr(desc), len(desc), _ptr(out))
        if rc:
            raise UvoError(rc, "uvo_haloc_hash")
        return out

    def SearchPointsInFrustum(self, kp, desc, assigned, cam, xyz, normal, min_distance, max_distance, usable, mp_desc, scale_factors,
                              scale_factor=1.2, viewing_cos_limit=0.5, th=1.0, want_projections=False):
        """Tracking::SearchReferencePointsInFrustum (src/Tracking.cc:2176-2230) in one call: isInFrustum on every map point, then
        SearchByProjection on the ones in view.  assigned (int32[n], -1 = free) is updated in place.  Returns (n_matches, in_view) or
        (n_matches, in_view, u, v, level, view_cos)."""
        kp = np.ascontiguousarray(kp, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        assert assigned.dtype == np.int32 and assigned.flags.c_contiguous and len(assigned) == len(kp)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        mx = np.ascontiguousarray(max_distance, np.float32)
        mn_inv = (np.float32(0.8) * np.ascontiguousarray(min_distance, np.float32)).astype(np.float32)
        mx_inv = (np.float32(1.2) * mx).astype(np.float32)
        us = None if usable is None else np.ascontiguousarray(usable, np.uint8)
        md, sf = np.ascontiguousarray(mp_desc, np.uint8), np.ascontiguousarray(scale_factors, np.float32)
        n = len(xyz)
        in_view = np.zeros(n, np.uint8)
        u = v = lv = vc = None
        if want_projections:
            u, v, lv, vc = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        ntm, nm = ctypes.c_int(), ctypes.c_int()
        rc = lib.uvo_search_points_in_frustum(self._h, _ptr(kp), len(kp), _ptr(desc), _ptr(assigned), ctypes.addressof(cam), n, _ptr(xyz), _ptr(nrm),
                                              _ptr(mn_inv), _ptr(mx_inv), _ptr(mx), _ptr(us), _ptr(md), _ptr(sf), len(sf), float(scale_factor),
                                              float(viewing_cos_limit), float(th), self.mfNNratio, _ptr(in_view), _ptr(u), _ptr(v), _ptr(lv),
                                              _ptr(vc), ctypes.byref(ntm), ctypes.byref(nm))
        if rc:
            raise UvoError(rc, "uvo_search_points_in_frustum")
        assert ntm.value == int(in_view.sum())
        return (nm.value, in_view, u, v, lv, vc) if want_projections else (nm.value, in_view)

    @staticmethod
    def sim3_decompose(scw, cam):
        """Head of SearchByProjection(pKF, Scw, ...) / Fuse(pKF, Scw, ...) (:299-303): fills cam.rcw / tcw / ow from a 4x4 (or 3x4) Scw."""
        scw = np.ascontiguousarray(scw, np.float32)
        assert scw.ndim == 2 and scw.shape[0] >= 3 and scw.shape[1] == 4
        rc = lib.uvo_sim3_decompose(_ptr(scw), 4, ctypes.addressof(cam))
        if rc:
            raise UvoError(rc, "uvo_sim3_decompose")
        return cam

    @staticmethod
    def sim3_relative(s12, r12, t12):
        """SearchBySim3 :1284-1287: returns (sR12, sR21, t21)."""
        r12, t12 = np.ascontiguousarray(r12, np.float32).reshape(3, 3), np.ascontiguousarray(t12, np.float32).reshape(3)
        a, b, c = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), np.zeros(3, np.float32)
        rc = lib.uvo_sim3_relative(float(s12), _ptr(r12), _ptr(t12), _ptr(a), _ptr(b), _ptr(c))
        if rc:
            raise UvoError(rc, "uvo_sim3_relative")
        return a, b, c

    def project_sim3(self, r_own, t_own, s_r, t, cam_other, xyz, min_distance, max_distance, usable, scale_factors):
        """Per-point prologue of one direction of SearchBySim3 (:1323-1359).  min_distance / max_distance = mfMinDistance / mfMaxDistance
        (the invariance bounds x 0.8f / x 1.2f are formed here).  Returns (valid, u, v, level)."""
        ro, to = np.ascontiguousarray(r_own, np.float32).reshape(9), np.ascontiguousarray(t_own, np.float32).reshape(3)
        sr, tt = np.ascontiguousarray(s_r, np.float32).reshape(9), np.ascontiguousarray(t, np.float32).reshape(3)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        mn_inv = (np.float32(0.8) * np.ascontiguousarray(min_distance, np.float32)).astype(np.float32)
        mx_inv = (np.float32(1.2) * np.ascontiguousarray(max_distance, np.float32)).astype(np.float32)
        us = None if usable is None else np.ascontiguousarray(usable, np.uint8)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        n = len(xyz)
        valid, u, v, level = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        rc = lib.uvo_project_sim3(self._h, _ptr(ro), _ptr(to), _ptr(sr), _ptr(tt), ctypes.addressof(cam_other), n, _ptr(xyz), _ptr(mn_inv), _ptr(mx_inv),
                                  _ptr(us), _ptr(sf), len(sf), _ptr(valid), _ptr(u), _ptr(v), _ptr(level))
        if rc:
            raise UvoError(rc, "uvo_project_sim3")
        return valid, u, v, level

    def SearchByProjectionSim3(self, kp, desc, bounds, matched, u, v, level, valid, mp_desc, scale_factors, th):
        """Search core of SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (:357-398).  matched (int32[n], >= 0 = taken) is
        updated in place; returns the number of new matches."""
        kp = np.ascontiguousarray(kp, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        assert matched.dtype == np.int32 and matched.flags.c_contiguous and len(matched) == len(kp)
        uu, vv = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
        lv, va = np.ascontiguousarray(level, np.int32), np.ascontiguousarray(valid, np.uint8)
        md, sf = np.ascontiguousarray(mp_desc, np.uint8), np.ascontiguousarray(scale_factors, np.float32)
        nm = ctypes.c_int()
        rc = lib.uvo_search_by_projection_sim3(self._h, _ptr(kp), len(kp), _ptr(desc), int(bounds[0]), int(bounds[1]), int(bounds[2]), int(bounds[3]),
                                               _ptr(matched), len(uu), _ptr(uu), _ptr(vv), _ptr(lv), _ptr(va), _ptr(md), _ptr(sf), len(sf), int(th),
                                               ctypes.byref(nm))
        if rc:
            raise UvoError(rc, "uvo_search_by_projection_sim3")
        return nm.value

    def SearchBySim3(self, kp1, desc1, bounds1, kp2, desc2, bounds2, proj12, mp_desc1, proj21, mp_desc2, scale_factors1, scale_factors2, th):
        """SearchBySim3 (:1361-1504) after the projections: proj12 = (valid, u, v, level) of KF1's points in KF2, proj21 the reverse.
        Returns (match12[n1], n_found)."""
        kp1, kp2 = np.ascontiguousarray(kp1, KEYPOINT_DTYPE), np.ascontiguousarray(kp2, KEYPOINT_DTYPE)
        d1, d2 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(desc2, np.uint8)
        b1, b2 = np.ascontiguousarray(bounds1, np.int32), np.ascontiguousarray(bounds2, np.int32)
        va12, u12, v12, l12 = (np.ascontiguousarray(proj12[0], np.uint8), np.ascontiguousarray(proj12[1], np.float32),
                               np.ascontiguousarray(proj12[2], np.float32), np.ascontiguousarray(proj12[3], np.int32))
        va21, u21, v21, l21 = (np.ascontiguousarray(proj21[0], np.uint8), np.ascontiguousarray(proj21[1], np.float32),
                               np.ascontiguousarray(proj21[2], np.float32), np.ascontiguousarray(proj21[3], np.int32))
        m1, m2 = np.ascontiguousarray(mp_desc1, np.uint8), np.ascontiguousarray(mp_desc2, np.uint8)
        s1, s2 = np.ascontiguousarray(scale_factors1, np.float32), np.ascontiguousarray(scale_factors2, np.float32)
        match12 = np.full(len(kp1), -1, np.int32)
        nf = ctypes.c_int()
        rc = lib.uvo_search_by_sim3(self._h, _ptr(kp1), len(kp1), _ptr(d1), _ptr(b1), _ptr(kp2), len(kp2), _ptr(d2), _ptr(b2), _ptr(u12), _ptr(v12),
                                    _ptr(l12), _ptr(va12), _ptr(m1), _ptr(u21), _ptr(v21), _ptr(l21), _ptr(va21), _ptr(m2), _ptr(s1), len(s1), _ptr(s2),
                                    len(s2), float(th), _ptr(match12), ctypes.byref(nf))
        if rc:
            raise UvoError(rc, "uvo_search_by_sim3")
        return match12, nf.value

    def FuseSearch(self, kp, desc, bounds, u, v, level, valid, mp_desc, scale_factors, th=3.0):
        """Search core of Fuse (:1077-1101): (best_idx[nmp], best_dist[nmp]), -1 where nothing within TH_LOW."""
        kp = np.ascontiguousarray(kp, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        uu, vv = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
        lv, va = np.ascontiguousarray(level, np.int32), np.ascontiguousarray(valid, np.uint8)
        md, sf = np.ascontiguousarray(mp_desc, np.uint8), np.ascontiguousarray(scale_factors, np.float32)
        bi, bd = np.full(len(uu), -1, np.int32), np.full(len(uu), -1, np.int32)
        rc = lib.uvo_fuse(self._h, _ptr(kp), len(kp), _ptr(desc), int(bounds[0]), int(bounds[1]), int(bounds[2]), int(bounds[3]), len(uu), _ptr(uu),
                          _ptr(vv), _ptr(lv), _ptr(va), _ptr(md), _ptr(sf), len(sf), float(th), _ptr(bi), _ptr(bd))
        if rc:
            raise UvoError(rc, "uvo_fuse")
        return bi, bd


class VocabularyDesc(ctypes.Structure):
    """uvo_vocabulary_desc."""
    _fields_ = [("n_nodes", ctypes.c_int32), ("child_start", ctypes.c_void_p), ("children", ctypes.c_void_p), ("descriptor", ctypes.c_void_p),
                ("word_id", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("L", ctypes.c_int32), ("weighting", ctypes.c_int32),
                ("normalize", ctypes.c_int32), ("device", ctypes.c_int32)]


class ORBVocabulary:
    """DBoW2 ORBVocabulary stand-in holding the tree on the device: transform() = TemplatedVocabulary::transform
    (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1125-1258).  Tree given flat: children of node i =
    children[child_start[i]:child_start[i+1]] (node 0 = root), descriptor[n_nodes][32], word_id[n_nodes], weight[n_nodes]."""
    TF_IDF, TF, IDF, BINARY = range(4)

    def __init__(self, child_start, children, descriptor, word_id, weight, L, weighting=0, normalize=1, device=0):
        self._k = [np.ascontiguousarray(child_start, np.int32), np.ascontiguousarray(children, np.int32), np.ascontiguousarray(descriptor, np.uint8),
                   np.ascontiguousarray(word_id, np.int32), np.ascontiguousarray(weight, np.float64)]
        d = VocabularyDesc(len(self._k[0]) - 1, _ptr(self._k[0]), _ptr(self._k[1]), _ptr(self._k[2]), _ptr(self._k[3]), _ptr(self._k[4]), int(L),
                           int(weighting), int(normalize), int(device))
        self._h = ctypes.c_void_p()
        rc = lib.uvo_vocabulary_create(ctypes.byref(d), ctypes.byref(self._h))
        if rc:
            raise UvoError(rc, "uvo_vocabulary_create")

    def close(self):
        if self._h:
            lib.uvo_vocabulary_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transform(self, desc, levelsup=4):
        """Returns (word_id[n], weight[n], node_id[n], BowVector as (ids, values), FeatureVector)."""
        desc = np.ascontiguousarray(desc, np.uint8)
        n = len(desc)
        wid, nid, ww = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
        bid, bval = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float64)
        fnode, fstart, ffeat = np.zeros(max(n, 1), np.uint32), np.zeros(n + 2, np.int32), np.zeros(max(n, 1), np.int32)
        nb, nf = ctypes.c_int(), ctypes.c_int()
        rc = lib.uvo_bow_transform(self._h, _ptr(desc), n, int(levelsup), _ptr(wid), _ptr(ww), _ptr(nid), _ptr(bid), _ptr(bval), len(bid), ctypes.byref(nb),
                                   _ptr(fnode), _ptr(fstart), _ptr(ffeat), len(fnode), ctypes.byref(nf))
        if rc:
            raise UvoError(rc, "uvo_bow_transform")
        groups = {int(fnode[j]): [int(x) for x in ffeat[fstart[j]:fstart[j + 1]]] for j in range(nf.value)}
        return wid, ww, nid, (bid[:nb.value].copy(), bval[:nb.value].copy()), FeatureVector(groups)


class CameraModel(ctypes.Structure):
    """uvo_camera_model: mK and mDistCoef of the reference's Tracking object (pin-hole: k1 k2 p1 p2 [k3 ..]; fisheye: 4 coefficients)."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("dist", ctypes.c_float * 8),
                ("n_dist", ctypes.c_int32), ("fisheye", ctypes.c_int32)]

    @classmethod
    def make(cls, fx, fy, cx, cy, dist, fisheye=False):
        c = cls(fx, fy, cx, cy)
        for i, v in enumerate(dist):
            c.dist[i] = v
        c.n_dist, c.fisheye = len(dist), 1 if fisheye else 0
        return c


UVO_FM_NONE, UVO_FM_SEVEN_POINT, UVO_FM_RANSAC, UVO_FM_LMEDS = 0, 1, 2, 3
FM_MAX_HYPOTHESES = 1000


class FmInfo(ctypes.Structure):
    """uvo_fm_info."""
    _fields_ = [("method", ctypes.c_int32), ("iterations", ctypes.c_int32), ("inliers", ctypes.c_int32), ("rng_draws", ctypes.c_uint32)]

    def astuple(self):
        return (self.method, self.iterations, self.inliers, self.rng_draws)


class PnpInfo(ctypes.Structure):
    """uvo_pnp_info."""
    _fields_ = [("ok", ctypes.c_int32), ("iterations", ctypes.c_int32), ("inliers", ctypes.c_int32), ("rng_draws", ctypes.c_uint32)]

    def astuple(self):
        return (self.ok, self.iterations, self.inliers, self.rng_draws)


class GlibcRand(ctypes.Structure):
    """uvo_glibc_rand: glibc's srand / rand as a value the caller owns (the reference's DUtils::Random::RandomInt runs on it, never
    seeded: srand(1)).  The library's iterate call advances it by exactly the draws the reference would have made."""
    _fields_ = [("r", ctypes.c_int32 * 34), ("k", ctypes.c_int32)]

    def __init__(self, seed=1):
        super().__init__()
        lib.uvo_glibc_srand(ctypes.byref(self), int(seed))

    def next(self):
        return lib.uvo_glibc_rand_next(ctypes.byref(self))

    def copy(self):
        g = GlibcRand.__new__(GlibcRand)
        ctypes.memmove(ctypes.byref(g), ctypes.byref(self), ctypes.sizeof(GlibcRand))
        return g

    def state(self):
        return bytes(self)


class PnPsolverParams(ctypes.Structure):
    """uvo_pnpsolver_params; the defaults are Relocalisation's SetRansacParameters(0.99,10,300,4,0.5,5.991)."""
    _fields_ = [("probability", ctypes.c_double), ("min_inliers", ctypes.c_int32), ("max_iterations", ctypes.c_int32), ("min_set", ctypes.c_int32),
                ("epsilon", ctypes.c_float), ("th2", ctypes.c_float)]

    def __init__(self, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991):
        super().__init__(probability, min_inliers, max_iterations, min_set, epsilon, th2)


class PnPsolverInfo(ctypes.Structure):
    """uvo_pnpsolver_info."""
    _fields_ = [("n", ctypes.c_int32), ("min_inliers", ctypes.c_int32), ("max_its", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("best_inliers", ctypes.c_int32)]


class PnPsolverStatus(ctypes.Structure):
    """uvo_pnpsolver_status."""
    _fields_ = [("touched", ctypes.c_int32), ("no_more", ctypes.c_int32), ("iterations", ctypes.c_int32)]


class PnPsolverResultC(ctypes.Structure):
    """uvo_pnpsolver_result."""
    _fields_ = [("returned", ctypes.c_int32), ("solver", ctypes.c_int32), ("n_inliers", ctypes.c_int32), ("refined", ctypes.c_int32),
                ("Tcw", ctypes.c_float * 16), ("draws", ctypes.c_uint32), ("pad_", ctypes.c_int32), ("status", ctypes.c_void_p),
                ("inliers", ctypes.c_void_p), ("inliers_cap", ctypes.c_int32), ("pad2_", ctypes.c_int32)]


class PnPsolverResult:
    """One iterate call: returned (position in ids, -1: none), solver (its id), n_inliers, refined, Tcw float32[4, 4], draws,
    status int32[n_ids, 3] (touched, bNoMore, mnIterations), inliers uint8[n_matches of the returning solver] (empty when none)."""

    def __init__(self, c, status, inliers):
        self.returned, self.solver, self.n_inliers, self.refined, self.draws = c.returned, c.solver, c.n_inliers, c.refined, c.draws
        self.Tcw = np.array(c.Tcw, np.float32).reshape(4, 4)
        self.status, self.inliers = status, inliers


class _SolverSet:
    """What PnPsolverSet and Sim3SolverSet share (csrc/solver_set.hpp behind both): a set made by `<_prefix>set_create` on a handle and
    freed by `<_prefix>set_destroy`, and the one call that marshals status, mask and inliers_cap.  A subclass names `_prefix`, `_info`,
    `_result_c` and `_result`.  `_api` / `_prefix` exist so that the tests' host build of the same source can be driven through the
    very subclass; errors name the library's function (`_where`) either way."""

    def __init__(self, handle, max_solvers, max_points, _api=None):
        self._api = _api if _api is not None else lib
        self._handle = handle   # the set launches in the handle's stream: keep it alive
        self._h = ctypes.c_void_p()
        self._n_matches = []
        rc = self._f("set_create")(handle._h if handle is not None else None, max_solvers, max_points, ctypes.byref(self._h))
        if rc:
            raise UvoError(rc, self._where + "set_create")

    def _f(self, name):
        return getattr(self._api, self._prefix + name)

    def _do(self, name, *args):
        rc = self._f(name)(self._h, *args)
        if rc:
            raise UvoError(rc, self._where + name)

    def close(self):
        if getattr(self, "_h", None) and self._api is not None:
            self._f("set_destroy")(self._h)
            self._h = None

    __del__ = close

    def clear(self):
        self._do("set_clear")
        self._n_matches = []

    def _added(self, n_matches, *args):
        sid = ctypes.c_int()
        self._do("add", *args, ctypes.byref(sid))
        self._n_matches.append(n_matches)
        return sid.value

    def query(self, sid):
        info = self._info()
        self._do("query", sid, ctypes.byref(info))
        return info

    def _call(self, name, ids, inliers_cap, *args):
        status = np.zeros((len(ids), 3), np.int32)
        cap = max([self._n_matches[i] for i in ids if 0 <= i < len(self._n_matches)] + [1]) if inliers_cap is None else int(inliers_cap)
        mask = np.zeros(max(cap, 1), np.uint8)
        res = self._result_c()
        res.status, res.inliers, res.inliers_cap = status.ctypes.data, mask.ctypes.data, cap
        rc = self._f(name)(self._h, *args, ctypes.byref(res))   # not through _do: one Python call less on the path that is timed
        if rc:
            raise UvoError(rc, self._where + name)
        return self._result(res, status, mask[:self._n_matches[res.solver]].copy() if res.returned >= 0 else mask[:0].copy())

    def iterate(self, ids, n_iterations, rng, inliers_cap=None):
        """iterate(n_iterations) on each id in order until one returns; rng (GlibcRand) is advanced in place -> the subclass's result."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        return self._call("iterate", ids, inliers_cap, _ptr(ids), len(ids), int(n_iterations), ctypes.byref(rng))

    def _tap(self, sid, cap, *arrays):
        """The arrays of a test tap, filled by `<_prefix>hypotheses` and cut to the hypotheses `sid` consumed in the last iterate call."""
        n = ctypes.c_int()
        self._do("hypotheses", sid, *(_ptr(a) for a in arrays), cap, ctypes.byref(n))
        return tuple(a[:n.value].copy() for a in arrays)


class PnPsolverSet(_SolverSet):
    """USLAM::PnPsolver for Tracking::Relocalisation (src/Tracking.cc:2415-2517): the solvers of all candidate key frames in one set on
    a KLT handle, iterate() over a list of them as one device call -> PnPsolverResult."""
    _prefix = _where = "uvo_pnpsolver_"
    _info, _result_c, _result = PnPsolverInfo, PnPsolverResultC, PnPsolverResult

    def __init__(self, klt, max_solvers, max_points, _api=None):
        super().__init__(klt, max_solvers, max_points, _api)

    def add(self, p3d, p2d, sigma2, kp_index=None, n_matches=None, K=(1.0, 1.0, 0.0, 0.0), params=None):
        """PnPsolver(F, vpMapPointMatches) + SetRansacParameters -> solver id.  kp_index defaults to 0..n-1, n_matches to n."""
        a = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
        sg = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
        kp = np.arange(len(a), dtype=np.int32) if kp_index is None else np.ascontiguousarray(kp_index, np.int32).reshape(-1)
        if not (len(a) == len(b) == len(sg) == len(kp)):
            raise ValueError("p3d, p2d, sigma2 and kp_index differ in length")
        nm = len(a) if n_matches is None else int(n_matches)
        prm = params if params is not None else PnPsolverParams()
        return self._added(nm, _ptr(a), _ptr(b), _ptr(sg), _ptr(kp), len(a), nm, K[0], K[1], K[2], K[3], ctypes.byref(prm))

    def find(self, sid, rng):
        """PnPsolver::find: iterate(mRansacMaxIts)."""
        return self.iterate([sid], self.query(sid).max_its, rng)

    def hypotheses(self, sid, min_set=4, cap=1024):
        """Test tap: (subsets int32[h, min_set], poses float64[h, 12], counts int32[h]) solver `sid` consumed in the last iterate call."""
        return self._tap(sid, cap, np.zeros((cap, min_set), np.int32), np.zeros((cap, 12)), np.zeros(cap, np.int32))


class PoseProblemC(ctypes.Structure):
    """uvo_pose_problem."""
    _fields_ = [("p3d", ctypes.c_void_p), ("p2d", ctypes.c_void_p), ("inv_sigma2", ctypes.c_void_p), ("n", ctypes.c_int32), ("fx", ctypes.c_float),
                ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("Tcw", ctypes.c_float * 16), ("pad_", ctypes.c_int32)]


class PoseResultC(ctypes.Structure):
    """uvo_pose_result."""
    _fields_ = [("Tcw", ctypes.c_float * 16), ("n_inliers", ctypes.c_int32), ("rounds", ctypes.c_int32), ("outlier", ctypes.c_void_p),
                ("outlier_cap", ctypes.c_int32), ("pad_", ctypes.c_int32)]


class PoseTraceLin(ctypes.Structure):
    """uvo_pose_trace_lin."""
    _fields_ = [("round", ctypes.c_int32), ("iteration", ctypes.c_int32), ("H", ctypes.c_double * 21), ("b", ctypes.c_double * 6), ("chi2", ctypes.c_double)]


class PoseTraceTrial(ctypes.Structure):
    """uvo_pose_trace_trial."""
    _fields_ = [("lin", ctypes.c_int32), ("ok", ctypes.c_int32), ("accepted", ctypes.c_int32), ("pad_", ctypes.c_int32), ("lambda_", ctypes.c_double),
                ("cur", ctypes.c_double), ("tmp", ctypes.c_double), ("scale", ctypes.c_double)]


class PoseTraceC(ctypes.Structure):
    """uvo_pose_trace."""
    _fields_ = [("n_lin", ctypes.c_int32), ("n_trials", ctypes.c_int32), ("R", ctypes.c_double * 9), ("t", ctypes.c_double * 3),
                ("lin", PoseTraceLin * 32), ("trial", PoseTraceTrial * 320)]


POSE_LIN_DTYPE = np.dtype([("round", "<i4"), ("iteration", "<i4"), ("H", "<f8", 21), ("b", "<f8", 6), ("chi2", "<f8")])
POSE_TRIAL_DTYPE = np.dtype([("lin", "<i4"), ("ok", "<i4"), ("accepted", "<i4"), ("pad_", "<i4"), ("lambda", "<f8"), ("cur", "<f8"), ("tmp", "<f8"),
                             ("scale", "<f8")])


class PoseTrace:
    """The test tap of one problem: R float64[3, 3], t float64[3], lin (POSE_LIN_DTYPE, one record per linearisation), trial
    (POSE_TRIAL_DTYPE, one per Levenberg trial)."""

    def __init__(self, c):
        self.R, self.t = np.array(c.R, np.float64).reshape(3, 3), np.array(c.t, np.float64)
        self.lin = np.frombuffer(bytes(c.lin), POSE_LIN_DTYPE)[:c.n_lin].copy()
        self.trial = np.frombuffer(bytes(c.trial), POSE_TRIAL_DTYPE)[:c.n_trials].copy()


class PoseResult:
    """One optimised problem: Tcw float32[4, 4], n_inliers (the reference's return value), rounds, outlier uint8[n]."""

    def __init__(self, c, outlier):
        self.Tcw = np.array(c.Tcw, np.float32).reshape(4, 4)
        self.n_inliers, self.rounds, self.outlier = c.n_inliers, c.rounds, outlier


class PoseOptimizer:
    """Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:2012-2145) on a KLT handle: optimize() takes a list of independent problems
    and runs them as one device call.  `_api` exists so that the tests can drive another build through this class."""

    def __init__(self, klt, max_problems=1, max_points=4096, _api=None):
        self._api = _api if _api is not None else lib
        self._klt = klt   # the set launches in the handle's stream: keep it alive
        self._h = ctypes.c_void_p()
        self.max_problems, self.max_points = max_problems, max_points
        rc = self._api.uvo_pose_optimizer_create(klt._h if klt is not None else None, max_problems, max_points, ctypes.byref(self._h))
        if rc:
            self._h = None
            raise UvoError(rc, "uvo_pose_optimizer_create")

    def close(self):
        if getattr(self, "_h", None) and self._api is not None:
            self._api.uvo_pose_optimizer_destroy(self._h)
            self._h = None

    __del__ = close

    def optimize(self, problems, outlier_cap=None):
        """problems: a list of (p3d [n, 3], p2d [n, 2], inv_sigma2 [n], K = (fx, fy, cx, cy), Tcw [4, 4]) -> a list of PoseResult.
        outlier_cap (for the tests): the mask capacity passed for every problem instead of its n."""
        cp = (PoseProblemC * max(len(problems), 1))()
        cr = (PoseResultC * max(len(problems), 1))()
        keep, masks = [], []
        for j, (p3d, p2d, w, K, Tcw) in enumerate(problems):
            a = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
            b = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
            c = np.ascontiguousarray(w, np.float32).reshape(-1)
            if not (len(a) == len(b) == len(c)):
                raise ValueError("p3d, p2d and inv_sigma2 differ in length")
            T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
            m = np.zeros(max(len(a), 1), np.uint8)
            keep.append((a, b, c))
            masks.append(m)
            cp[j].p3d, cp[j].p2d, cp[j].inv_sigma2, cp[j].n = a.ctypes.data, b.ctypes.data, c.ctypes.data, len(a)
            cp[j].fx, cp[j].fy, cp[j].cx, cp[j].cy = [float(v) for v in K]
            cp[j].Tcw = (ctypes.c_float * 16)(*T.tolist())
            cr[j].outlier, cr[j].outlier_cap = m.ctypes.data, len(a) if outlier_cap is None else outlier_cap
        rc = self._api.uvo_pose_optimize(self._h, cp, len(problems), cr)
        if rc:
            raise UvoError(rc, "uvo_pose_optimize")
        return [PoseResult(cr[j], masks[j][:cp[j].n].copy()) for j in range(len(problems))]

    def trace(self, problem=0):
        """Test tap: PoseTrace of problem `problem` of the last optimize() call."""
        c = PoseTraceC()
        rc = self._api.uvo_pose_optimizer_trace(self._h, problem, ctypes.byref(c))
        if rc:
            raise UvoError(rc, "uvo_pose_optimizer_trace")
        return PoseTrace(c)


class NavStateC(ctypes.Structure):
    """uvo_nav_state: P, V, q (x y z w), bg, ba, dbg, dba."""
    _fields_ = [("P", ctypes.c_double * 3), ("V", ctypes.c_double * 3), ("q", ctypes.c_double * 4), ("bg", ctypes.c_double * 3), ("ba", ctypes.c_double * 3),
                ("dbg", ctypes.c_double * 3), ("dba", ctypes.c_double * 3)]

    def set(self, s):
        """s: a dict of arrays under the field names."""
        for k, _ in self._fields_:
            getattr(self, k)[:] = [float(v) for v in np.asarray(s[k], np.float64).reshape(-1)]
        return self

    def get(self):
        return {k: np.array(getattr(self, k), np.float64) for k, _ in self._fields_}


_D = ctypes.c_double


class NavProblemC(ctypes.Structure):
    """uvo_nav_problem."""
    _fields_ = [("form", ctypes.c_int32), ("has_depth", ctypes.c_int32), ("compute_marg", ctypes.c_int32), ("n", ctypes.c_int32), ("n_last", ctypes.c_int32),
                ("pad_", ctypes.c_int32), ("cur", NavStateC), ("last", NavStateC), ("dT", _D), ("dP", _D * 3), ("dV", _D * 3), ("dR", _D * 9), ("JPg", _D * 9),
                ("JPa", _D * 9), ("JVg", _D * 9), ("JVa", _D * 9), ("JRg", _D * 9), ("cov_pvphi", _D * 81), ("gw", _D * 3), ("Rbc", _D * 9), ("Pbc", _D * 3),
                ("fx", _D), ("fy", _D), ("cx", _D), ("cy", _D), ("gyr_bias_rw2", _D), ("acc_bias_rw2", _D), ("prior", NavStateC), ("prior_info", _D * 225),
                ("depth_meas", _D), ("shi", _D), ("depth_info", _D), ("p3d", ctypes.c_void_p), ("p2d", ctypes.c_void_p), ("inv_sigma2", ctypes.c_void_p),
                ("p3d_last", ctypes.c_void_p), ("p2d_last", ctypes.c_void_p), ("inv_sigma2_last", ctypes.c_void_p)]


class NavResultC(ctypes.Structure):
    """uvo_nav_result."""
    _fields_ = [("ns", NavStateC), ("Tcw", ctypes.c_float * 16), ("n_inliers", ctypes.c_int32), ("rounds", ctypes.c_int32), ("marg_ok", ctypes.c_int32),
                ("outlier_cap", ctypes.c_int32), ("outlier_last_cap", ctypes.c_int32), ("pad_", ctypes.c_int32), ("outlier", ctypes.c_void_p),
                ("outlier_last", ctypes.c_void_p), ("marg_cov", _D * 225), ("marg_cov_inv", _D * 225)]


class NavTraceLin(ctypes.Structure):
    """uvo_nav_trace_lin."""
    _fields_ = [("round", ctypes.c_int32), ("iteration", ctypes.c_int32), ("H", _D * 465), ("b", _D * 30), ("chi2", _D)]


class NavTraceC(ctypes.Structure):
    """uvo_nav_trace."""
    _fields_ = [("n_lin", ctypes.c_int32), ("n_trials", ctypes.c_int32), ("lin", NavTraceLin * 40), ("trial", PoseTraceTrial * 400)]


NAV_KEYFRAME, NAV_FRAME = 0, 1
NAV_LIN_DTYPE = np.dtype([("round", "<i4"), ("iteration", "<i4"), ("H", "<f8", 465), ("b", "<f8", 30), ("chi2", "<f8")])


class NavTrace:
    """The test tap of one problem: lin (NAV_LIN_DTYPE, one record per linearisation; H the packed upper triangle of the 15 x 15 or
    30 x 30 matrix), trial (POSE_TRIAL_DTYPE, one per Levenberg trial)."""

    def __init__(self, c):
        self.lin = np.frombuffer(bytes(c.lin), NAV_LIN_DTYPE)[:c.n_lin].copy()
        self.trial = np.frombuffer(bytes(c.trial), POSE_TRIAL_DTYPE)[:c.n_trials].copy()


class NavResult:
    """One optimised problem: ns (the recovered NavState, a dict of arrays), Tcw float32[4, 4] by UpdatePoseFromNS, n_inliers, rounds,
    outlier uint8[n], outlier_last uint8[n_last], marg_cov and marg_cov_inv float64[15, 15], marg_ok."""

    def __init__(self, c, outlier, outlier_last):
        self.ns = c.ns.get()
        self.Tcw = np.array(c.Tcw, np.float32).reshape(4, 4)
        self.n_inliers, self.rounds, self.marg_ok, self.outlier, self.outlier_last = c.n_inliers, c.rounds, c.marg_ok, outlier, outlier_last
        self.marg_cov, self.marg_cov_inv = np.array(c.marg_cov, np.float64).reshape(15, 15), np.array(c.marg_cov_inv, np.float64).reshape(15, 15)


class NavOptimizer:
    """The two IMU overloads of Optimizer::PoseOptimization (src/Optimizer.cc:319-777 the frame form, :779-1103 the key-frame form) on a
    KLT handle: optimize() takes a list of independent problems and runs them as one device call."""

    def __init__(self, klt, max_problems=1, max_points=4096, _api=None):
        self._api = _api if _api is not None else lib
        self._klt = klt   # the set launches in the handle's stream: keep it alive
        self._h = ctypes.c_void_p()
        self.max_problems, self.max_points = max_problems, max_points
        rc = self._api.uvo_nav_optimizer_create(klt._h if klt is not None else None, max_problems, max_points, ctypes.byref(self._h))
        if rc:
            self._h = None
            raise UvoError(rc, "uvo_nav_optimizer_create")

    def close(self):
        if getattr(self, "_h", None) and self._api is not None:
            self._api.uvo_nav_optimizer_destroy(self._h)
            self._h = None

    __del__ = close

    @staticmethod
    def problem(sc, keep):
        """A NavProblemC of a problem given as a dict: form, has_depth, compute_marg, cur, last, prior (dicts of P V q bg ba dbg dba), dT, dP,
        dV, dR, JPg, JPa, JVg, JVa, JRg, cov, gw, Rbc, Pbc, K = (fx, fy, cx, cy), gyr_rw2, acc_rw2, prior_info, depth_meas, shi, depth_info,
        edges [n, 6] and edges_last [n_last, 6] (point, observation, invSigma2).  keep: a list that takes the arrays the record points into."""
        c = NavProblemC()
        c.form, c.has_depth, c.compute_marg = int(sc["form"]), int(bool(sc["has_depth"])), int(bool(sc["compute_marg"]))
        c.cur.set(sc["cur"]), c.last.set(sc["last"]), c.prior.set(sc["prior"])
        for k, name in (("dP", "dP"), ("dV", "dV"), ("dR", "dR"), ("JPg", "JPg"), ("JPa", "JPa"), ("JVg", "JVg"), ("JVa", "JVa"), ("JRg", "JRg"), ("cov", "cov_pvphi"),
                        ("gw", "gw"), ("Rbc", "Rbc"), ("Pbc", "Pbc"), ("prior_info", "prior_info")):
            getattr(c, name)[:] = [float(v) for v in np.asarray(sc[k], np.float64).reshape(-1)]
        c.dT, c.gyr_bias_rw2, c.acc_bias_rw2 = float(sc["dT"]), float(sc["gyr_rw2"]), float(sc["acc_rw2"])
        c.fx, c.fy, c.cx, c.cy = [float(v) for v in sc["K"]]
        c.depth_meas, c.shi, c.depth_info = float(sc["depth_meas"]), float(sc["shi"]), float(sc["depth_info"])
        for key, names in (("edges", ("p3d", "p2d", "inv_sigma2")), ("edges_last", ("p3d_last", "p2d_last", "inv_sigma2_last"))):
            e = np.asarray(sc.get(key, np.zeros((0, 6))), np.float32).reshape(-1, 6)
            parts = [np.ascontiguousarray(e[:, :3]), np.ascontiguousarray(e[:, 3:5]), np.ascontiguousarray(e[:, 5])]
            keep.append(parts)
            for nm, a in zip(names, parts):
                setattr(c, nm, a.ctypes.data if len(e) else None)
            if key == "edges":
                c.n = len(e)
            else:
                c.n_last = len(e)
        return c

    def optimize(self, problems, outlier_cap=None):
        """problems: a list of dicts (see problem()) -> a list of NavResult.  outlier_cap (for the tests): the capacity passed for every
        mask instead of its count."""
        cp = (NavProblemC * max(len(problems), 1))()
        cr = (NavResultC * max(len(problems), 1))()
        keep, masks = [], []
        for j, sc in enumerate(problems):
            cp[j] = self.problem(sc, keep)
            m, ml = np.zeros(max(cp[j].n, 1), np.uint8), np.zeros(max(cp[j].n_last, 1), np.uint8)
            masks.append((m, ml))
            cr[j].outlier, cr[j].outlier_last = m.ctypes.data, ml.ctypes.data
            cr[j].outlier_cap = cp[j].n if outlier_cap is None else outlier_cap
            cr[j].outlier_last_cap = cp[j].n_last if outlier_cap is None else outlier_cap
        rc = self._api.uvo_nav_optimize(self._h, cp, len(problems), cr)
        if rc:
            raise UvoError(rc, "uvo_nav_optimize")
        return [NavResult(cr[j], masks[j][0][:cp[j].n].copy(), masks[j][1][:cp[j].n_last if cp[j].form == NAV_FRAME else 0].copy()) for j in range(len(problems))]

    def trace(self, problem=0):
        """Test tap: NavTrace of problem `problem` of the last optimize() call."""
        c = NavTraceC()
        rc = self._api.uvo_nav_optimizer_trace(self._h, problem, ctypes.byref(c))
        if rc:
            raise UvoError(rc, "uvo_nav_optimizer_trace")
        return NavTrace(c)


class Sim3SolverParams(ctypes.Structure):
    """uvo_sim3solver_params; the defaults are ComputeSim3's SetRansacParameters(0.99,2,300) (src/LoopClosing.cc:410)."""
    _fields_ = [("probability", ctypes.c_double), ("min_inliers", ctypes.c_int32), ("max_iterations", ctypes.c_int32)]

    def __init__(self, probability=0.99, min_inliers=2, max_iterations=300):
        super().__init__(probability, min_inliers, max_iterations)


class Sim3KeyFrame(ctypes.Structure):
    """uvo_sim3_keyframe: Rcw (row-major), tcw, fx, fy, cx, cy of one key frame."""
    _fields_ = [("Rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float),
                ("cy", ctypes.c_float)]

    @staticmethod
    def make(Rcw, tcw, K):
        kf = Sim3KeyFrame()
        kf.Rcw[:] = [float(v) for v in np.asarray(Rcw, np.float32).reshape(9)]
        kf.tcw[:] = [float(v) for v in np.asarray(tcw, np.float32).reshape(3)]
        kf.fx, kf.fy, kf.cx, kf.cy = (float(np.float32(v)) for v in K)
        return kf


class Sim3SolverInfo(ctypes.Structure):
    """uvo_sim3solver_info."""
    _fields_ = [("n", ctypes.c_int32), ("max_its", ctypes.c_int32), ("iterations", ctypes.c_int32), ("best_inliers", ctypes.c_int32)]


class Sim3SolverResultC(ctypes.Structure):
    """uvo_sim3solver_result."""
    _fields_ = [("returned", ctypes.c_int32), ("solver", ctypes.c_int32), ("n_inliers", ctypes.c_int32), ("draws", ctypes.c_uint32),
                ("T12", ctypes.c_float * 16), ("R12", ctypes.c_float * 9), ("t12", ctypes.c_float * 3), ("scale", ctypes.c_float), ("pad_", ctypes.c_int32),
                ("status", ctypes.c_void_p), ("inliers", ctypes.c_void_p), ("inliers_cap", ctypes.c_int32), ("pad2_", ctypes.c_int32)]


class Sim3SolverResult:
    """One iterate call: returned (position in ids, -1: none), solver (its id), n_inliers, draws, T12 float32[4, 4], R float32[3, 3],
    t float32[3], s, status int32[n_ids, 3] (touched, bNoMore, mnIterations), inliers uint8[n_matches of the returning solver]."""

    def __init__(self, c, status, inliers):
        self.returned, self.solver, self.n_inliers, self.draws = c.returned, c.solver, c.n_inliers, c.draws
        self.T12 = np.array(c.T12, np.float32).reshape(4, 4)
        self.R, self.t, self.s = np.array(c.R12, np.float32).reshape(3, 3), np.array(c.t12, np.float32), np.float32(c.scale)
        self.status, self.inliers = status, inliers


class Sim3SolverSet(_SolverSet):
    """USLAM::Sim3Solver for LoopClosing::ComputeSim3 (src/LoopClosing.cc:373-479): the solvers of all loop candidates in one set on an
    ORBmatcher handle, iterate() over a list of them as one device call -> Sim3SolverResult."""
    _prefix = _where = "uvo_sim3solver_"
    _info, _result_c, _result = Sim3SolverInfo, Sim3SolverResultC, Sim3SolverResult

    def __init__(self, matcher, max_solvers, max_points, _api=None):
        super().__init__(matcher, max_solvers, max_points, _api)

    def add(self, x1w, x2w, sigma2_1, sigma2_2, index1, n_matches, kf1, kf2, params=None):
        """Sim3Solver(pKF1, pKF2, vpMatched12) + SetRansacParameters -> solver id.  kf1, kf2: (Rcw, tcw, (fx, fy, cx, cy)) or
        Sim3KeyFrame; index1 defaults to 0..n-1, n_matches to n."""
        a = np.ascontiguousarray(x1w, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(x2w, np.float32).reshape(-1, 3)
        s1 = np.ascontiguousarray(sigma2_1, np.float32).reshape(-1)
        s2 = np.ascontiguousarray(sigma2_2, np.float32).reshape(-1)
        ix = np.arange(len(a), dtype=np.int32) if index1 is None else np.ascontiguousarray(index1, np.int32).reshape(-1)
        if not (len(a) == len(b) == len(s1) == len(s2) == len(ix)):
            raise ValueError("x1w, x2w, sigma2_1, sigma2_2 and index1 differ in length")
        nm = len(a) if n_matches is None else int(n_matches)
        k1 = kf1 if isinstance(kf1, Sim3KeyFrame) else Sim3KeyFrame.make(*kf1)
        k2 = kf2 if isinstance(kf2, Sim3KeyFrame) else Sim3KeyFrame.make(*kf2)
        prm = params if params is not None else Sim3SolverParams()
        return self._added(nm, _ptr(a), _ptr(b), _ptr(s1), _ptr(s2), _ptr(ix), len(a), nm, ctypes.byref(k1), ctypes.byref(k2), ctypes.byref(prm))

    def set_ransac_parameters(self, sid, params):
        self._do("set_ransac_parameters", sid, ctypes.byref(params))

    def find(self, sid, rng):
        """Sim3Solver::find: iterate(mRansacMaxIts)."""
        return self._call("find", [sid], None, int(sid), ctypes.byref(rng))

    def hypotheses(self, sid, cap=1024):
        """Test tap: (subsets int32[h, 3], T12 float32[h, 16], T21 float32[h, 16], counts int32[h]) of the last iterate call."""
        return self._tap(sid, cap, np.zeros((cap, 3), np.int32), np.zeros((cap, 16), np.float32), np.zeros((cap, 16), np.float32), np.zeros(cap, np.int32))


class Sim3OptProblemC(ctypes.Structure):
    """uvo_sim3_opt_problem."""
    _fields_ = [("x1w", ctypes.c_void_p), ("x2w", ctypes.c_void_p), ("obs1", ctypes.c_void_p), ("obs2", ctypes.c_void_p), ("info1", ctypes.c_void_p),
                ("info2", ctypes.c_void_p), ("n", ctypes.c_int32), ("th2", ctypes.c_float), ("kf1", Sim3KeyFrame), ("kf2", Sim3KeyFrame),
                ("R12", ctypes.c_float * 9), ("t12", ctypes.c_float * 3), ("s12", ctypes.c_float), ("pad_", ctypes.c_int32)]


class Sim3OptResultC(ctypes.Structure):
    """uvo_sim3_opt_result."""
    _fields_ = [("q", ctypes.c_double * 4), ("t", ctypes.c_double * 3), ("s", ctypes.c_double), ("R12", ctypes.c_float * 9), ("t12", ctypes.c_float * 3),
                ("scale", ctypes.c_float), ("n_inliers", ctypes.c_int32), ("n_correspondences", ctypes.c_int32), ("n_bad", ctypes.c_int32),
                ("more_iterations", ctypes.c_int32), ("removed_cap", ctypes.c_int32), ("removed", ctypes.c_void_p)]


class Sim3OptTraceLin(ctypes.Structure):
    """uvo_sim3_opt_trace_lin."""
    _fields_ = [("round", ctypes.c_int32), ("iteration", ctypes.c_int32), ("H", ctypes.c_double * 28), ("b", ctypes.c_double * 7), ("chi2", ctypes.c_double)]


class Sim3OptTraceC(ctypes.Structure):
    """uvo_sim3_opt_trace."""
    _fields_ = [("n_lin", ctypes.c_int32), ("n_trials", ctypes.c_int32), ("q", ctypes.c_double * 4), ("t", ctypes.c_double * 3), ("s", ctypes.c_double),
                ("lin", Sim3OptTraceLin * 15), ("trial", PoseTraceTrial * 150)]


SIM3OPT_LIN_DTYPE = np.dtype([("round", "<i4"), ("iteration", "<i4"), ("H", "<f8", 28), ("b", "<f8", 7), ("chi2", "<f8")])


class Sim3OptTrace:
    """The test tap of one problem: q float64[4] (x y z w), t float64[3], s, lin (SIM3OPT_LIN_DTYPE, one record per linearisation), trial
    (POSE_TRIAL_DTYPE, one per Levenberg trial)."""

    def __init__(self, c):
        self.q, self.t, self.s = np.array(c.q, np.float64), np.array(c.t, np.float64), float(c.s)
        self.lin = np.frombuffer(bytes(c.lin), SIM3OPT_LIN_DTYPE)[:c.n_lin].copy()
        self.trial = np.frombuffer(bytes(c.trial), POSE_TRIAL_DTYPE)[:c.n_trials].copy()


class Sim3OptResult:
    """One optimised candidate: q float64[4] (x y z w, not normalised), t float64[3], s; R12 float32[3, 3], t12 float32[3], scale;
    n_inliers (the reference's return value; 0 on the early return, the estimate is then the input's), n_correspondences, n_bad,
    more_iterations, removed uint8[n] (1 where the reference nulls vpMatches1[idx])."""

    def __init__(self, c, removed):
        self.q, self.t, self.s = np.array(c.q, np.float64), np.array(c.t, np.float64), float(c.s)
        self.R12, self.t12, self.scale = np.array(c.R12, np.float32).reshape(3, 3), np.array(c.t12, np.float32), np.float32(c.scale)
        self.n_inliers, self.n_correspondences, self.n_bad, self.more_iterations = c.n_inliers, c.n_correspondences, c.n_bad, c.more_iterations
        self.removed = removed


class Sim3Optimizer:
    """Optimizer::OptimizeSim3 (src/Optimizer.cc:2660-2856) on an ORBmatcher handle: optimize() takes the problems of all loop candidates
    and runs them as one device call; the caller takes the first in candidate order with n_inliers >= 10.  `_api` exists so that the
    tests can drive another build through this class."""

    def __init__(self, matcher, max_problems=1, max_pairs=4096, _api=None):
        self._api = _api if _api is not None else lib
        self._matcher = matcher   # the set launches in the handle's stream: keep it alive
        self._h = ctypes.c_void_p()
        self.max_problems, self.max_pairs = max_problems, max_pairs
        rc = self._api.uvo_sim3_optimizer_create(matcher._h if matcher is not None else None, max_problems, max_pairs, ctypes.byref(self._h))
        if rc:
            self._h = None
            raise UvoError(rc, "uvo_sim3_optimizer_create")

    def close(self):
        if getattr(self, "_h", None) and self._api is not None:
            self._api.uvo_sim3_optimizer_destroy(self._h)
            self._h = None

    __del__ = close

    def optimize(self, problems, removed_cap=None):
        """problems: a list of dicts x1w [n, 3], x2w [n, 3], obs1 [n, 2], obs2 [n, 2], info1 [n] (the reference: GetInvSigma2(octave1)),
        info2 [n] (the reference: GetSigma2(octave2)), kf1 and kf2 = (Rcw, tcw, K) or Sim3KeyFrame, R12 [3, 3], t12 [3], s12, th2
        -> a list of Sim3OptResult.  removed_cap (for the tests): the mask capacity passed for every problem instead of its n."""
        cp = (Sim3OptProblemC * max(len(problems), 1))()
        cr = (Sim3OptResultC * max(len(problems), 1))()
        keep, masks = [], []
        for j, p in enumerate(problems):
            arr = [np.ascontiguousarray(p[k], np.float32).reshape(-1, w) for k, w in (("x1w", 3), ("x2w", 3), ("obs1", 2), ("obs2", 2), ("info1", 1), ("info2", 1))]
            n = len(arr[0])
            if any(len(a) != n for a in arr):
                raise ValueError("the arrays of a problem differ in length")
            m = np.zeros(max(n, 1), np.uint8)
            keep.append(arr)
            masks.append(m)
            c = cp[j]
            c.x1w, c.x2w, c.obs1, c.obs2, c.info1, c.info2 = [a.ctypes.data for a in arr]
            c.n, c.th2 = n, float(np.float32(p["th2"]))
            c.kf1, c.kf2 = [k if isinstance(k, Sim3KeyFrame) else Sim3KeyFrame.make(*k) for k in (p["kf1"], p["kf2"])]
            c.R12 = (ctypes.c_float * 9)(*np.asarray(p["R12"], np.float32).reshape(9).tolist())
            c.t12 = (ctypes.c_float * 3)(*np.asarray(p["t12"], np.float32).reshape(3).tolist())
            c.s12 = float(np.float32(p["s12"]))
            cr[j].removed, cr[j].removed_cap = m.ctypes.data, n if removed_cap is None else removed_cap
        rc = self._api.uvo_sim3_optimize(self._h, cp, len(problems), cr)
        if rc:
            raise UvoError(rc, "uvo_sim3_optimize")
        return [Sim3OptResult(cr[j], masks[j][:cp[j].n].copy()) for j in range(len(problems))]

    def trace(self, problem=0):
        """Test tap: Sim3OptTrace of problem `problem` of the last optimize() call."""
        c = Sim3OptTraceC()
        rc = self._api.uvo_sim3_optimizer_trace(self._h, problem, ctypes.byref(c))
        if rc:
            raise UvoError(rc, "uvo_sim3_optimizer_trace")
        return Sim3OptTrace(c)


UVO_BA_LOCAL, UVO_BA_FULL = 0, 1


class BaProblemC(ctypes.Structure):
    """uvo_ba_problem."""
    _fields_ = [("mode", ctypes.c_int32), ("n_iterations", ctypes.c_int32), ("n_keyframes", ctypes.c_int32), ("n_points", ctypes.c_int32),
                ("n_edges", ctypes.c_int32), ("n_cameras", ctypes.c_int32), ("kf_Tcw", ctypes.c_void_p), ("kf_fixed", ctypes.c_void_p),
                ("points", ctypes.c_void_p), ("point_bad", ctypes.c_void_p), ("point_edge_begin", ctypes.c_void_p), ("edge_kf", ctypes.c_void_p),
                ("edge_obs", ctypes.c_void_p), ("edge_inv_sigma2", ctypes.c_void_p), ("edge_camera", ctypes.c_void_p), ("cameras", ctypes.c_void_p)]


class BaResultC(ctypes.Structure):
    """uvo_ba_result."""
    _fields_ = [("kf_estimate", ctypes.c_void_p), ("kf_Tcw", ctypes.c_void_p), ("point_estimate", ctypes.c_void_p), ("points", ctypes.c_void_p),
                ("removed1", ctypes.c_void_p), ("removed2", ctypes.c_void_p), ("n_removed1", ctypes.c_int32), ("n_removed2", ctypes.c_int32),
                ("iterations", ctypes.c_int32 * 2), ("n_trials", ctypes.c_int32), ("n_syncs", ctypes.c_int32)]


class BaTraceLin(ctypes.Structure):
    """uvo_ba_trace_lin."""
    _fields_ = [("round", ctypes.c_int32), ("iteration", ctypes.c_int32), ("n_edges", ctypes.c_int32), ("n_free", ctypes.c_int32),
                ("n_points", ctypes.c_int32), ("pad_", ctypes.c_int32), ("chi2", ctypes.c_double), ("maxdiag", ctypes.c_double)]


class BaTraceC(ctypes.Structure):
    """uvo_ba_trace."""
    _fields_ = [("n_lin", ctypes.c_int32), ("n_trials", ctypes.c_int32), ("lin", BaTraceLin * 32), ("trial", PoseTraceTrial * 320)]


BA_LIN_DTYPE = np.dtype([("round", "<i4"), ("iteration", "<i4"), ("n_edges", "<i4"), ("n_free", "<i4"), ("n_points", "<i4"), ("pad_", "<i4"),
                         ("chi2", "<f8"), ("maxdiag", "<f8")])


class BaTrace:
    """The test tap of a call: lin (BA_LIN_DTYPE, one record per linearisation), trial (POSE_TRIAL_DTYPE, one per Levenberg trial)."""

    def __init__(self, c):
        self.lin = np.frombuffer(bytes(c.lin), BA_LIN_DTYPE)[:c.n_lin].copy()
        self.trial = np.frombuffer(bytes(c.trial), POSE_TRIAL_DTYPE)[:c.n_trials].copy()


class BaResult:
    """One adjusted problem: kf_estimate float64[K, 7] (quaternion x y z w, t), kf_Tcw float32[K, 4, 4], point_estimate float64[P, 3],
    points float32[P, 3], removed1 / removed2 uint8[E] (the observations the two checks erase), their counts, iterations (linearisations
    per optimize()), n_trials, n_syncs."""

    def __init__(self, c, arrays):
        self.kf_estimate, self.kf_Tcw, self.point_estimate, self.points, self.removed1, self.removed2 = arrays
        self.n_removed1, self.n_removed2, self.iterations = c.n_removed1, c.n_removed2, (c.iterations[0], c.iterations[1])
        self.n_trials, self.n_syncs = c.n_trials, c.n_syncs


def _ba_graph(scene, c, K, also=()):
    """The lists uvo_ba_problem and uvo_nav_ba_problem name alike (fixed, points, point_bad, begin, the four edge lists, cameras):
    converted, their lengths checked against K key frames (`also`: further arrays of K entries) and each other, set in c with the counts
    -> what to keep alive."""
    f32, i32, u8 = np.float32, np.int32, np.uint8
    fixed = np.ascontiguousarray(scene["fixed"], u8).reshape(-1)
    pts = np.ascontiguousarray(scene["points"], f32).reshape(-1, 3)
    bad = None if scene.get("point_bad") is None else np.ascontiguousarray(scene["point_bad"], u8).reshape(-1)
    begin = np.ascontiguousarray(scene["begin"], i32).reshape(-1)
    ekf = np.ascontiguousarray(scene["edge_kf"], i32).reshape(-1)
    obs = np.ascontiguousarray(scene["edge_obs"], f32).reshape(-1, 2)
    w = np.ascontiguousarray(scene["edge_inv_sigma2"], f32).reshape(-1)
    ecam = np.ascontiguousarray(scene["edge_camera"], i32).reshape(-1)
    cams = np.ascontiguousarray(scene["cameras"], f32).reshape(-1, 4)
    P, E = len(pts), len(ekf)
    if any(len(a) != K for a in (fixed,) + tuple(also)) or len(begin) != P + 1 or len(obs) != E or len(w) != E or len(ecam) != E or (bad is not None and len(bad) != P):
        raise ValueError("the arrays of the problem differ in length")
    c.n_keyframes, c.n_points, c.n_edges, c.n_cameras = K, P, E, len(cams)
    c.kf_fixed, c.points, c.point_bad = fixed.ctypes.data, pts.ctypes.data, None if bad is None else bad.ctypes.data
    c.point_edge_begin, c.edge_kf, c.edge_obs, c.edge_inv_sigma2 = begin.ctypes.data, ekf.ctypes.data, obs.ctypes.data, w.ctypes.data
    c.edge_camera, c.cameras = ecam.ctypes.data, cams.ctypes.data
    return fixed, pts, bad, begin, ekf, obs, w, ecam, cams


def _ba_outputs(c, r, kf_words, names):
    """The six arrays of a result of problem c, the key frames' estimates kf_words wide, set in r under `names` -> (the arrays cut to
    the problem's counts, what to keep alive)."""
    K, P, E = c.n_keyframes, c.n_points, c.n_edges
    out = [np.zeros((max(K, 1), kf_words)), np.zeros((max(K, 1), 4, 4), np.float32), np.zeros((max(P, 1), 3)), np.zeros((max(P, 1), 3), np.float32),
           np.zeros(max(E, 1), np.uint8), np.zeros(max(E, 1), np.uint8)]
    for name, a in zip(names, out):
        setattr(r, name, a.ctypes.data)
    return [out[0][:K], out[1][:K], out[2][:P], out[3][:P], out[4][:E], out[5][:E]], out


def ba_marshal(scene, mode=UVO_BA_LOCAL, n_iterations=0):
    """A scene dict (Tcw [K, 12] or [K, 3, 4], fixed [K], points [P, 3], point_bad [P] or absent, begin [P + 1], edge_kf [E],
    edge_obs [E, 2], edge_inv_sigma2 [E], edge_camera [E], cameras [C, 4]) -> (BaProblemC, BaResultC, the result's arrays, what to keep alive)."""
    T = np.ascontiguousarray(scene["Tcw"], np.float32).reshape(-1, 12)
    c = BaProblemC()
    graph = _ba_graph(scene, c, len(T))
    c.mode, c.n_iterations, c.kf_Tcw = mode, n_iterations, T.ctypes.data
    r = BaResultC()
    arrays, out = _ba_outputs(c, r, 7, ("kf_estimate", "kf_Tcw", "point_estimate", "points", "removed1", "removed2"))
    return c, r, arrays, (T, graph, out)


class _Adjuster:
    """What BundleAdjuster and NavBundleAdjuster share: a handle made by `<_handle>_create` on an ORBmatcher handle, run by `_call`, read
    by `<_handle>_trace`, freed by `<_handle>_destroy`."""

    def __init__(self, matcher, sizes, _api):
        self._api = _api if _api is not None else lib
        self._matcher = matcher   # the adjuster launches in the handle's stream: keep it alive
        self._h = ctypes.c_void_p()
        rc = getattr(self._api, self._handle + "_create")(matcher._h if matcher is not None else None, *sizes, ctypes.byref(self._h))
        if rc:
            self._h = None
            raise UvoError(rc, self._handle + "_create")

    def close(self):
        if getattr(self, "_h", None) and self._api is not None:
            getattr(self._api, self._handle + "_destroy")(self._h)
            self._h = None

    __del__ = close

    def _adjust(self, c, r):
        rc = getattr(self._api, self._call)(self._h, ctypes.byref(c), ctypes.byref(r))
        if rc:
            raise UvoError(rc, self._call)

    def _trace(self, c):
        rc = getattr(self._api, self._handle + "_trace")(self._h, ctypes.byref(c))
        if rc:
            raise UvoError(rc, self._handle + "_trace")
        return c


class BundleAdjuster(_Adjuster):
    """Optimizer::LocalBundleAdjustment (src/Optimizer.cc:2147-2405) and Optimizer::BundleAdjustment (:1896-2010) on an ORBmatcher
    handle, the mapping thread's stream: adjust() runs one problem, every phase a launch of its own and the Levenberg decision on the
    device.  `_api` exists so that the tests can drive another build through this class."""
    _handle, _call = "uvo_bundle_adjuster", "uvo_bundle_adjust"

    def __init__(self, matcher, max_free=32, max_fixed=64, max_points=8192, max_edges=65536, _api=None):
        super().__init__(matcher, (max_free, max_fixed, max_points, max_edges), _api)

    def adjust(self, scene, mode=UVO_BA_LOCAL, n_iterations=0):
        """scene: the dict ba_marshal() describes -> BaResult."""
        c, r, arrays, keep = ba_marshal(scene, mode, n_iterations)
        self._adjust(c, r)
        return BaResult(r, arrays)

    def trace(self):
        """Test tap: BaTrace of the last adjust() call."""
        return BaTrace(self._trace(BaTraceC()))


NAV_STATE_WORDS = 22      # uvo_nav_state: P V q (x y z w) bg ba dbg dba
NAVBA_LINK_DTYPE = np.dtype([("kf0", "<i4"), ("kf1", "<i4"), ("dT", "<f8"), ("dP", "<f8", 3), ("dV", "<f8", 3), ("dR", "<f8", 9), ("JPg", "<f8", 9),
                             ("JPa", "<f8", 9), ("JVg", "<f8", 9), ("JVa", "<f8", 9), ("JRg", "<f8", 9), ("cov", "<f8", 81)])
NAVBA_DEPTH_DTYPE = np.dtype([("ka", "<i4"), ("kb", "<i4"), ("kc", "<i4"), ("link", "<i4"), ("shi", "<f8"), ("meas", "<f8"), ("info", "<f8")])


class NavBaProblemC(ctypes.Structure):
    """uvo_nav_ba_problem."""
    _fields_ = [("n_keyframes", ctypes.c_int32), ("n_points", ctypes.c_int32), ("n_edges", ctypes.c_int32), ("n_cameras", ctypes.c_int32),
                ("n_links", ctypes.c_int32), ("n_depth", ctypes.c_int32), ("kf_state", ctypes.c_void_p), ("kf_fixed", ctypes.c_void_p),
                ("kf_has_bias", ctypes.c_void_p), ("points", ctypes.c_void_p), ("point_bad", ctypes.c_void_p), ("point_edge_begin", ctypes.c_void_p),
                ("edge_kf", ctypes.c_void_p), ("edge_obs", ctypes.c_void_p), ("edge_inv_sigma2", ctypes.c_void_p), ("edge_camera", ctypes.c_void_p),
                ("cameras", ctypes.c_void_p), ("Rbc", ctypes.c_double * 9), ("Pbc", ctypes.c_double * 3), ("gw", ctypes.c_double * 3),
                ("gyr_bias_rw2", ctypes.c_double), ("acc_bias_rw2", ctypes.c_double), ("links", ctypes.c_void_p), ("depth", ctypes.c_void_p)]


class NavBaResultC(ctypes.Structure):
    """uvo_nav_ba_result."""
    _fields_ = [("kf_state", ctypes.c_void_p), ("kf_Tcw", ctypes.c_void_p), ("point_estimate", ctypes.c_void_p), ("points", ctypes.c_void_p),
                ("excluded", ctypes.c_void_p), ("erased", ctypes.c_void_p), ("n_excluded", ctypes.c_int32), ("n_erased", ctypes.c_int32),
                ("iterations", ctypes.c_int32 * 2), ("n_trials", ctypes.c_int32), ("n_syncs", ctypes.c_int32)]


class NavBaTraceC(ctypes.Structure):
    """uvo_nav_ba_trace."""
    _fields_ = [("n_lin", ctypes.c_int32), ("n_trials", ctypes.c_int32), ("lin", BaTraceLin * 32), ("trial", PoseTraceTrial * 320)]


class NavBaTrace(BaTrace):
    """The test tap of a call: lin (BA_LIN_DTYPE; n_edges counts the inertial edges too), trial (POSE_TRIAL_DTYPE)."""


class NavBaResult:
    """One adjusted window: kf_state float64[K, 22] (P V q bg ba dbg dba), kf_Tcw float32[K, 4, 4], point_estimate float64[P, 3], points
    float32[P, 3], excluded uint8[E] (the first check's level 1) and erased uint8[E] (the final check), their counts, iterations, n_trials,
    n_syncs."""

    def __init__(self, c, arrays):
        self.kf_state, self.kf_Tcw, self.point_estimate, self.points, self.excluded, self.erased = arrays
        self.n_excluded, self.n_erased, self.iterations = c.n_excluded, c.n_erased, (c.iterations[0], c.iterations[1])
        self.n_trials, self.n_syncs = c.n_trials, c.n_syncs


def navba_marshal(scene):
    """A scene dict (states [K, 22], fixed [K], has_bias [K], points [P, 3], point_bad [P] or absent, begin [P + 1], edge_kf [E], edge_obs
    [E, 2], edge_inv_sigma2 [E], edge_camera [E], cameras [C, 4], Rbc [9], Pbc [3], gw [3], gyr_rw2, acc_rw2, links (NAVBA_LINK_DTYPE [L]),
    depth (NAVBA_DEPTH_DTYPE [D])) -> (NavBaProblemC, NavBaResultC, the result's arrays, what to keep alive)."""
    f64 = np.float64
    st = np.ascontiguousarray(scene["states"], f64).reshape(-1, NAV_STATE_WORDS)
    hb = np.ascontiguousarray(scene["has_bias"], np.uint8).reshape(-1)
    links = np.ascontiguousarray(scene["links"], NAVBA_LINK_DTYPE).reshape(-1)
    depth = np.ascontiguousarray(scene["depth"], NAVBA_DEPTH_DTYPE).reshape(-1)
    c = NavBaProblemC()
    graph = _ba_graph(scene, c, len(st), also=(hb,))
    c.n_links, c.n_depth = len(links), len(depth)
    c.kf_state, c.kf_has_bias, c.links, c.depth = st.ctypes.data, hb.ctypes.data, links.ctypes.data, depth.ctypes.data
    c.Rbc[:] = [float(v) for v in np.asarray(scene["Rbc"], f64).reshape(9)]
    c.Pbc[:] = [float(v) for v in np.asarray(scene["Pbc"], f64).reshape(3)]
    c.gw[:] = [float(v) for v in np.asarray(scene["gw"], f64).reshape(3)]
    c.gyr_bias_rw2, c.acc_bias_rw2 = float(scene["gyr_rw2"]), float(scene["acc_rw2"])
    r = NavBaResultC()
    arrays, out = _ba_outputs(c, r, NAV_STATE_WORDS, ("kf_state", "kf_Tcw", "point_estimate", "points", "excluded", "erased"))
    return c, r, arrays, (st, hb, links, depth, graph, out)


class NavBundleAdjuster(_Adjuster):
    """Optimizer::LocalBundleAdjustmentNavState (src/Optimizer.cc:1105-1732) on an ORBmatcher handle, the mapping thread's stream:
    adjust() runs one window, every phase a launch of its own and the Levenberg decision on the device.  `_api` exists so that the tests
    can drive another build through this class."""
    _handle, _call = "uvo_nav_bundle_adjuster", "uvo_nav_bundle_adjust"

    def __init__(self, matcher, max_free=24, max_fixed=64, max_points=8192, max_edges=65536, max_depth=64, _api=None):
        super().__init__(matcher, (max_free, max_fixed, max_points, max_edges, max_depth), _api)

    def adjust(self, scene):
        """scene: the dict navba_marshal() describes -> NavBaResult."""
        c, r, arrays, keep = navba_marshal(scene)
        self._adjust(c, r)
        return NavBaResult(r, arrays)

    def trace(self):
        """Test tap: NavBaTrace of the last adjust() call."""
        return NavBaTrace(self._trace(NavBaTraceC()))


class EssentialProblemC(ctypes.Structure):
    """uvo_essential_problem."""
    _fields_ = [("n_keyframes", ctypes.c_int32), ("n_edges", ctypes.c_int32), ("n_points", ctypes.c_int32), ("fixed", ctypes.c_int32),
                ("Scw", ctypes.c_void_p), ("Scw_normal", ctypes.c_void_p), ("edge_i", ctypes.c_void_p), ("edge_j", ctypes.c_void_p),
                ("edge_connection", ctypes.c_void_p), ("points", ctypes.c_void_p), ("point_ref", ctypes.c_void_p), ("n_iterations", ctypes.c_int32)]


class EssentialResultC(ctypes.Structure):
    """uvo_essential_result."""
    _fields_ = [("Scw", ctypes.c_void_p), ("kf_Tcw", ctypes.c_void_p), ("points", ctypes.c_void_p), ("iterations", ctypes.c_int32),
                ("n_trials", ctypes.c_int32), ("n_syncs", ctypes.c_int32), ("envelope_blocks", ctypes.c_int32)]


class EssentialResult:
    """One optimised graph: Scw float64[K, 8] (quaternion x y z w not normalised, t, s), kf_Tcw float32[K, 4, 4] = [R | t / s], points
    float32[P, 3], iterations (linearisations), n_trials, n_syncs, envelope_blocks."""

    def __init__(self, c, arrays):
        self.Scw, self.kf_Tcw, self.points = arrays
        self.iterations, self.n_trials, self.n_syncs, self.envelope_blocks = c.iterations, c.n_trials, c.n_syncs, c.envelope_blocks


def essential_marshal(scene, n_iterations=None):
    """A scene dict (Scw [K, 8], Scwn [K, 8] or absent: Scw, edge_i [E], edge_j [E], conn [E], points [P, 3], ref [P], fixed, n_iterations)
    -> (EssentialProblemC, EssentialResultC, the result's arrays, what to keep alive)."""
    f64, i32 = np.float64, np.int32
    S = np.ascontiguousarray(scene["Scw"], f64).reshape(-1, 8)
    Sn = np.ascontiguousarray(scene["Scwn"] if scene.get("Scwn") is not None else S, f64).reshape(-1, 8)
    ei, ej = np.ascontiguousarray(scene["edge_i"], i32).reshape(-1), np.ascontiguousarray(scene["edge_j"], i32).reshape(-1)
    conn = np.ascontiguousarray(scene["conn"], np.uint8).reshape(-1)
    pts, ref = np.ascontiguousarray(scene["points"], np.float32).reshape(-1, 3), np.ascontiguousarray(scene["ref"], i32).reshape(-1)
    K, E, P = len(S), len(ei), len(pts)
    if len(Sn) != K or len(ej) != E or len(conn) != E or len(ref) != P:
        raise ValueError("the arrays of the problem differ in length")
    c = EssentialProblemC()
    c.n_keyframes, c.n_edges, c.n_points, c.fixed = K, E, P, int(scene["fixed"])
    c.Scw, c.Scw_normal, c.edge_i, c.edge_j, c.edge_connection = S.ctypes.data, Sn.ctypes.data, ei.ctypes.data, ej.ctypes.data, conn.ctypes.data
    c.points, c.point_ref = pts.ctypes.data, ref.ctypes.data
    c.n_iterations = int(scene.get("n_iterations", 20) if n_iterations is None else n_iterations)
    out = [np.zeros((max(K, 1), 8)), np.zeros((max(K, 1), 4, 4), np.float32), np.zeros((max(P, 1), 3), np.float32)]
    r = EssentialResultC()
    r.Scw, r.kf_Tcw, r.points = out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data
    return c, r, [out[0][:K], out[1][:K], out[2][:P]], (S, Sn, ei, ej, conn, pts, ref, out)


class EssentialGraph(_Adjuster):
    """Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2409-2658) for a gathered graph on an ORBmatcher handle, the loop-closing
    thread's stream: optimize() runs one graph, every phase a launch of its own, the Levenberg decision on the device, the system by a
    block-envelope LDL^T in key-frame order.  `_api` exists so that the tests can drive another build through this class."""
    _handle, _call = "uvo_essential_graph", "uvo_essential_graph_optimize"

    def __init__(self, matcher, max_keyframes=2048, max_edges=16384, max_envelope_blocks=1 << 18, max_points=1 << 17, _api=None):
        super().__init__(matcher, (max_keyframes, max_edges, max_envelope_blocks, max_points), _api)

    def optimize(self, scene, n_iterations=None):
        """scene: the dict essential_marshal() describes -> EssentialResult."""
        c, r, arrays, keep = essential_marshal(scene, n_iterations)
        self._adjust(c, r)
        return EssentialResult(r, arrays)

    def trace(self):
        """Test tap: BaTrace of the last optimize() call (lin: chi2 per linearisation; trial: lambda, cur, tmp, scale, ok, accepted)."""
        return BaTrace(self._trace(BaTraceC()))


class InitializerResultC(ctypes.Structure):
    """uvo_initializer_result."""
    _fields_ = [("initialized", ctypes.c_int32), ("best", ctypes.c_int32), ("n_inliers", ctypes.c_int32), ("draws", ctypes.c_uint32),
                ("deciding", ctypes.c_int32), ("n_good", ctypes.c_int32 * 4), ("parallax", ctypes.c_float * 4), ("score", ctypes.c_float),
                ("R21", ctypes.c_float * 9), ("t21", ctypes.c_float * 3), ("F21", ctypes.c_float * 9), ("pad_", ctypes.c_int32),
                ("inliers", ctypes.c_void_p), ("p3d", ctypes.c_void_p), ("triangulated", ctypes.c_void_p)]


class InitializerResult:
    """One Initialize call: initialized (its return value), best (the hypothesis kept, -1: none), n_inliers, draws, deciding (0..3, -1),
    n_good int32[4], parallax float32[4], score (SF), R21 float32[3, 3], t21 float32[3], F21 float32[3, 3], inliers uint8[n2],
    p3d float32[n2, 3] and triangulated uint8[n2], both indexed by the current frame's key."""

    def __init__(self, c, inliers, p3d, triangulated):
        self.initialized, self.best, self.n_inliers, self.draws, self.deciding = bool(c.initialized), c.best, c.n_inliers, c.draws, c.deciding
        self.n_good, self.parallax, self.score = np.array(c.n_good, np.int32), np.array(c.parallax, np.float32), np.float32(c.score)
        self.R21, self.t21 = np.array(c.R21, np.float32).reshape(3, 3), np.array(c.t21, np.float32)
        self.F21 = np.array(c.F21, np.float32).reshape(3, 3)
        self.inliers, self.p3d, self.triangulated = inliers, p3d, triangulated


class Initializer:
    """USLAM::Initializer for Tracking::Initialize (src/Tracking.cc:1340, :1582): the F path of Initialize as one device call on a KLT
    handle.  `_api` / `_prefix` exist so that the tests' host build of the same source can be driven through this very class."""
    _prefix = "uvo_initializer_"

    def __init__(self, klt, max_keys, _api=None):
        self._api = _api if _api is not None else lib
        self._klt = klt   # the object launches in the handle's stream: keep it alive
        self._h = ctypes.c_void_p()
        rc = self._f("create")(klt._h if klt is not None else None, max_keys, ctypes.byref(self._h))
        if rc:
            raise UvoError(rc, "uvo_initializer_create")

    def _f(self, name):
        return getattr(self._api, self._prefix + name)

    def close(self):
        if getattr(self, "_h", None) and self._api is not None:
            self._f("destroy")(self._h)
            self._h = None

    __del__ = close

    def set_reference(self, keys1, cam, sigma=1.0, iterations=200):
        """Initializer(ReferenceFrame, sigma, iterations): keys1 float32[n1, 2] = mvKeysUn, cam a CameraModel or (fx, fy, cx, cy)."""
        k1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
        c = cam if isinstance(cam, CameraModel) else CameraModel.make(*cam, [])
        rc = self._f("set_reference")(self._h, _ptr(k1), len(k1), ctypes.addressof(c), float(sigma), int(iterations))
        if rc:
            raise UvoError(rc, "uvo_initializer_set_reference")

    def initialize(self, keys2, matches12, rng):
        """Initialize(CurrentFrame, vMatches12, ...): keys2 float32[n2, 2], matches12 int32[n2]; rng (GlibcRand) is advanced in place."""
        k2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
        m = np.ascontiguousarray(matches12, np.int32).reshape(-1)
        if len(m) != len(k2):
            raise ValueError("keys2 and matches12 differ in length")
        n = len(k2)
        inl, p3d, tri = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.uint8)
        res = InitializerResultC()
        res.inliers, res.p3d, res.triangulated = inl.ctypes.data, p3d.ctypes.data, tri.ctypes.data
        rc = self._f("initialize")(self._h, _ptr(k2), n, _ptr(m), ctypes.addressof(rng), ctypes.byref(res))
        if rc:
            raise UvoError(rc, "uvo_initializer_initialize")
        return InitializerResult(res, inl[:n], p3d[:n], tri[:n])

    def hypotheses(self, cap=1024):
        """Test tap: (sets int32[h, 8], F21i float32[h, 9], scores float32[h]) of the last initialize call."""
        sub, F, sc, n = np.zeros((cap, 8), np.int32), np.zeros((cap, 9), np.float32), np.zeros(cap, np.float32), ctypes.c_int()
        rc = self._f("hypotheses")(self._h, _ptr(sub), _ptr(F), _ptr(sc), cap, ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_initializer_hypotheses")
        return sub[:n.value].copy(), F[:n.value].copy(), sc[:n.value].copy()


KFDB_STATE_DTYPE = np.dtype([("loop_query", np.int64), ("reloc_query", np.int64), ("loop_words", np.int32), ("reloc_words", np.int32),
                             ("loop_score", np.float32), ("reloc_score", np.float32)])                      # uvo_kfdb_state
KFDB_ROW_DTYPE = np.dtype([("slot", np.int32), ("words", np.int32), ("flags", np.int32), ("best", np.int32), ("score", np.float32),
                           ("acc", np.float32)])                                                             # uvo_kfdb_query_row
KFDB_LISTED, KFDB_SCORED, KFDB_ENTERED, KFDB_RETAINED = 1, 2, 4, 8


class KeyFrameDatabase:
    """USLAM::KeyFrameDatabase (src/KeyFrameDatabase.cc) held on the device: add / erase / clear and the three Detect* queries, one call
    each.  Keyframes are named by the slot add() returns; BoW vectors are (ids uint32 ascending, values float64) as ORBVocabulary.transform
    returns them.  `_api` / `_prefix` exist so that the tests' host build of the same rules can be driven through this very class."""
    _prefix = "uvo_kfdb_"

    def __init__(self, max_keyframes, max_words, hash_len, device=0, _api=None):
        self._api = _api if _api is not None else lib
        self.max_keyframes, self.max_words, self.hash_len = int(max_keyframes), int(max_words), int(hash_len)
        self._h = ctypes.c_void_p()
        rc = self._f("create")(self.max_keyframes, self.max_words, self.hash_len, int(device), ctypes.byref(self._h))
        if rc:
            raise UvoError(rc, "uvo_kfdb_create")

    def _f(self, name):
        return getattr(self._api, self._prefix + name)

    def close(self):
        if getattr(self, "_h", None) and self._api is not None:
            self._f("destroy")(self._h)
            self._h = None

    __del__ = close

    def __len__(self):
        return self._f("size")(self._h)

    @staticmethod
    def _bow(bow):
        ids, vals = np.ascontiguousarray(bow[0], np.uint32).reshape(-1), np.ascontiguousarray(bow[1], np.float64).reshape(-1)
        if len(ids) != len(vals):
            raise ValueError("BoW ids and values differ in length")
        return ids, vals

    def _hash(self, h):
        if h is None:
            return None
        h = np.ascontiguousarray(h, np.float32).reshape(-1)
        if len(h) != self.hash_len:
            raise ValueError("hash of %d floats, the database holds %d" % (len(h), self.hash_len))
        return h

    def add(self, mn_id, bow, hash=None):
        """KeyFrameDatabase::add: returns the keyframe's slot."""
        ids, vals = self._bow(bow)
        h, slot = self._hash(hash), ctypes.c_int()
        rc = self._f("add")(self._h, int(mn_id), _ptr(ids), _ptr(vals), len(ids), _ptr(h), ctypes.byref(slot))
        if rc:
            raise UvoError(rc, "uvo_kfdb_add")
        return slot.value

    def erase(self, slot):
        rc = self._f("erase")(self._h, int(slot))
        if rc:
            raise UvoError(rc, "uvo_kfdb_erase")

    def clear(self):
        rc = self._f("clear")(self._h)
        if rc:
            raise UvoError(rc, "uvo_kfdb_clear")

    def set_covisibles(self, slot, neigh_slots):
        """GetBestCovisibilityKeyFrames(10) of the keyframe in `slot`, as slots in its order (-1: a neighbour without one)."""
        nb = np.ascontiguousarray(neigh_slots, np.int32).reshape(-1)
        rc = self._f("set_covisibles")(self._h, int(slot), _ptr(nb), len(nb))
        if rc:
            raise UvoError(rc, "uvo_kfdb_set_covisibles")

    def detect_reloc(self, query_id, bow):
        """DetectRelocalisationCandidates: the candidates' slots, in the reference's order."""
        ids, vals = self._bow(bow)
        cand, n = np.zeros(max(self.max_keyframes, 1), np.int32), ctypes.c_int()
        rc = self._f("detect_reloc")(self._h, int(query_id), _ptr(ids), _ptr(vals), len(ids), _ptr(cand), len(cand), ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_kfdb_detect_reloc")
        return cand[:n.value].copy()

    def detect_loop(self, query_id, bow, connected_slots, min_score):
        """DetectLoopCandidates(pKF, minScore); connected_slots: the slots of pKF->GetConnectedKeyFrames()."""
        ids, vals = self._bow(bow)
        conn = np.ascontiguousarray(connected_slots, np.int32).reshape(-1)
        cand, n = np.zeros(max(self.max_keyframes, 1), np.int32), ctypes.c_int()
        rc = self._f("detect_loop")(self._h, int(query_id), _ptr(ids), _ptr(vals), len(ids), _ptr(conn), len(conn), float(min_score), _ptr(cand), len(cand),
                                    ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_kfdb_detect_loop")
        return cand[:n.value].copy()

    def detect_loop_haloc(self, query_id, hash, exclude_ids, max_score):
        """DetectLoopCandidatesHaloc: three slots, or none when fewer than three matches were kept."""
        h, ex = self._hash(hash), np.ascontiguousarray(exclude_ids, np.int64).reshape(-1)
        cand, n = np.zeros(3, np.int32), ctypes.c_int()
        rc = self._f("detect_loop_haloc")(self._h, int(query_id), _ptr(h), _ptr(ex), len(ex), float(max_score), _ptr(cand), ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_kfdb_detect_loop_haloc")
        return cand[:n.value].copy()

    def last_query(self):
        """Test tap: (rows KFDB_ROW_DTYPE[n] in list order, maxCommonWords, minCommonWords) of the last BoW query."""
        rows, n, mx, mn = np.zeros(max(self.max_keyframes, 1), KFDB_ROW_DTYPE), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = self._f("last_query")(self._h, _ptr(rows), len(rows), ctypes.byref(n), ctypes.byref(mx), ctypes.byref(mn))
        if rc:
            raise UvoError(rc, "uvo_kfdb_last_query")
        return rows[:n.value].copy(), mx.value, mn.value

    def last_haloc(self):
        """Test tap: (m float32[slots], kept uint8[slots]) of the last haloc query."""
        m, kept, n = np.zeros(max(self.max_keyframes, 1), np.float32), np.zeros(max(self.max_keyframes, 1), np.uint8), ctypes.c_int()
        rc = self._f("last_haloc")(self._h, _ptr(m), _ptr(kept), len(m), ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_kfdb_last_haloc")
        return m[:n.value].copy(), kept[:n.value].copy()

    def state(self):
        """The six persistent fields of every slot, KFDB_STATE_DTYPE[len(self)]."""
        n = len(self)
        out = np.zeros(max(n, 1), KFDB_STATE_DTYPE)
        rc = self._f("state")(self._h, 0, n, _ptr(out))
        if rc:
            raise UvoError(rc, "uvo_kfdb_state")
        return out[:n].copy()


class KltCfg(ctypes.Structure):
    """uvo_klt_cfg."""
    _fields_ = [("max_width", ctypes.c_int32), ("max_height", ctypes.c_int32), ("max_level", ctypes.c_int32), ("win_width", ctypes.c_int32),
                ("win_height", ctypes.c_int32), ("max_points", ctypes.c_int32), ("slots", ctypes.c_int32), ("device", ctypes.c_int32)]


class KLT:
    """cv::buildOpticalFlowPyramid (src/FrameKTL.cc:76) + cv::calcOpticalFlowPyrLK as called at src/Tracking.cc:1046-1047
    (USE_INITIAL_FLOW + LK_GET_MIN_EIGENVALS, 30 iterations / eps 0.01)."""

    def __init__(self, max_width, max_height, win=(21, 21), max_level=5, max_points=4096, slots=2, device=0):
        cfg = KltCfg(max_width, max_height, max_level, win[0], win[1], max_points, slots, device)
        self._h = ctypes.c_void_p()
        self.max_level = max_level
        rc = lib.uvo_klt_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc:
            raise UvoError(rc, "uvo_klt_create")

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.uvo_klt_destroy(self._h)
            self._h = None

    __del__ = close

    def build_pyramid(self, slot, img):
        img = np.ascontiguousarray(img, np.uint8)
        n = ctypes.c_int()
        rc = lib.uvo_klt_build_pyramid(self._h, slot, _ptr(img), img.shape[1], img.shape[0], img.strides[0], ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_klt_build_pyramid")
        return n.value

    def build_pyramid_from(self, slot, extractor):
        """Pyramid of the extractor's last clahe() result, taken from HBM (no upload)."""
        n = ctypes.c_int()
        rc = lib.uvo_klt_build_pyramid_from_extractor(self._h, slot, extractor._h, ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_klt_build_pyramid_from_extractor")
        return n.value

    def read_level(self, slot, level):
        w, h = ctypes.c_int(), ctypes.c_int()
        rc = lib.uvo_klt_read_level(self._h, slot, level, None, None, ctypes.byref(w), ctypes.byref(h))
        if rc:
            raise UvoError(rc, "uvo_klt_read_level")
        img, der = np.zeros((h.value, w.value), np.uint8), np.zeros((h.value, w.value, 2), np.int16)
        rc = lib.uvo_klt_read_level(self._h, slot, level, _ptr(img), _ptr(der), ctypes.byref(w), ctypes.byref(h))
        if rc:
            raise UvoError(rc, "uvo_klt_read_level")
        return img, der

    def track(self, prev_slot, next_slot, prev_pts, next_pts0=None, max_count=30, epsilon=0.01, min_eig_threshold=1e-4, max_level=None):
        """Returns (next_pts, status, err).  max_level: the top pyramid level tracked (None: the handle's; clamped to the levels built)."""
        p0 = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
        p1 = p0.copy() if next_pts0 is None else np.ascontiguousarray(next_pts0, np.float32).reshape(-1, 2).copy()
        st, er = np.zeros(len(p0), np.uint8), np.zeros(len(p0), np.float32)
        rc = lib.uvo_klt_track(self._h, prev_slot, next_slot, _ptr(p0), _ptr(p1), len(p0), self._level(max_level), int(max_count), float(epsilon),
                               float(min_eig_threshold), _ptr(st), _ptr(er))
        if rc:
            raise UvoError(rc, "uvo_klt_track")
        return p1, st, er

    def _level(self, max_level):
        return self.max_level if max_level is None else int(max_level)

    def undistort(self, cam, pts):
        """Tracking::undistort_point (src/Tracking.cc:1265-1283) for an (n, 2) float32 array; cam: CameraModel."""
        p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        out = np.zeros_like(p)
        rc = lib.uvo_undistort_points(self._h, ctypes.byref(cam), _ptr(p), len(p), _ptr(out))
        if rc:
            raise UvoError(rc, "uvo_undistort_points")
        return out

    def track_undistorted(self, prev_slot, next_slot, prev_pts, cam, next_pts0=None, max_count=30, epsilon=0.01, min_eig_threshold=1e-4, max_level=None):
        """uvo_klt_track_undistorted: the LK step + undistort_point of both point sets in one call; max_level as in track().
        Returns (next, status, err, prev_un, next_un)."""
        a = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
        b = a.copy() if next_pts0 is None else np.ascontiguousarray(next_pts0, np.float32).reshape(-1, 2).copy()
        n = len(a)
        st, er = np.zeros(n, np.uint8), np.zeros(n, np.float32)
        pu, nu = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        rc = lib.uvo_klt_track_undistorted(self._h, prev_slot, next_slot, _ptr(a), _ptr(b), n, self._level(max_level), int(max_count), float(epsilon), float(min_eig_threshold),
                                           ctypes.byref(cam), _ptr(st), _ptr(er), _ptr(pu), _ptr(nu))
        if rc:
            raise UvoError(rc, "uvo_klt_track_undistorted")
        return b, st, er, pu, nu

    def find_fundamental(self, p0, p1, thr=1.0, conf=0.999):
        """uvo_klt_find_fundamental: cv::findFundamentalMat(p0, p1, FM_RANSAC, thr, conf, mask) (src/Tracking.cc:1062) on the device.
        Returns (mask uint8[n], F float64[3, 3] (zeros: no model), FmInfo)."""
        a = np.ascontiguousarray(p0, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
        if len(a) != len(b):
            raise ValueError("p0 and p1 differ in length")
        mask, F, info = np.zeros(len(a), np.uint8), np.zeros(9), FmInfo()
        rc = lib.uvo_klt_find_fundamental(self._h, _ptr(a), _ptr(b), len(a), float(thr), float(conf), _ptr(mask), _ptr(F), ctypes.byref(info))
        if rc:
            raise UvoError(rc, "uvo_klt_find_fundamental")
        return mask, F.reshape(3, 3), info

    def track_filtered(self, prev_slot, next_slot, prev_pts, cam, next_pts0=None, thr=1.0, conf=0.999, want_F=True, max_count=30, epsilon=0.01,
                       min_eig_threshold=1e-4, max_level=None):
        """uvo_klt_track_filtered: Tracking::perform_matching from :1037 on (tracker, undistortion, findFundamentalMat, mask_out = status &&
        inlier) in one call.  Returns (next, status, err, prev_un, next_un, mask_out, F or None); below 10 points only mask_out (all 0)
        and F (zeros) are written."""
        a = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
        b = a.copy() if next_pts0 is None else np.ascontiguousarray(next_pts0, np.float32).reshape(-1, 2).copy()
        n = len(a)
        st, er = np.zeros(n, np.uint8), np.zeros(n, np.float32)
        pu, nu = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        mask, F = np.zeros(n, np.uint8), (np.zeros(9) if want_F else None)
        rc = lib.uvo_klt_track_filtered(self._h, prev_slot, next_slot, _ptr(a), _ptr(b), n, self._level(max_level), int(max_count), float(epsilon),
                                        float(min_eig_threshold), ctypes.byref(cam), _ptr(st), _ptr(er), _ptr(pu), _ptr(nu), float(thr), float(conf),
                                        _ptr(mask), _ptr(F))
        if rc:
            raise UvoError(rc, "uvo_klt_track_filtered")
        return b, st, er, pu, nu, mask, (None if F is None else F.reshape(3, 3))

    def fm_hypotheses(self):
        """uvo_klt_fm_hypotheses: the last findFundamentalMat call's hypotheses in draw order -- (subsets int32[h, 7], n_models int32[h],
        scores float64[h, 3]: inlier counts or LMedS medians, -1 where no model)."""
        cap = FM_MAX_HYPOTHESES
        sub, nm, sc, n = np.zeros((cap, 7), np.int32), np.zeros(cap, np.int32), np.zeros((cap, 3)), ctypes.c_int()
        rc = lib.uvo_klt_fm_hypotheses(self._h, _ptr(sub), _ptr(nm), _ptr(sc), cap, ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_klt_fm_hypotheses")
        return sub[:n.value].copy(), nm[:n.value].copy(), sc[:n.value].copy()

    def solve_pnp_ransac(self, obj, img, cam, iterations=300, reproj_err=3.0, conf=0.99):
        """uvo_klt_solve_pnp_ransac: cv::solvePnPRansac(obj, img, mK, mDistCoef, rvec, tvec, false, iterations, reproj_err, conf, inliers,
        SOLVEPNP_EPNP) of Tracking::TrackWithPnP (src/Tracking.cc:1864) on the device; cam: CameraModel (pin-hole).
        Returns (rvec float64[3], tvec float64[3], Tcw float32[4, 4], inliers int32[k] ascending, PnpInfo); info.ok == 0: no pose."""
        a = np.ascontiguousarray(obj, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(img, np.float32).reshape(-1, 2)
        if len(a) != len(b):
            raise ValueError("obj and img differ in length")
        rvec, tvec, Tcw, inl, info = np.zeros(3), np.zeros(3), np.zeros((4, 4), np.float32), np.zeros(max(len(a), 1), np.int32), PnpInfo()
        rc = lib.uvo_klt_solve_pnp_ransac(self._h, _ptr(a), _ptr(b), len(a), ctypes.byref(cam), int(iterations), float(reproj_err), float(conf),
                                          _ptr(rvec), _ptr(tvec), _ptr(Tcw), _ptr(inl), ctypes.byref(info))
        if rc:
            raise UvoError(rc, "uvo_klt_solve_pnp_ransac")
        return rvec, tvec, Tcw, inl[:info.inliers].copy(), info

    def pnp_hypotheses(self):
        """uvo_klt_pnp_hypotheses: the last solve_pnp_ransac call's hypotheses in draw order -- (subsets int32[h, 5], poses float64[h, 12]
        (R row-major, t; zeros where EPnP gave no finite pose), counts int32[h] (-1 where there is no pose))."""
        cap = FM_MAX_HYPOTHESES
        sub, poses, cnt, n = np.zeros((cap, 5), np.int32), np.zeros((cap, 12)), np.zeros(cap, np.int32), ctypes.c_int()
        rc = lib.uvo_klt_pnp_hypotheses(self._h, _ptr(sub), _ptr(poses), _ptr(cnt), cap, ctypes.byref(n))
        if rc:
            raise UvoError(rc, "uvo_klt_pnp_hypotheses")
        return sub[:n.value].copy(), poses[:n.value].copy(), cnt[:n.value].copy()


def DescriptorDistance(a, b):
    """ORBmatcher::DescriptorDistance for one pair (src/ORBmatcher.cc:1794-1810); host convenience for scripts.
    Bulk distances go through ORBmatcher.knn2 / distance_matrix on the GPU."""
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())
