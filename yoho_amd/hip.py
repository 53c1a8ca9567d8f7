"""ctypes binding of libyoho_hip.so (include/yoho_hip.h, include/yoho_knn.h, include/yoho_trainset.h, include/yoho_refine.h, include/yoho_plane.h,
include/yoho_verify.h, include/yoho_consist.h, include/yoho_keypoints.h, include/yoho_multiway.h, include/yoho_fuse.h, include/yoho_clean.h) + a thin
tensor-level wrapper.

PyTorch-ROCm tensors are the device-memory container only: every method passes
``tensor.data_ptr()`` and the current HIP stream to the C ABI.  There is NO CPU fallback: if the
library cannot be loaded, importing a GPU op raises.
"""
import ctypes as C
import os
import sys
import threading
import warnings
import numpy as np
import torch  # must be imported before the library so that both share one HIP runtime (libamdhip64.so.7)

from . import tables as _tables
from . import weights as _weights

# YOHO_LIB=exp: the experiments build (YOHO_EXPERIMENTS=1 python -m yoho_amd.build: the timing switches compiled in) - measurement tools only
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                         "libyoho_hip_exp.so" if os.environ.get("YOHO_LIB") == "exp" else "libyoho_hip.so")
_lib = None

SYMBOLS = [
    "yoho_last_error", "yoho_version", "yoho_ctx_create", "yoho_ctx_destroy", "yoho_load_partI",
    "yoho_load_partII", "yoho_partI_forward", "yoho_partI_forward_pair", "yoho_group_mean_np", "yoho_nn_search", "yoho_mutual_nn",
    "yoho_gconv_layer", "yoho_load_fcgf", "yoho_fcgf_voxelize", "yoho_fcgf_forward", "yoho_fcgf_forward_batch", "yoho_fcgf_voxelize_rotated", "yoho_rotate_select",
    "yoho_des2r", "yoho_des2r_indexed", "yoho_partII_forward", "yoho_partII_forward_indexed", "yoho_hyp_from_quat", "yoho_o_score", "yoho_c_ransac",
    "yoho_group_gather", "yoho_set_profiling", "yoho_get_kernel_ms", "yoho_set_gconv_mode", "yoho_set_partII_mode", "yoho_set_nn_grid",
    "yoho_range_status", "yoho_c_ransac_device", "yoho_group_scatter", "yoho_set_nn_prefilter", "yoho_set_fcgf_sort", "yoho_fcgf_voxelize_rotated_batch", "yoho_gconv_wgrad", "yoho_bn_stats", "yoho_bn_relu_apply", "yoho_bn_relu_apply_sub", "yoho_bn_relu_backward", "yoho_set_partI_schedule", "yoho_clock_probe", "yoho_group_transfer_batch",
    "yoho_register_pair", "yoho_vote_order", "yoho_c_draw_np", "yoho_phase_profile", "yoho_phase_read", "yoho_poison_scratch",
]
# the entries of include/yoho_knn.h: a header and a list of their own, because the two ABI tests pin SYMBOLS to include/yoho_hip.h
KNN_SYMBOLS = ["yoho_knn_search"]
KNN_MAX = 16                                # YOHO_KNN_MAX
# the entries of include/yoho_trainset.h (training-set generation), kept apart for the same reason
TRAINSET_SYMBOLS = ["yoho_radius_pairs", "yoho_trainset_gather"]
RADIUS_MAX_POINTS = 1 << 20                 # YOHO_RADIUS_MAX_POINTS
# the entries of include/yoho_refine.h (refinement behind the estimators), kept apart for the same reason
REFINE_SYMBOLS = ["yoho_nn_within", "yoho_refit_matches", "yoho_icp_refine"]
REFINE_MAX_POINTS = 1 << 22                 # YOHO_REFINE_MAX_POINTS
REFIT_MAX_ITERS = 32                        # YOHO_REFIT_MAX_ITERS
ICP_MAX_ITERS = 64                          # YOHO_ICP_MAX_ITERS
ICP_REASONS = ("iters", "converged", "few_pairs", "rank")      # YOHO_ICP_ITERS .. YOHO_ICP_RANK
# the entries of include/yoho_plane.h (normals and point-to-plane ICP), kept apart for the same reason; they reuse the limits and reasons above
PLANE_SYMBOLS = ["yoho_estimate_normals", "yoho_icp_plane"]
# the entries of include/yoho_verify.h (hypotheses verified on the clouds), kept apart for the same reason
VERIFY_SYMBOLS = ["yoho_eval_transforms", "yoho_verify_hypotheses"]
VERIFY_MAX_K = 64                           # YOHO_VERIFY_MAX_K
# the entries of include/yoho_consist.h (hypotheses from the match list alone), kept apart for the same reason
CONSIST_SYMBOLS = ["yoho_consistency_graph", "yoho_sc2_scores", "yoho_consensus_hypotheses"]
CONSIST_MAX_M = 1 << 14                     # YOHO_CONSIST_MAX_M
CONSIST_MAX_K = 64                          # YOHO_CONSIST_MAX_K
# the entry of include/yoho_keypoints.h (farthest-point sampling), kept apart for the same reason
KEYPOINT_SYMBOLS = ["yoho_fps"]
FPS_MAX_POINTS = 1 << 22                    # YOHO_FPS_MAX_POINTS
FPS_ONE_WG_MAX = 16384                      # YOHO_FPS_ONE_WG_MAX
FPS_BLOCK_POINTS = 1024                     # YOHO_FPS_BLOCK_POINTS
FPS_PATHS = {"auto": 0, "one_wg": 1, "per_pick": 2}      # YOHO_FPS_AUTO, YOHO_FPS_ONE_WG, YOHO_FPS_PER_PICK
# the entry of include/yoho_multiway.h (the information matrix of a scene's edges), kept apart for the same reason
MULTIWAY_SYMBOLS = ["yoho_edge_information"]
MULTIWAY_MAX_K = 64                         # YOHO_MULTIWAY_MAX_K
MULTIWAY_MAX_SOURCE_POINTS = 1 << 26        # YOHO_MULTIWAY_MAX_SOURCE_POINTS
# the entry of include/yoho_fuse.h (a registered scene fused into one cloud), kept apart for the same reason
FUSE_SYMBOLS = ["yoho_fuse_clouds"]
FUSE_MAX_K = 1024                           # YOHO_FUSE_MAX_K
FUSE_MAX_POINTS = 1 << 26                   # YOHO_FUSE_MAX_POINTS
# the entries of include/yoho_clean.h (k-NN inside a radius, the statistical outlier filter), kept apart for the same reason
CLEAN_SYMBOLS = ["yoho_knn_within", "yoho_statistical_outliers"]
KNN3_MAX = 32                               # YOHO_KNN3_MAX
# the entry of include/yoho_cluster.h (exact DBSCAN labels), kept apart for the same reason
CLUSTER_SYMBOLS = ["yoho_dbscan"]
# the entry of include/yoho_disk.h (exact Poisson-disk thinning), kept apart for the same reason
DISK_SYMBOLS = ["yoho_disk_sample"]
DISK_MAX_ROUNDS = 64                        # YOHO_DISK_MAX_ROUNDS
DISK_DEFAULT_ROUNDS = 16                    # Context.disk_sample's rounds per call (profiles/disk.md: what a scan needs, and the margin)
# the entries of include/yoho_salient.h (ISS saliency, thinning in the order of a priority), kept apart for the same reason
SALIENT_SYMBOLS = ["yoho_iss_saliency", "yoho_disk_sample_prio"]


class ConvW(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p)]


class BnW(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("mean", C.c_void_p), ("var", C.c_void_p)]


class PartIWeights(C.Structure):
    _fields_ = [("conv_in", ConvW), ("res_in_bn", BnW), ("res_in", ConvW), ("res_out_bn", BnW),
                ("res_out", ConvW), ("out_bn", BnW), ("conv_out", ConvW)]


class PartIIWeights(C.Structure):
    _fields_ = [("init_bn", BnW), ("init", ConvW), ("res_in_bn", BnW), ("res_in", ConvW),
                ("res_out_bn", BnW), ("res_out", ConvW), ("fc0", ConvW), ("fc0_bn", BnW),
                ("fc1", ConvW), ("fc1_bn", BnW), ("fc2", ConvW)]


def lib_path():
    return _LIB_PATH


class FcgfConfig(C.Structure):
    _fields_ = [("channels", C.c_int * 5), ("tr_channels", C.c_int * 5), ("out_channels", C.c_int),
                ("conv1_kernel_size", C.c_int), ("in_channels", C.c_int), ("normalize_feature", C.c_int)]


class PairResultC(C.Structure):
    _fields_ = [("trans", C.c_double * 12), ("matches", C.c_int32), ("best_h", C.c_int32), ("best_count", C.c_int32),
                ("hypotheses", C.c_int32), ("range_flag", C.c_int32), ("reserved", C.c_int32)]


def load_library():
    """Load libyoho_hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"{_LIB_PATH} not found: build it with `python -m yoho_amd.build` "
            "(there is no CPU fallback for the YOHO hot path)")
    lib = C.CDLL(_LIB_PATH, mode=C.RTLD_GLOBAL)
    for s in SYMBOLS + KNN_SYMBOLS + TRAINSET_SYMBOLS + REFINE_SYMBOLS + PLANE_SYMBOLS + VERIFY_SYMBOLS + CONSIST_SYMBOLS + KEYPOINT_SYMBOLS + MULTIWAY_SYMBOLS + FUSE_SYMBOLS + CLEAN_SYMBOLS + CLUSTER_SYMBOLS + DISK_SYMBOLS + SALIENT_SYMBOLS:
        if not hasattr(lib, s):
            raise RuntimeError(f"libyoho_hip.so does not export {s}")
    lib.yoho_last_error.restype = C.c_char_p
    lib.yoho_version.restype = C.c_char_p
    vp, ci = C.c_void_p, C.c_int
    lib.yoho_ctx_create.argtypes = [ci, vp, vp, vp, C.POINTER(vp)]
    lib.yoho_ctx_destroy.argtypes = [vp]
    lib.yoho_load_partI.argtypes = [vp, C.POINTER(PartIWeights)]
    lib.yoho_load_partII.argtypes = [vp, C.POINTER(PartIIWeights)]
    lib.yoho_partI_forward.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    lib.yoho_partI_forward_pair.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp]
    lib.yoho_group_mean_np.argtypes = [vp, vp, ci, vp, vp]
    lib.yoho_nn_search.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp, vp, vp]
    lib.yoho_mutual_nn.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp]
    lib.yoho_des2r.argtypes = [vp, vp, vp, ci, vp, vp, vp]
    lib.yoho_des2r_indexed.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp, vp, vp]
    lib.yoho_partII_forward_indexed.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp]
    lib.yoho_partII_forward.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, vp]
    lib.yoho_hyp_from_quat.argtypes = [vp, vp, vp, vp, vp, ci, vp, vp]
    lib.yoho_o_score.argtypes = [vp, vp, vp, ci, vp, vp, ci, C.c_double, vp, vp, vp, vp]
    lib.yoho_c_ransac.argtypes = [vp, vp, vp, ci, vp, vp, ci, C.c_double, vp, vp, vp, vp, vp, vp]
    lib.yoho_group_gather.argtypes = [vp, vp, ci, vp, vp, ci, ci, vp, vp, vp, vp]
    lib.yoho_gconv_layer.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, vp, vp]
    lib.yoho_load_fcgf.argtypes = [vp, C.POINTER(FcgfConfig), C.POINTER(vp), ci]
    lib.yoho_fcgf_voxelize.argtypes = [vp, vp, ci, C.c_double, vp, vp, C.POINTER(ci), vp]
    lib.yoho_fcgf_forward.argtypes = [vp, vp, ci, vp, vp]
    lib.yoho_fcgf_forward_batch.argtypes = [vp, vp, vp, ci, vp, vp]
    lib.yoho_set_profiling.argtypes = [vp, ci]
    lib.yoho_set_gconv_mode.argtypes = [vp, ci]
    lib.yoho_set_partII_mode.argtypes = [vp, ci]
    lib.yoho_set_partI_schedule.argtypes = [vp, ci, ci]
    lib.yoho_clock_probe.argtypes = [vp, ci, vp, vp]
    lib.yoho_group_transfer_batch.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp]
    lib.yoho_set_nn_grid.argtypes = [vp, C.c_double]
    lib.yoho_set_nn_prefilter.argtypes = [vp, ci]
    lib.yoho_set_fcgf_sort.argtypes = [vp, ci, ci]
    lib.yoho_fcgf_voxelize_rotated.argtypes = [vp, vp, ci, vp, C.c_double, vp, vp, vp, vp, vp]
    lib.yoho_rotate_select.argtypes = [vp, vp, vp, vp, ci, vp, vp]
    lib.yoho_fcgf_voxelize_rotated_batch.argtypes = [vp, vp, ci, vp, ci, C.c_double, vp, vp, vp, vp, vp]
    lib.yoho_get_kernel_ms.argtypes = [vp, ci, C.POINTER(C.c_float)]
    lib.yoho_bn_stats.argtypes = [vp, vp, ci, ci, vp, vp, vp]
    lib.yoho_bn_relu_apply.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp]
    lib.yoho_bn_relu_apply_sub.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp]
    lib.yoho_bn_relu_backward.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp]
    lib.yoho_gconv_wgrad.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp]
    lib.yoho_group_scatter.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp]
    lib.yoho_range_status.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), vp]
    lib.yoho_c_ransac_device.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, ci, C.c_uint64, C.c_double, vp, vp, vp, vp, vp]
    lib.yoho_register_pair.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, C.c_double, C.c_uint64, ci, C.POINTER(PairResultC), vp]
    lib.yoho_vote_order.argtypes = [C.c_uint32, ci, vp]
    lib.yoho_c_draw_np.argtypes = [vp, C.POINTER(ci), vp, vp, vp, ci, vp, C.POINTER(ci), C.POINTER(ci)]
    lib.yoho_phase_profile.argtypes = [vp, ci]
    lib.yoho_phase_read.argtypes = [vp, vp, vp, vp, vp]
    lib.yoho_poison_scratch.argtypes = [vp, C.c_uint32, vp]
    lib.yoho_knn_search.argtypes = [vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp]
    lib.yoho_radius_pairs.argtypes = [vp, vp, ci, vp, ci, C.c_float, vp, C.c_int64, vp, vp]
    lib.yoho_trainset_gather.argtypes = [vp, vp, ci, ci, vp, vp, ci, vp, vp]
    lib.yoho_nn_within.argtypes = [vp, vp, ci, vp, ci, C.c_float, vp, vp, vp]
    lib.yoho_refit_matches.argtypes = [vp, vp, vp, ci, vp, C.c_double, ci, vp, vp, vp, vp]
    lib.yoho_icp_refine.argtypes = [vp, vp, ci, vp, ci, vp, C.c_float, ci, C.c_double, vp, vp, vp, vp, vp]
    lib.yoho_estimate_normals.argtypes = [vp, vp, ci, C.c_float, ci, C.c_float, C.c_float, C.c_float, vp, vp, vp, vp]
    lib.yoho_icp_plane.argtypes = [vp, vp, ci, vp, ci, vp, vp, C.c_float, ci, C.c_double, vp, vp, vp, vp, vp]
    lib.yoho_eval_transforms.argtypes = [vp, vp, ci, vp, ci, vp, ci, C.c_float, vp, vp, vp, vp]
    lib.yoho_verify_hypotheses.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, ci, ci, ci, C.c_double, C.c_float, vp, vp, vp, vp, vp, vp, vp]
    lib.yoho_consistency_graph.argtypes = [vp, vp, vp, ci, C.c_double, C.c_double, vp, vp, vp]
    lib.yoho_sc2_scores.argtypes = [vp, vp, ci, vp, vp]
    lib.yoho_consensus_hypotheses.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp]
    lib.yoho_fps.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp]
    lib.yoho_edge_information.argtypes = [vp, vp, vp, ci, vp, ci, vp, C.c_float, vp, vp, vp, vp]
    lib.yoho_fuse_clouds.argtypes = [vp, vp, vp, ci, vp, vp, C.c_double, ci, ci, vp, vp, vp, vp, vp, C.c_int64, vp, vp]
    lib.yoho_knn_within.argtypes = [vp, vp, ci, vp, ci, C.c_float, ci, ci, vp, vp, vp, vp]
    lib.yoho_statistical_outliers.argtypes = [vp, vp, ci, C.c_float, ci, ci, C.c_double, vp, vp, vp, vp, vp, vp]
    lib.yoho_dbscan.argtypes = [vp, vp, ci, C.c_float, ci, vp, vp, vp, vp, vp, vp]
    lib.yoho_disk_sample.argtypes = [vp, vp, ci, C.c_float, C.c_uint32, ci, ci, vp, vp, vp]
    lib.yoho_iss_saliency.argtypes = [vp, vp, ci, C.c_float, ci, C.c_double, C.c_double, vp, vp, vp, vp]
    lib.yoho_disk_sample_prio.argtypes = [vp, vp, ci, C.c_float, vp, C.c_uint32, ci, ci, vp, vp, vp]
    for s in SYMBOLS[2:] + KNN_SYMBOLS + TRAINSET_SYMBOLS + REFINE_SYMBOLS + PLANE_SYMBOLS + VERIFY_SYMBOLS + CONSIST_SYMBOLS + KEYPOINT_SYMBOLS + MULTIWAY_SYMBOLS + FUSE_SYMBOLS + CLEAN_SYMBOLS + CLUSTER_SYMBOLS + DISK_SYMBOLS + SALIENT_SYMBOLS:
        getattr(lib, s).restype = ci
    _lib = lib
    return lib


def vote_order(seed, M):
    """np.random.RandomState(seed).shuffle(np.arange(M)) as the library computes it on the host (yoho_vote_order)"""
    lib = load_library()
    out = np.empty((M,), dtype=np.int64)
    rc = lib.yoho_vote_order(int(seed) & 0xFFFFFFFF, int(M), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise YohoError(f"libyoho_hip error {rc}: {lib.yoho_last_error().decode()}", rc)
    return out


def c_draw_np(prob, bucket_start, bucket_members, max_iter, rng=None):
    """The draws of the reference's YOHO-C loop (tests/estimator.py:113-128) taken from numpy's legacy stream in C (yoho_c_draw_np):
    rng is a np.random.RandomState or None for the global np.random state, which is advanced exactly as the reference's
    `np.random.choice(range(60), p=prob)` / `np.random.choice(bucket, 3)` calls advance it.  -> (triples (I,3) int64, draws)"""
    lib = load_library()
    src = np.random if rng is None else rng
    st = src.get_state()
    if st[0] != "MT19937":
        raise YohoError(f"c_draw_np continues numpy's legacy MT19937 stream; the generator is {st[0]!r}")
    key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
    pos = C.c_int(int(st[2]))
    prob = np.ascontiguousarray(prob, dtype=np.float64)
    start = np.ascontiguousarray(bucket_start, dtype=np.int64)
    members = np.ascontiguousarray(bucket_members, dtype=np.int64)
    if prob.shape != (60,) or start.shape != (61,) or members.ndim != 1 or int(start[-1]) > members.shape[0]:
        raise ValueError("c_draw_np: prob (60,), bucket_start (61,), bucket_members (>= bucket_start[60],)")
    tri = np.empty((max(int(max_iter), 0), 3), dtype=np.int64)
    n, draws = C.c_int(0), C.c_int(0)
    rc = lib.yoho_c_draw_np(key.ctypes.data_as(C.c_void_p), C.byref(pos), prob.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p),
                            members.ctypes.data_as(C.c_void_p), int(max_iter), tri.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(draws))
    if rc != 0:
        raise YohoError(f"libyoho_hip error {rc}: {lib.yoho_last_error().decode()}", rc)
    src.set_state((st[0], key, pos.value) + tuple(st[3:]))
    return tri[:n.value], draws.value


class YohoError(RuntimeError):
    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


GCONV_MODES = {"f32": 0, "bf16x3": 1, "fourier": 2, "fp16x2": 3, "fgemm": 4, "fgemm256": 5, "fgemm128": 6, "fgemm8": 7}
PARTII_MODES = {"f32": 0, "bf16x3": 1, "fp16x2": 2, "cgemm": 3, "cgemm8": 4}
FP16_PARTII_MODES = ("fp16x2", "cgemm", "cgemm8")       # fp16 planes: Fourier first layer, row-indexed entries, the fp16 range guard
FP16_GCONV_MODES = ("fp16x2", "fgemm", "fgemm256", "fgemm128", "fgemm8")      # arithmetic with fp16 planes: guarded by the range flag (yoho_range_status)
MAX_PAIR_KEYPOINTS = 16384                  # yoho_partI_forward_pair takes both fragments in one pass up to this many rows


def _check(rc):
    if rc != 0:
        raise YohoError(f"libyoho_hip error {rc}: {_lib.yoho_last_error().decode()}", rc)


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError(f"{name}: expected a CUDA/HIP tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


class Context:
    """One yoho_ctx per device: group tables + (optionally) PartI / PartII weights."""

    def __init__(self, device=None, so3_dir=None):
        lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("yoho_amd.hip.Context needs a visible MI355X (torch.cuda.is_available() is False)")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.tables = _tables.GroupTables(so3_dir)
        h = C.c_void_p()
        R = np.ascontiguousarray(self.tables.R32.reshape(60, 9))
        _check(lib.yoho_ctx_create(self.device, _np_ptr(R), _np_ptr(self.tables.N_u8), _np_ptr(self.tables.P_u8), C.byref(h)))
        self._h = h
        self._lib = lib
        # arithmetic modes are tracked here as well (the library reads the same variables at yoho_ctx_create)
        gm, pm = os.environ.get("YOHO_GCONV", "fgemm"), os.environ.get("YOHO_PARTII", "fp16x2")
        self.gconv_mode = gm if gm in GCONV_MODES else "fourier"
        self.partII_mode = pm if pm in PARTII_MODES else "bf16x3"
        self.set_gconv_mode(self.gconv_mode)
        self.set_partII_mode(self.partII_mode)
        self.range_fallbacks = 0            # passes repeated in bf16x3 because a value left the fp16 range (both networks, ever)
        # per network, since its checkpoint was loaded: repeats, and whether the network has been switched to bf16x3 for good
        self.range_repeats = {"gconv": 0, "partII": 0}
        self.range_sticky = {"gconv": None, "partII": None}       # None, or the mode the network ran in before it was switched
        self.range_sticky_after = int(os.environ.get("YOHO_RANGE_STICKY", "3"))    # 0: never switch, repeat every time
        self._range_pending = [False, False]  # flags read from the device but not yet consumed by a caller (range_status)
        self.partI_owner = self.partII_owner = self.fcgf_owner = None      # whose weights are resident (network objects)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.yoho_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self, "_lib", None) is not None:
            self.close()

    # ---- weights ---------------------------------------------------------------------------
    @staticmethod
    def _conv(sd, k, keep):
        w = np.ascontiguousarray(sd[k + ".weight"], dtype=np.float32)
        b = np.ascontiguousarray(sd[k + ".bias"], dtype=np.float32)
        keep += [w, b]
        return ConvW(w.ctypes.data, b.ctypes.data)

    @staticmethod
    def _bn(sd, k, keep):
        arrs = [np.ascontiguousarray(sd[k + s], dtype=np.float32) for s in (".weight", ".bias", ".running_mean", ".running_var")]
        keep += arrs
        return BnW(*[a.ctypes.data for a in arrs])

    def load_partI(self, sd, owner=None):
        """owner: the network object these weights belong to; objects sharing the context compare ``ctx.partI_owner``
        with themselves before a forward pass and upload again when another checkpoint has been loaded since."""
        self.partI_owner = owner
        self._new_checkpoint("gconv")
        sd = _weights.to_numpy_state_dict(sd)
        _weights.check_state_dict(sd, _weights.PARTI_SPEC, strict=False)
        keep = []
        p, r = "PartI_net.", "PartI_net.SO3_Conv_layers.0."
        w = PartIWeights(self._conv(sd, p + "Conv_in.0", keep),
                         self._bn(sd, r + "comb_layer_in.0", keep), self._conv(sd, r + "comb_layer_in.2", keep),
                         self._bn(sd, r + "comb_layer_out.0", keep), self._conv(sd, r + "comb_layer_out.2", keep),
                         self._bn(sd, p + "Conv_out.comb_layer.0", keep), self._conv(sd, p + "Conv_out.comb_layer.2", keep))
        _check(self._lib.yoho_load_partI(self._h, C.byref(w)))

    def load_partII(self, sd, owner=None):
        self.partII_owner = owner
        self._new_checkpoint("partII")
        sd = _weights.to_numpy_state_dict(sd)
        _weights.check_state_dict(sd, _weights.PARTII_SPEC, strict=False)
        keep = []
        r, f = "PartII_SO3_Conv_layers.0.", "PartII_To_R_FC."
        w = PartIIWeights(self._bn(sd, "Conv_init.comb_layer.0", keep), self._conv(sd, "Conv_init.comb_layer.2", keep),
                          self._bn(sd, r + "comb_layer_in.0", keep), self._conv(sd, r + "comb_layer_in.2", keep),
                          self._bn(sd, r + "comb_layer_out.0", keep), self._conv(sd, r + "comb_layer_out.2", keep),
                          self._conv(sd, f + "0", keep), self._bn(sd, f + "1", keep),
                          self._conv(sd, f + "3", keep), self._bn(sd, f + "4", keep), self._conv(sd, f + "6", keep))
        _check(self._lib.yoho_load_partII(self._h, C.byref(w)))

    # ---- training path ------------------------------------------------------------------------
    def gconv_layer(self, x, weight, bias=None, transpose=False):
        """One (1,13) group-conv layer on device tensors.  weight (cout,cin,1,13), bias (cout) or None.
        transpose=False: x (B,cin,60) -> (B,cout,60); transpose=True: x = output gradient (B,cout,60) -> input gradient (B,cin,60)."""
        cout, cin = int(weight.shape[0]), int(weight.shape[1])
        B = x.shape[0]
        xc, yc = (cout, cin) if transpose else (cin, cout)
        if x.dim() != 3 or x.shape[1] != xc or x.shape[2] != 60:
            raise ValueError(f"expected ({'B'},{xc},60), got {tuple(x.shape)}")
        y = torch.empty((B, yc, 60), dtype=torch.float32, device=x.device)
        _check(self._lib.yoho_gconv_layer(self._h, _dev(x, torch.float32, "x"), B, cin, cout, _dev(weight, torch.float32, "weight"),
                                          _dev(bias, torch.float32, "bias") if (bias is not None and not transpose) else None,
                                          1 if transpose else 0, C.c_void_p(y.data_ptr()), _stream()))
        return y

    def bn_stats(self, x):
        """per-channel mean and biased variance of a (B,C,60) tensor"""
        B, Cn = x.shape[0], x.shape[1]
        mean = torch.empty((Cn,), dtype=torch.float32, device=x.device)
        var = torch.empty((Cn,), dtype=torch.float32, device=x.device)
        _check(self._lib.yoho_bn_stats(self._h, _dev(x, torch.float32, "x"), B, Cn, C.c_void_p(mean.data_ptr()), C.c_void_p(var.data_ptr()), _stream()))
        return mean, var

    def bn_relu_apply(self, x, scale, shift):
        y = torch.empty_like(x)
        _check(self._lib.yoho_bn_relu_apply(self._h, _dev(x, torch.float32, "x"), x.shape[0], x.shape[1], _dev(scale, torch.float32, "scale"),
                                            _dev(shift, torch.float32, "shift"), C.c_void_p(y.data_ptr()), _stream()))
        return y

    def bn_relu_apply_sub(self, x, mean, scale, beta):
        """y = relu((x - mean[c]) * scale[c] + beta[c]): bn_relu_apply with the mean subtracted first (accurate where |mean| >> std)"""
        y = torch.empty_like(x)
        _check(self._lib.yoho_bn_relu_apply_sub(self._h, _dev(x, torch.float32, "x"), x.shape[0], x.shape[1], _dev(mean, torch.float32, "mean"),
                                                _dev(scale, torch.float32, "scale"), _dev(beta, torch.float32, "beta"),
                                                C.c_void_p(y.data_ptr()), _stream()))
        return y

    def bn_relu_backward(self, x, y, dy, gamma, mean, rstd, batch_stats):
        dx = torch.empty_like(x)
        dg = torch.empty((x.shape[1],), dtype=torch.float32, device=x.device)
        db = torch.empty((x.shape[1],), dtype=torch.float32, device=x.device)
        _check(self._lib.yoho_bn_relu_backward(self._h, _dev(x, torch.float32, "x"), _dev(y, torch.float32, "y"), _dev(dy, torch.float32, "dy"),
                                               x.shape[0], x.shape[1], _dev(gamma, torch.float32, "gamma"), _dev(mean, torch.float32, "mean"),
                                               _dev(rstd, torch.float32, "rstd"), 1 if batch_stats else 0, C.c_void_p(dx.data_ptr()),
                                               C.c_void_p(dg.data_ptr()), C.c_void_p(db.data_ptr()), _stream()))
        return dx, dg, db

    def gconv_wgrad(self, x, dy, want_bias=True):
        """weight / bias gradient of the (1,13) group conv: x (B,cin,60), dy (B,cout,60) -> (dW (cout,cin,1,13), db (cout) or None)"""
        B, cin, cout = x.shape[0], int(x.shape[1]), int(dy.shape[1])
        dW = torch.empty((cout, cin, 1, 13), dtype=torch.float32, device=x.device)
        db = torch.empty((cout,), dtype=torch.float32, device=x.device) if want_bias else None
        _check(self._lib.yoho_gconv_wgrad(self._h, _dev(x, torch.float32, "x"), _dev(dy, torch.float32, "dy"), B, cin, cout,
                                          C.c_void_p(dW.data_ptr()), C.c_void_p(db.data_ptr()) if want_bias else None, _stream()))
        return dW, db

    # ---- FCGF backbone ------------------------------------------------------------------------
    def load_fcgf(self, sd, channels=(0, 32, 64, 128, 256), tr_channels=(0, 64, 64, 64, 128), out_channels=32, conv1_kernel_size=7,
                  in_channels=1, normalize_feature=True, owner=None):
        """sd: FCGF backbone state_dict (torch tensors or ndarrays); architecture parameters as in fcgf_model/resunet.py.
        The convolutions run as fp16x2 split MFMA products (fp32-accurate for activations between about 2^-7 and 4094, include/yoho_hip.h
        at the FCGF section) unless the context was created with YOHO_FCGF=f32 in the environment: then the fp32 MFMA kernels are loaded."""
        self.fcgf_owner = owner
        sd = _weights.to_numpy_state_dict(sd)
        spec = _weights.fcgf_spec(tuple(channels), tuple(tr_channels), out_channels, conv1_kernel_size, in_channels)
        _weights.check_state_dict(sd, spec, strict=False)
        names = [n for n, _ in spec if not n.endswith("num_batches_tracked")]
        arrs = [np.ascontiguousarray(sd[n], dtype=np.float32) for n in names]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        cfg = FcgfConfig((C.c_int * 5)(*[int(v or 0) for v in channels]), (C.c_int * 5)(*[int(v or 0) for v in tr_channels]),
                         int(out_channels), int(conv1_kernel_size), int(in_channels), int(bool(normalize_feature)))
        _check(self._lib.yoho_load_fcgf(self._h, C.byref(cfg), ptrs, len(arrs)))
        self._fcgf_out = int(out_channels)

    def fcgf_voxelize(self, pts, voxel_size):
        """pts (n,3) f64 cuda -> (sel (m,) int64 ascending, coords (m,3) int32): first point of every voxel (fcgf_feat.py:33-43)."""
        n = pts.shape[0]
        sel = torch.empty((n,), dtype=torch.int64, device=pts.device)
        coords = torch.empty((n, 3), dtype=torch.int32, device=pts.device)
        cnt = C.c_int(0)
        _check(self._lib.yoho_fcgf_voxelize(self._h, _dev(pts, torch.float64, "pts"), n, float(voxel_size), C.c_void_p(sel.data_ptr()),
                                            C.c_void_p(coords.data_ptr()), C.byref(cnt), _stream()))
        return sel[:cnt.value], coords[:cnt.value]

    def fcgf_voxelize_rotated(self, pts, R, voxel_size, want_points=True):
        """voxelise the copy of pts (n,3) f64 cuda rotated by R (3,3) (p' = R p) without materialising it ->
        (sel, coords[, rotated selected points (m,3) f32])."""
        n = pts.shape[0]
        Rh = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(3, 3))
        sel = torch.empty((n,), dtype=torch.int64, device=pts.device)
        coords = torch.empty((n, 3), dtype=torch.int32, device=pts.device)
        ps = torch.empty((n, 3), dtype=torch.float32, device=pts.device) if want_points else None
        cnt = C.c_int(0)
        _check(self._lib.yoho_fcgf_voxelize_rotated(self._h, _dev(pts, torch.float64, "pts"), n, _np_ptr(Rh), float(voxel_size),
                                                    C.c_void_p(sel.data_ptr()), C.c_void_p(coords.data_ptr()),
                                                    C.c_void_p(ps.data_ptr()) if want_points else None, C.byref(cnt), _stream()))
        m = cnt.value
        return (sel[:m], coords[:m], ps[:m]) if want_points else (sel[:m], coords[:m])

    def fcgf_voxelize_rotated_batch(self, pts, Rs, voxel_size, want_points=True):
        """fcgf_voxelize_rotated for a list of rotations of the same cloud in one library call (one count read-back for all):
        -> list of (sel, coords[, rotated selected points]) views into shared (nb, n, ...) buffers."""
        n, nb = pts.shape[0], len(Rs)
        Rh = np.ascontiguousarray(np.stack([np.asarray(R, dtype=np.float64).reshape(3, 3) for R in Rs]))
        sel = torch.empty((nb, n), dtype=torch.int64, device=pts.device)
        coords = torch.empty((nb, n, 3), dtype=torch.int32, device=pts.device)
        ps = torch.empty((nb, n, 3), dtype=torch.float32, device=pts.device) if want_points else None
        cnt = (C.c_int * nb)()
        _check(self._lib.yoho_fcgf_voxelize_rotated_batch(self._h, _dev(pts, torch.float64, "pts"), n, _np_ptr(Rh), nb, float(voxel_size),
                                                          C.c_void_p(sel.data_ptr()), C.c_void_p(coords.data_ptr()),
                                                          C.c_void_p(ps.data_ptr()) if want_points else None, cnt, _stream()))
        out = []
        for b in range(nb):
            m = cnt[b]
            out.append((sel[b, :m], coords[b, :m], ps[b, :m]) if want_points else (sel[b, :m], coords[b, :m]))
        return out

    def rotate_select(self, pts, R, sel):
        """(float32)(R pts[sel]) for pts (n,3) f64 cuda, sel (m,) int64 cuda; R (3,3) or None."""
        m = sel.shape[0]
        out = torch.empty((m, 3), dtype=torch.float32, device=pts.device)
        Rh = None if R is None else np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(3, 3))
        _check(self._lib.yoho_rotate_select(self._h, _dev(pts, torch.float64, "pts"), _np_ptr(Rh) if Rh is not None else None,
                                            _dev(sel, torch.int64, "sel"), m, C.c_void_p(out.data_ptr()), _stream()))
        return out

    def fcgf_forward(self, coords):
        """coords (n,3) int32 cuda, distinct voxels -> (n, out_channels) f32 unit rows.  fp16x2 split products by default: a row reached by
        an activation of 4095 or more comes back as NaN (every finite row is right); there is no automatic repeat - a context created
        under YOHO_FCGF=f32 has the fp32 exponent range."""
        n = coords.shape[0]
        out = torch.empty((n, getattr(self, "_fcgf_out", 32)), dtype=torch.float32, device=coords.device)
        _check(self._lib.yoho_fcgf_forward(self._h, _dev(coords, torch.int32, "coords"), n, C.c_void_p(out.data_ptr()), _stream()))
        return out

    def fcgf_forward_batch(self, coords_list):
        """several clouds ((n_b,3) int32 cuda each) in one pass -> list of (n_b, out_channels) feature tensors (arithmetic and range as
        fcgf_forward)."""
        nb = len(coords_list)
        off = np.zeros(nb + 1, dtype=np.int32)
        off[1:] = np.cumsum([c.shape[0] for c in coords_list])
        allc = torch.cat(coords_list).contiguous()
        out = torch.empty((int(off[-1]), getattr(self, "_fcgf_out", 32)), dtype=torch.float32, device=allc.device)
        _check(self._lib.yoho_fcgf_forward_batch(self._h, _dev(allc, torch.int32, "coords"), off.ctypes.data_as(C.c_void_p), nb,
                                                 C.c_void_p(out.data_ptr()), _stream()))
        return [out[int(off[b]):int(off[b + 1])] for b in range(nb)]

    # ---- descriptor path -------------------------------------------------------------------
    # ---- fp16 range guard -------------------------------------------------------------------
    def range_status(self, consume=(True, True)):
        """(partI_overflow, partII_overflow): waits for the current stream and reads the device flags the fp16x2 kernels raise when
        a value does not fit an fp16 plane (include/yoho_hip.h).  A raised flag stays pending until a call CONSUMES that
        component: a caller that looks at one network only passes consume=(True, False) / (False, True), so a PartI overflow left
        behind by an unchecked pass is not wiped by a PartII check (and vice versa)."""
        a, b = C.c_int(0), C.c_int(0)
        rc = self._lib.yoho_range_status(self._h, C.byref(a), C.byref(b), _stream())
        if rc not in (0, -5):                      # YOHO_ERANGE is the report itself
            _check(rc)
        self._range_pending[0] |= bool(a.value)
        self._range_pending[1] |= bool(b.value)
        out = tuple(self._range_pending)
        for i in (0, 1):
            if consume[i]:
                self._range_pending[i] = False
        return out

    def poison_scratch(self, pattern):
        """test hook (yoho_poison_scratch): fill the workspace and the pair scratch with the 32-bit `pattern` on the current stream, now and
        at every later (re)allocation.  Only for contexts that run nothing but PartI / PartII passes: the other entries keep indices there."""
        _check(self._lib.yoho_poison_scratch(self._h, int(pattern) & 0xFFFFFFFF, _stream()))

    def partI_overflow(self):
        return self.range_status(consume=(True, False))[0]

    def partII_overflow(self):
        return self.range_status(consume=(False, True))[1]

    def _new_checkpoint(self, which):
        """another checkpoint for network `which`: its repeat count starts again, and a network that had been switched to bf16x3
        for the previous checkpoint goes back to the mode it was configured with"""
        self.range_repeats[which] = 0
        prev, self.range_sticky[which] = self.range_sticky[which], None
        if prev is not None:
            (self.set_gconv_mode if which == "gconv" else self.set_partII_mode)(prev)

    def _repeat_wider(self, which, fn):
        """repeat fn() with `which` ('gconv' / 'partII') switched to the bf16x3 planes (fp32 exponent range).

        A checkpoint whose activations do not fit the fp16 planes would otherwise pay fp16x2 pass + flag + bf16x3 pass on EVERY
        call, behind nothing but a RuntimeWarning per pass: after `range_sticky_after` repeats since the checkpoint was loaded the
        network STAYS in bf16x3 (about 3x the fp16x2 time, but once instead of 1 + 3), which is said once, loudly, and is visible
        in range_report(); loading another checkpoint restores the configured mode."""
        self.range_fallbacks += 1
        self.range_repeats[which] += 1
        attr, setter = ("gconv_mode", self.set_gconv_mode) if which == "gconv" else ("partII_mode", self.set_partII_mode)
        old = getattr(self, attr)
        stick = self.range_sticky_after > 0 and self.range_repeats[which] >= self.range_sticky_after and old != "bf16x3"
        if stick:
            warnings.warn(f"yoho_amd: {self.range_repeats[which]} passes of this checkpoint left the fp16 range of the {which} fp16x2 arithmetic; "
                          f"the network now STAYS in bf16x3 (fp32 exponent range, about 3x slower than {old}) until another checkpoint is "
                          f"loaded (YOHO_RANGE_STICKY=0 keeps repeating pass by pass instead)", RuntimeWarning)
        else:
            warnings.warn(f"yoho_amd: a value left the fp16 range of the {which} fp16x2 arithmetic; pass repeated in bf16x3", RuntimeWarning)
        setter("bf16x3")
        try:
            return fn()
        finally:
            if stick:
                self.range_sticky[which] = old
            else:
                setter(old)

    def range_report(self):
        """what the range guard has done on this context: repeats per network since its checkpoint was loaded, networks switched
        to bf16x3 for good, total repeats ever - for the stats of the dataset driver and the bench line"""
        return {"partI_repeats": self.range_repeats["gconv"], "partII_repeats": self.range_repeats["partII"],
                "partI_stays_bf16x3": self.range_sticky["gconv"] is not None, "partII_stays_bf16x3": self.range_sticky["partII"] is not None,
                "repeats_total": self.range_fallbacks}

    def supports_pair(self, n_rows):
        """yoho_partI_forward_pair (no concatenation copy) exists for the default arithmetic mode and one pass"""
        return self.gconv_mode in ("fgemm", "fgemm256", "fgemm128", "fgemm8") and n_rows <= MAX_PAIR_KEYPOINTS

    def supports_matched(self):
        """row-indexed PartII (yoho_partII_forward_indexed) exists for the default PartII mode"""
        return self.partII_mode in FP16_PARTII_MODES

    def partI_forward(self, x, want_inv=True, want_inv_np=False, check_range=True):
        """x (B,32,60) f32 cuda -> dict(eqv, inv[, inv_np]).  check_range: in the fp16x2 modes verify the range flag
        (one stream synchronisation) and repeat the pass in bf16x3 if it is raised; callers that pass False poll
        range_status() themselves (pipeline.run_pair does, at its first host read-back)."""
        if check_range and self.gconv_mode in FP16_GCONV_MODES:
            out = self.partI_forward(x, want_inv, want_inv_np, check_range=False)
            if self.partI_overflow():
                out = self._repeat_wider("gconv", lambda: self.partI_forward(x, want_inv, want_inv_np, check_range=False))
            return out
        B = x.shape[0]
        if x.dim() != 3 or x.shape[1] != 32 or x.shape[2] != 60:
            raise ValueError(f"group feature must be (B,32,60), got {tuple(x.shape)}")
        eqv = torch.empty_like(x)
        inv = torch.empty((B, 32), dtype=torch.float32, device=x.device) if want_inv else None
        inv_np = torch.empty((B, 32), dtype=torch.float32, device=x.device) if want_inv_np else None
        _check(self._lib.yoho_partI_forward(self._h, _dev(x, torch.float32, "x"), B, C.c_void_p(eqv.data_ptr()),
                                            C.c_void_p(inv.data_ptr()) if want_inv else None,
                                            C.c_void_p(inv_np.data_ptr()) if want_inv_np else None, _stream()))
        out = {"eqv": eqv}
        if want_inv:
            out["inv"] = inv
        if want_inv_np:
            out["inv_np"] = inv_np
        return out

    def partI_forward_pair(self, x0, x1, want_inv=True, want_inv_np=False, check_range=True):
        """both fragments in one pass, no concatenation copy: outputs have B0 + B1 rows (x0's first).  Default mode only
        (supports_pair)."""
        if check_range:
            out = self.partI_forward_pair(x0, x1, want_inv, want_inv_np, check_range=False)
            if self.partI_overflow():
                xc = torch.cat([x0, x1])
                out = self._repeat_wider("gconv", lambda: self.partI_forward(xc, want_inv, want_inv_np, check_range=False))
            return out
        B0, B1 = x0.shape[0], x1.shape[0]
        eqv = torch.empty((B0 + B1, 32, 60), dtype=torch.float32, device=x0.device)
        inv = torch.empty((B0 + B1, 32), dtype=torch.float32, device=x0.device) if want_inv else None
        inv_np = torch.empty((B0 + B1, 32), dtype=torch.float32, device=x0.device) if want_inv_np else None
        _check(self._lib.yoho_partI_forward_pair(self._h, _dev(x0, torch.float32, "x0"), B0, _dev(x1, torch.float32, "x1"), B1,
                                                 C.c_void_p(eqv.data_ptr()), C.c_void_p(inv.data_ptr()) if want_inv else None,
                                                 C.c_void_p(inv_np.data_ptr()) if want_inv_np else None, _stream()))
        out = {"eqv": eqv}
        if want_inv:
            out["inv"] = inv
        if want_inv_np:
            out["inv_np"] = inv_np
        return out

    def group_mean_np(self, eqv):
        B = eqv.shape[0]
        out = torch.empty((B, 32), dtype=torch.float32, device=eqv.device)
        _check(self._lib.yoho_group_mean_np(self._h, _dev(eqv, torch.float32, "eqv"), B, C.c_void_p(out.data_ptr()), _stream()))
        return out

    def nn_search(self, src, tgt, want_dist=True, squared=False):
        """src (Ns,D), tgt (Nt,D) f32, D in {32,3} -> (dist (Ns) f32 or None, idx (Ns) int64).
        squared=False: pdist 'L2' (sqrt(D2 + 1e-7)); True: 'SquareL2' (D2)."""
        Ns, D = src.shape
        Nt = tgt.shape[0]
        idx = torch.empty((Ns,), dtype=torch.int64, device=src.device)
        dist = torch.empty((Ns,), dtype=torch.float32, device=src.device) if want_dist else None
        _check(self._lib.yoho_nn_search(self._h, _dev(src, torch.float32, "src"), Ns, _dev(tgt, torch.float32, "tgt"), Nt, D, 1 if squared else 0,
                                        C.c_void_p(idx.data_ptr()), C.c_void_p(dist.data_ptr()) if want_dist else None, _stream()))
        return dist, idx

    def knn_search(self, src, tgt, k, want_dist=True, squared=False):
        """src (Ns,D), tgt (Nt,D) f32, D in {32,3}, 1 <= k <= min(KNN_MAX, Nt) -> (dist (Ns,k) f32 or None, idx (Ns,k) int64): the k
        nearest rows of tgt, ascending by (distance as returned, index); column 0 is nn_search's answer (yoho_knn_search)."""
        Ns, D = src.shape
        Nt = tgt.shape[0]
        k = int(k)
        idx = torch.empty((Ns, k), dtype=torch.int64, device=src.device)
        dist = torch.empty((Ns, k), dtype=torch.float32, device=src.device) if want_dist else None
        _check(self._lib.yoho_knn_search(self._h, _dev(src, torch.float32, "src"), Ns, _dev(tgt, torch.float32, "tgt"), Nt, D, 1 if squared else 0, k,
                                         C.c_void_p(idx.data_ptr()), C.c_void_p(dist.data_ptr()) if want_dist else None, _stream()))
        return dist, idx

    def radius_pairs(self, a, b, radius):
        """a (Na,3), b (Nb,3) f32 -> (M,2) int64: every (i, j) with |a_i - b_j| < radius in np.where's order (ascending i, then j), the
        distance in f32 as include/yoho_trainset.h fixes it (yoho_radius_pairs).  One call with room for a few pairs per point and
        one read of the count; a second call with the exact capacity only when that was short."""
        Na, Nb = a.shape[0], b.shape[0]
        pa, pb = _dev(a, torch.float32, "a"), _dev(b, torch.float32, "b")
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != 3 or b.shape[1] != 3:
            raise ValueError("radius_pairs: a (Na,3), b (Nb,3)")
        count = torch.empty((1,), dtype=torch.int64, device=a.device)
        cap = 4 * max(Na, Nb)
        while True:
            pairs = torch.empty((cap, 2), dtype=torch.int64, device=a.device)
            _check(self._lib.yoho_radius_pairs(self._h, pa, Na, pb, Nb, float(radius), C.c_void_p(pairs.data_ptr()) if cap else None, cap,
                                               C.c_void_p(count.data_ptr()), _stream()))
            M = int(count.item())
            if M <= cap:
                return pairs[:M]
            cap = M

    def trainset_gather(self, feats, rot, key):
        """feats (nr,kn,32,60) f32 on the device, rot / key (B) host integer arrays -> (B,32,60) f32: out[b] = feats[rot[b], key[b]],
        rows copied unchanged (yoho_trainset_gather; the indices are checked on the host and travel in kernel arguments)."""
        if feats.dim() != 4 or tuple(feats.shape[2:]) != (32, 60):
            raise ValueError("trainset_gather: feats (nr,kn,32,60)")
        rot = np.ascontiguousarray(rot, dtype=np.int64).reshape(-1)
        key = np.ascontiguousarray(key, dtype=np.int64).reshape(-1)
        if rot.shape != key.shape:
            raise ValueError("trainset_gather: rot and key must have one length")
        B = rot.shape[0]
        out = torch.empty((B, 32, 60), dtype=torch.float32, device=feats.device)
        _check(self._lib.yoho_trainset_gather(self._h, _dev(feats, torch.float32, "feats"), feats.shape[0], feats.shape[1], _np_ptr(rot), _np_ptr(key), B,
                                              C.c_void_p(out.data_ptr()), _stream()))
        return out

    # ---- refinement (include/yoho_refine.h) -------------------------------------------------
    def nn_within(self, q, tgt, max_dist, want_d2=True):
        """q (Nq,3), tgt (Nt,3) f32 -> (d2 (Nq) f32 or None, idx (Nq) int64): the nearest row of tgt strictly inside max_dist - nn_search's
        D = 3 squared answer kept iff it is below the gate -, idx -1 / d2 +inf where there is none (yoho_nn_within)."""
        if q.dim() != 2 or tgt.dim() != 2 or q.shape[1] != 3 or tgt.shape[1] != 3:
            raise ValueError("nn_within: q (Nq,3), tgt (Nt,3)")
        Nq, Nt = q.shape[0], tgt.shape[0]
        idx = torch.empty((Nq,), dtype=torch.int64, device=q.device)
        d2 = torch.empty((Nq,), dtype=torch.float32, device=q.device) if want_d2 else None
        _check(self._lib.yoho_nn_within(self._h, _dev(q, torch.float32, "q"), Nq, _dev(tgt, torch.float32, "tgt"), Nt, float(max_dist),
                                        C.c_void_p(idx.data_ptr()), C.c_void_p(d2.data_ptr()) if want_d2 else None, _stream()))
        return d2, idx

    # ---- k-NN inside a radius and the outlier filter (include/yoho_clean.h) -------------------
    def knn_within(self, q, tgt, max_dist, k, skip_same_row=False, want_idx=True, want_d2=True, want_count=True):
        """q (Nq,3), tgt (Nt,3) f32, 1 <= k <= KNN3_MAX -> (d2 (Nq,k) f32, idx (Nq,k) int64, count (Nq) int32), each None when not
        wanted: the k rows of tgt nearest to every query strictly inside max_dist, ascending by (d2, index), -1 / +inf where there are
        fewer; count is the exact number inside the gate, not capped at k.  skip_same_row: row i is no neighbour of query i (q is tgt).
        Without idx and d2 the call only counts (yoho_knn_within)."""
        if q.dim() != 2 or tgt.dim() != 2 or q.shape[1] != 3 or tgt.shape[1] != 3:
            raise ValueError("knn_within: q (Nq,3), tgt (Nt,3)")
        Nq, Nt, k = q.shape[0], tgt.shape[0], int(k)
        idx = torch.empty((Nq, max(k, 0)), dtype=torch.int64, device=q.device) if want_idx else None
        d2 = torch.empty((Nq, max(k, 0)), dtype=torch.float32, device=q.device) if want_d2 else None
        count = torch.empty((Nq,), dtype=torch.int32, device=q.device) if want_count else None
        _check(self._lib.yoho_knn_within(self._h, _dev(q, torch.float32, "q"), Nq, _dev(tgt, torch.float32, "tgt"), Nt, float(max_dist), k,
                                         1 if skip_same_row else 0, C.c_void_p(idx.data_ptr()) if want_idx else None,
                                         C.c_void_p(d2.data_ptr()) if want_d2 else None, C.c_void_p(count.data_ptr()) if want_count else None, _stream()))
        return d2, idx, count

    def statistical_outliers(self, pts, max_dist, k=16, min_found=1, std_ratio=2.0, want_mean_dist=True, want_count=True):
        """pts (N,3) f32 -> dict(keep (N) uint8, mean_dist (N) f64 or None, count (N) int32 or None, stats (4) f64 = (n_valid, mu, sigma,
        thr), n_keep (1) int32), device tensors: mean_dist the mean distance to the min(k, count) nearest other points inside max_dist
        (NaN with fewer than min_found of them), keep = valid and mean_dist <= mu + std_ratio * sigma (yoho_statistical_outliers)."""
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError("statistical_outliers: pts (N,3)")
        N = pts.shape[0]
        keep = torch.empty((N,), dtype=torch.uint8, device=pts.device)
        mean_dist = torch.empty((N,), dtype=torch.float64, device=pts.device) if want_mean_dist else None
        count = torch.empty((N,), dtype=torch.int32, device=pts.device) if want_count else None
        stats = torch.empty((4,), dtype=torch.float64, device=pts.device)
        n_keep = torch.empty((1,), dtype=torch.int32, device=pts.device)
        _check(self._lib.yoho_statistical_outliers(self._h, _dev(pts, torch.float32, "pts"), N, float(max_dist), int(k), int(min_found), float(std_ratio),
                                                   C.c_void_p(mean_dist.data_ptr()) if want_mean_dist else None,
                                                   C.c_void_p(count.data_ptr()) if want_count else None, C.c_void_p(keep.data_ptr()),
                                                   C.c_void_p(stats.data_ptr()), C.c_void_p(n_keep.data_ptr()), _stream()))
        return {"keep": keep, "mean_dist": mean_dist, "count": count, "stats": stats, "n_keep": n_keep}

    # ---- density clusters (include/yoho_cluster.h) ----------------------------------------------
    def dbscan(self, pts, eps, min_pts=4, want_count=True, want_core=True, want_sizes=True):
        """pts (N,3) f32 -> dict(labels (N) int32, count (N) int32 or None, core (N) uint8 or None, sizes (N) int32 or None, n (3) int32 =
        (clusters, core rows, noise rows)), device tensors: exact DBSCAN.  count = knn_within's other rows strictly inside eps, core =
        finite and count + 1 >= min_pts, a cluster = a connected component of neighbouring core rows plus the border rows whose nearest
        core neighbour (smallest (d2, index)) is in it, numbered by lowest core row; -1 = noise; sizes[c] = the members of cluster c, 0
        behind the last (yoho_dbscan)."""
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError("dbscan: pts (N,3)")
        N = pts.shape[0]
        labels = torch.empty((N,), dtype=torch.int32, device=pts.device)
        count = torch.empty((N,), dtype=torch.int32, device=pts.device) if want_count else None
        core = torch.empty((N,), dtype=torch.uint8, device=pts.device) if want_core else None
        sizes = torch.empty((N,), dtype=torch.int32, device=pts.device) if want_sizes else None
        n = torch.empty((3,), dtype=torch.int32, device=pts.device)
        _check(self._lib.yoho_dbscan(self._h, _dev(pts, torch.float32, "pts"), N, float(eps), int(min_pts), C.c_void_p(labels.data_ptr()),
                                     C.c_void_p(count.data_ptr()) if want_count else None, C.c_void_p(core.data_ptr()) if want_core else None,
                                     C.c_void_p(sizes.data_ptr()) if want_sizes else None, C.c_void_p(n.data_ptr()), _stream()))
        return {"labels": labels, "count": count, "core": core, "sizes": sizes, "n": n}

    # ---- Poisson-disk thinning (include/yoho_disk.h) ---------------------------------------------
    def disk_sample(self, pts, radius, seed=0, rounds=DISK_DEFAULT_ROUNDS, state=None):
        """pts (N,3) f32 -> (state (N) uint8: 0 undecided, 1 kept, 2 dropped; n (3) int32 = (kept rows, rounds that ran, rows still
        undecided)), device tensors: the maximal set of rows no two of which are closer than radius, greedy in the order of
        key(i) = mix32(i ^ seed), by at most `rounds` synchronous rounds.  state=None starts afresh; a state that a call with the same
        pts, radius and seed returned is continued IN PLACE (and returned) while n[2] > 0 (yoho_disk_sample)."""
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError("disk_sample: pts (N,3)")
        N = pts.shape[0]
        resume = state is not None
        if resume:
            if state.dtype != torch.uint8 or tuple(state.shape) != (N,) or not state.is_contiguous() or state.device != pts.device:
                raise ValueError("disk_sample: state (N) uint8, contiguous, on the device of pts")
        else:
            state = torch.empty((N,), dtype=torch.uint8, device=pts.device)
        n = torch.empty((3,), dtype=torch.int32, device=pts.device)
        _check(self._lib.yoho_disk_sample(self._h, _dev(pts, torch.float32, "pts"), N, float(radius), int(seed) & 0xFFFFFFFF, int(rounds),
                                          1 if resume else 0, C.c_void_p(state.data_ptr()), C.c_void_p(n.data_ptr()), _stream()))
        return state, n

    # ---- salient keypoints (include/yoho_salient.h) --------------------------------------------------
    def iss_saliency(self, pts, radius, min_nbrs=5, gamma21=0.975, gamma32=0.975, want_eig=False):
        """pts (N,3) f32 -> (prio (N) f32, count (N) int32[, eig (N,3) f64]), device tensors: the eigenvalues l1 <= l2 <= l3 of the f64
        covariance of the neighbours inside `radius` (the point itself included; count = their number), divided by the count and
        clamped at 0; prio = l1 where count >= min_nbrs, l2 < gamma21 l3 and l1 < gamma32 l2, NaN elsewhere (yoho_iss_saliency)."""
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError("iss_saliency: pts (N,3)")
        N = pts.shape[0]
        prio = torch.empty((N,), dtype=torch.float32, device=pts.device)
        count = torch.empty((N,), dtype=torch.int32, device=pts.device)
        eig = torch.empty((N, 3), dtype=torch.float64, device=pts.device) if want_eig else None
        _check(self._lib.yoho_iss_saliency(self._h, _dev(pts, torch.float32, "pts"), N, float(radius), int(min_nbrs), float(gamma21), float(gamma32),
                                           C.c_void_p(count.data_ptr()), C.c_void_p(eig.data_ptr()) if want_eig else None,
                                           C.c_void_p(prio.data_ptr()), _stream()))
        return (prio, count, eig) if want_eig else (prio, count)

    def disk_sample_prio(self, pts, radius, prio, seed=0, rounds=DISK_DEFAULT_ROUNDS, state=None):
        """disk_sample in the order of prio (N) f32: higher first, NaN last, equal values in the hashed order of key(i) = mix32(i ^ seed)
        -> (state (N) uint8, n (3) int32).  state=None starts afresh; a state handed in is continued IN PLACE (and returned): a byte 0
        is undecided, any other byte is decided and stays - the state of an unfinished call, or the caller's mask, whose rows set to
        2 are never kept and block nobody (yoho_disk_sample_prio)."""
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError("disk_sample_prio: pts (N,3)")
        N = pts.shape[0]
        if prio.dtype != torch.float32 or tuple(prio.shape) != (N,) or prio.device != pts.device:
            raise ValueError("disk_sample_prio: prio (N) float32 on the device of pts")
        resume = state is not None
        if resume:
            if state.dtype != torch.uint8 or tuple(state.shape) != (N,) or not state.is_contiguous() or state.device != pts.device:
                raise ValueError("disk_sample_prio: state (N) uint8, contiguous, on the device of pts")
        else:
            state = torch.empty((N,), dtype=torch.uint8, device=pts.device)
        n = torch.empty((3,), dtype=torch.int32, device=pts.device)
        _check(self._lib.yoho_disk_sample_prio(self._h, _dev(pts, torch.float32, "pts"), N, float(radius), _dev(prio, torch.float32, "prio"),
                                               int(seed) & 0xFFFFFFFF, int(rounds), 1 if resume else 0, C.c_void_p(state.data_ptr()),
                                               C.c_void_p(n.data_ptr()), _stream()))
        return state, n

    def refit_matches(self, k0, k1, T, inlier_dist, iters=4):
        """k0, k1 (M,3) f64 matched keypoints, T (3,4) f64 on the device (a winner of o_score / c_ransac chains in without a host read)
        -> (T_out (3,4) f64, counts (iters + 1) int32, info int32[2] = (index of the iterate returned, iterates evaluated)), device
        tensors: iterated Kabsch on the inlier matches, the iterate with the most inliers (yoho_refit_matches)."""
        M, iters = k0.shape[0], int(iters)
        if tuple(k0.shape) != (M, 3) or tuple(k1.shape) != (M, 3) or T.numel() != 12:
            raise ValueError("refit_matches: k0, k1 (M,3), T (3,4)")
        T_out = torch.empty((3, 4), dtype=torch.float64, device=T.device)
        counts = torch.empty((max(iters, 0) + 1,), dtype=torch.int32, device=T.device)
        info = torch.empty((2,), dtype=torch.int32, device=T.device)
        _check(self._lib.yoho_refit_matches(self._h, _dev(k0, torch.float64, "k0") if M else None, _dev(k1, torch.float64, "k1") if M else None, M,
                                            _dev(T, torch.float64, "T"), float(inlier_dist), iters, C.c_void_p(T_out.data_ptr()),
                                            C.c_void_p(counts.data_ptr()), C.c_void_p(info.data_ptr()), _stream()))
        return T_out, counts, info

    def icp_refine(self, src, tgt, T, max_dist, iters=30, tol=0.0):
        """src (Ns,3), tgt (Nt,3) f32 clouds, T (3,4) f64 on the device mapping src onto tgt -> (T_out (3,4) f64, npairs (iters) int32,
        rmse (iters) f64, info int32[2] = (iterations made, reason: index into ICP_REASONS)), device tensors: gated point-to-point ICP
        (yoho_icp_refine); entries of npairs / rmse behind the last iteration made hold -1."""
        if src.dim() != 2 or tgt.dim() != 2 or src.shape[1] != 3 or tgt.shape[1] != 3 or T.numel() != 12:
            raise ValueError("icp_refine: src (Ns,3), tgt (Nt,3), T (3,4)")
        iters = int(iters)
        T_out = torch.empty((3, 4), dtype=torch.float64, device=T.device)
        npairs = torch.empty((max(iters, 0),), dtype=torch.int32, device=T.device)
        rmse = torch.empty((max(iters, 0),), dtype=torch.float64, device=T.device)
        info = torch.empty((2,), dtype=torch.int32, device=T.device)
        _check(self._lib.yoho_icp_refine(self._h, _dev(src, torch.float32, "src"), src.shape[0], _dev(tgt, torch.float32, "tgt"), tgt.shape[0],
                                         _dev(T, torch.float64, "T"), float(max_dist), iters, float(tol), C.c_void_p(T_out.data_ptr()),
                                         C.c_void_p(npairs.data_ptr()) if iters > 0 else None, C.c_void_p(rmse.data_ptr()) if iters > 0 else None,
                                         C.c_void_p(info.data_ptr()), _stream()))
        return T_out, npairs, rmse, info

    # ---- normals and point-to-plane ICP (include/yoho_plane.h) -------------------------------
    def estimate_normals(self, pts, radius, min_nbrs=6, viewpoint=(0, 0, 0), want_curv=False):
        """pts (N,3) f32 -> (normals (N,3) f32, count (N) int32[, curv (N) f32]), device tensors: the unit eigenvector of the smallest
        eigenvalue of the f64 covariance of the neighbours inside `radius` (the point itself included; count = their number), turned
        towards `viewpoint`; (0, 0, 0) and curv -1 where count < min_nbrs or the neighbours are collinear (yoho_estimate_normals)."""
        if pts.dim() != 2 or pts.shape[1] != 3 or len(viewpoint) != 3:
            raise ValueError("estimate_normals: pts (N,3), viewpoint (3)")
        N = pts.shape[0]
        normals = torch.empty((N, 3), dtype=torch.float32, device=pts.device)
        count = torch.empty((N,), dtype=torch.int32, device=pts.device)
        curv = torch.empty((N,), dtype=torch.float32, device=pts.device) if want_curv else None
        _check(self._lib.yoho_estimate_normals(self._h, _dev(pts, torch.float32, "pts"), N, float(radius), int(min_nbrs), float(viewpoint[0]),
                                               float(viewpoint[1]), float(viewpoint[2]), C.c_void_p(normals.data_ptr()), C.c_void_p(count.data_ptr()),
                                               C.c_void_p(curv.data_ptr()) if want_curv else None, _stream()))
        return (normals, count, curv) if want_curv else (normals, count)

    def icp_plane(self, src, tgt, tgt_normals, T, max_dist, iters=30, tol=0.0):
        """src (Ns,3), tgt (Nt,3), tgt_normals (Nt,3) f32, T (3,4) f64 on the device mapping src onto tgt -> icp_refine's tuple (T_out,
        npairs, rmse, info), device tensors: gated point-to-plane ICP (yoho_icp_plane); rmse is the point-to-plane rms in front of
        every step, a pair whose target normal is (0, 0, 0) or not finite is not kept."""
        if src.dim() != 2 or tgt.dim() != 2 or src.shape[1] != 3 or tgt.shape[1] != 3 or tuple(tgt_normals.shape) != tuple(tgt.shape) or T.numel() != 12:
            raise ValueError("icp_plane: src (Ns,3), tgt (Nt,3), tgt_normals (Nt,3), T (3,4)")
        iters = int(iters)
        T_out = torch.empty((3, 4), dtype=torch.float64, device=T.device)
        npairs = torch.empty((max(iters, 0),), dtype=torch.int32, device=T.device)
        rmse = torch.empty((max(iters, 0),), dtype=torch.float64, device=T.device)
        info = torch.empty((2,), dtype=torch.int32, device=T.device)
        _check(self._lib.yoho_icp_plane(self._h, _dev(src, torch.float32, "src"), src.shape[0], _dev(tgt, torch.float32, "tgt"), tgt.shape[0],
                                        _dev(tgt_normals, torch.float32, "tgt_normals"), _dev(T, torch.float64, "T"), float(max_dist), iters, float(tol),
                                        C.c_void_p(T_out.data_ptr()), C.c_void_p(npairs.data_ptr()) if iters > 0 else None,
                                        C.c_void_p(rmse.data_ptr()) if iters > 0 else None, C.c_void_p(info.data_ptr()), _stream()))
        return T_out, npairs, rmse, info

    # ---- hypotheses verified on the clouds (include/yoho_verify.h) ---------------------------
    def eval_transforms(self, src, tgt, T, max_dist):
        """src (Ns,3), tgt (Nt,3) f32 clouds, T (K,3,4) f64 on the device, every row mapping src onto tgt, 1 <= K <= VERIFY_MAX_K ->
        (npairs (K) int32, rmse (K) f64, cost (K) f64), device tensors: per row the source points with a partner inside max_dist, their
        rms distance (+inf without a pair) and the truncated cost SUM(paired ? d2 : max_dist^2) (yoho_eval_transforms); one grid
        build for all rows."""
        if src.dim() != 2 or tgt.dim() != 2 or src.shape[1] != 3 or tgt.shape[1] != 3 or T.dim() != 3 or tuple(T.shape[1:]) != (3, 4):
            raise ValueError("eval_transforms: src (Ns,3), tgt (Nt,3), T (K,3,4)")
        K = T.shape[0]
        npairs = torch.empty((K,), dtype=torch.int32, device=T.device)
        rmse = torch.empty((K,), dtype=torch.float64, device=T.device)
        cost = torch.empty((K,), dtype=torch.float64, device=T.device)
        _check(self._lib.yoho_eval_transforms(self._h, _dev(src, torch.float32, "src"), src.shape[0], _dev(tgt, torch.float32, "tgt"), tgt.shape[0],
                                              _dev(T, torch.float64, "T") if K else None, K, float(max_dist), C.c_void_p(npairs.data_ptr()),
                                              C.c_void_p(rmse.data_ptr()), C.c_void_p(cost.data_ptr()), _stream()))
        return npairs, rmse, cost

    def verify_hypotheses(self, src, tgt, T, counts, K, max_dist, order=None, min_count=1, distinct_tol=0.0):
        """src (Ns,3), tgt (Nt,3) f32 clouds, T (.,3,4) f64 hypotheses, counts (H) int32 and order (H) int64 or None as o_score took /
        left them (position h = hypothesis T[order[h]] with counts[h] inliers), all on the device -> (T_out (3,4) f64, top (K) int32,
        npairs (K) int32, rmse (K) f64, cost (K) f64, info int32[4] = (Kc, best, top[best], counts[top[best]])), device tensors: the K
        positions with the most inliers among those with at least min_count - hypotheses within distinct_tol of one already taken
        are skipped -, each evaluated as eval_transforms does, T_out the one with the smallest cost (yoho_verify_hypotheses); rows
        behind Kc hold -1, T_out = [I|0] when Kc = 0.  T_out chains into refit_matches / icp_refine / icp_plane."""
        if src.dim() != 2 or tgt.dim() != 2 or src.shape[1] != 3 or tgt.shape[1] != 3 or T.dim() != 3 or tuple(T.shape[1:]) != (3, 4) or counts.dim() != 1:
            raise ValueError("verify_hypotheses: src (Ns,3), tgt (Nt,3), T (.,3,4), counts (H)")
        H, K = counts.shape[0], int(K)
        if order is not None and tuple(order.shape) != (H,):
            raise ValueError("verify_hypotheses: order must have one entry per count")
        if order is None and T.shape[0] < H:
            raise ValueError("verify_hypotheses: without an order T needs a row per count")
        dev = src.device
        T_out = torch.empty((3, 4), dtype=torch.float64, device=dev)
        top = torch.empty((max(K, 0),), dtype=torch.int32, device=dev)
        npairs = torch.empty((max(K, 0),), dtype=torch.int32, device=dev)
        rmse = torch.empty((max(K, 0),), dtype=torch.float64, device=dev)
        cost = torch.empty((max(K, 0),), dtype=torch.float64, device=dev)
        info = torch.empty((4,), dtype=torch.int32, device=dev)
        _check(self._lib.yoho_verify_hypotheses(self._h, _dev(src, torch.float32, "src"), src.shape[0], _dev(tgt, torch.float32, "tgt"), tgt.shape[0],
                                                _dev(T, torch.float64, "T") if H else None,
                                                _dev(order, torch.int64, "order") if (order is not None and H) else None,
                                                _dev(counts, torch.int32, "counts") if H else None, H, K, int(min_count), float(distinct_tol),
                                                float(max_dist), C.c_void_p(T_out.data_ptr()), C.c_void_p(top.data_ptr()), C.c_void_p(npairs.data_ptr()),
                                                C.c_void_p(rmse.data_ptr()), C.c_void_p(cost.data_ptr()), C.c_void_p(info.data_ptr()), _stream()))
        return T_out, top, npairs, rmse, cost, info

    # ---- hypotheses from the match list alone (include/yoho_consist.h) ------------------------
    def consistency_graph(self, k0, k1, tol, min_len=0.0):
        """k0, k1 (M,3) f64 matched keypoints, 1 <= M <= CONSIST_MAX_M -> (bits (M, W) int64, deg (M) int32), device tensors, W = (M + 63) // 64:
        bit j % 64 of word j // 64 of row i says that matches i and j keep their distance, | |k0[i] - k0[j]| - |k1[i] - k1[j]| | < tol with
        both lengths >= min_len (yoho_consistency_graph).  The words are the header's uint64 carried as int64: the bit pattern is the
        contract (numpy: .view(np.uint64))."""
        M = k0.shape[0]
        if tuple(k0.shape) != (M, 3) or tuple(k1.shape) != (M, 3):
            raise ValueError("consistency_graph: k0, k1 (M,3)")
        bits = torch.empty((M, (M + 63) // 64), dtype=torch.int64, device=k0.device)
        deg = torch.empty((M,), dtype=torch.int32, device=k0.device)
        _check(self._lib.yoho_consistency_graph(self._h, _dev(k0, torch.float64, "k0") if M else None, _dev(k1, torch.float64, "k1") if M else None, M,
                                                float(tol), float(min_len), C.c_void_p(bits.data_ptr()), C.c_void_p(deg.data_ptr()), _stream()))
        return bits, deg

    def sc2_scores(self, bits):
        """bits (M, W) int64 as consistency_graph leaves it -> s2 (M) int32 on the device: per match the common compatible neighbours
        summed over its compatible pairs (yoho_sc2_scores)."""
        if bits.dim() != 2 or bits.shape[1] != (bits.shape[0] + 63) // 64:
            raise ValueError("sc2_scores: bits (M, (M + 63) // 64)")
        M = bits.shape[0]
        s2 = torch.empty((M,), dtype=torch.int32, device=bits.device)
        _check(self._lib.yoho_sc2_scores(self._h, _dev(bits, torch.int64, "bits") if M else None, M, C.c_void_p(s2.data_ptr()), _stream()))
        return s2

    def consensus_hypotheses(self, k0, k1, bits, s2, K):
        """k0, k1 (M,3) f64, bits / s2 as the two methods above leave them, 1 <= K <= CONSIST_MAX_K -> (T (K,3,4) f64, seeds (K) int32,
        sizes (K) int32, info int32[2] = (Kc, M)), device tensors: greedy seeds by s2, one per cluster, the seed's set (the matches sharing
        at least half as many neighbours with it as its best partner) fitted by the Kabsch step (yoho_consensus_hypotheses).  A row whose
        set has fewer than 3 members or rank below 2 is NaN with sizes = -n; rows behind Kc hold [I|0], seeds -1, sizes 0.  T chains into
        o_score / verify_hypotheses / refit_matches without a host read."""
        M, K = k0.shape[0], int(K)
        if tuple(k0.shape) != (M, 3) or tuple(k1.shape) != (M, 3) or tuple(bits.shape) != (M, (M + 63) // 64) or tuple(s2.shape) != (M,):
            raise ValueError("consensus_hypotheses: k0, k1 (M,3), bits (M, (M + 63) // 64), s2 (M)")
        dev = k0.device
        T = torch.empty((max(K, 0), 3, 4), dtype=torch.float64, device=dev)
        seeds = torch.empty((max(K, 0),), dtype=torch.int32, device=dev)
        sizes = torch.empty((max(K, 0),), dtype=torch.int32, device=dev)
        info = torch.empty((2,), dtype=torch.int32, device=dev)
        _check(self._lib.yoho_consensus_hypotheses(self._h, _dev(k0, torch.float64, "k0") if M else None, _dev(k1, torch.float64, "k1") if M else None, M,
                                                   _dev(bits, torch.int64, "bits") if M else None, _dev(s2, torch.int32, "s2") if M else None, K,
                                                   C.c_void_p(T.data_ptr()), C.c_void_p(seeds.data_ptr()), C.c_void_p(sizes.data_ptr()),
                                                   C.c_void_p(info.data_ptr()), _stream()))
        return T, seeds, sizes, info

    # ---- keypoints (include/yoho_keypoints.h) -----------------------------------------------
    def fps(self, pts, k, start=0, want_dist2=True, path="auto"):
        """pts (m,3) f32, 0 <= k <= m -> (idx (k) int64, dist2 (k) f32 or None): exact farthest-point sampling from `start` in nn_search's
        D = 3 squared arithmetic, ties to the lowest index, the k picks distinct; dist2[0] = +inf, dist2[s] the running minimum of pick s
        when it was chosen (yoho_fps).  path "auto" / "one_wg" (m <= FPS_ONE_WG_MAX) / "per_pick": the same bytes from each."""
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError("fps: pts (m,3)")
        if path not in FPS_PATHS:
            raise ValueError(f"fps: path must be one of {sorted(FPS_PATHS)}, got {path!r}")
        m, k = pts.shape[0], int(k)
        idx = torch.empty((max(k, 0),), dtype=torch.int64, device=pts.device)
        dist2 = torch.empty((max(k, 0),), dtype=torch.float32, device=pts.device) if want_dist2 else None
        _dev(pts, torch.float32, "pts")
        if k == 0:                                   # nothing to pick (an empty tensor has no address to hand to the library)
            return idx, dist2
        _check(self._lib.yoho_fps(self._h, _dev(pts, torch.float32, "pts"), m, k, int(start), FPS_PATHS[path], C.c_void_p(idx.data_ptr()),
                                  C.c_void_p(dist2.data_ptr()) if want_dist2 else None, _stream()))
        return idx, dist2

    # ---- multiway registration (include/yoho_multiway.h) ---------------------------------------
    def edge_information(self, src, soff, tgt, T, max_dist):
        """src (S,3) f32: K source fragments one behind another, soff (K+1) int32 HOST offsets (soff[0] = 0, strictly increasing,
        soff[K] = S), tgt (Nt,3) f32 the one target, T (K,3,4) f64 source k onto the target, 1 <= K <= MULTIWAY_MAX_K ->
        (npairs (K) int32, rmse (K) f64, info (K,6,6) f64), device tensors: per edge the source points with a partner inside max_dist,
        their rms distance (+inf without a pair) and the information matrix SUM G^T G, G = [I | -[p]x] over the partners p, in the
        order (translation, rotation) (yoho_edge_information); one grid build for all K edges."""
        soff = np.ascontiguousarray(np.asarray(soff), dtype=np.int32).reshape(-1)
        K = soff.shape[0] - 1
        if src.dim() != 2 or tgt.dim() != 2 or src.shape[1] != 3 or tgt.shape[1] != 3 or T.dim() != 3 or tuple(T.shape) != (K, 3, 4):
            raise ValueError("edge_information: src (S,3), soff (K+1), tgt (Nt,3), T (K,3,4)")
        if K >= 1 and int(soff[-1]) != src.shape[0]:
            raise ValueError(f"edge_information: soff[K]={int(soff[-1])} must be the number of rows of src, {src.shape[0]}")
        npairs = torch.empty((max(K, 0),), dtype=torch.int32, device=T.device)
        rmse = torch.empty((max(K, 0),), dtype=torch.float64, device=T.device)
        info = torch.empty((max(K, 0), 6, 6), dtype=torch.float64, device=T.device)
        _check(self._lib.yoho_edge_information(self._h, _dev(src, torch.float32, "src"), _np_ptr(soff), K, _dev(tgt, torch.float32, "tgt"), tgt.shape[0],
                                               _dev(T, torch.float64, "T") if K > 0 else None, float(max_dist), C.c_void_p(npairs.data_ptr()),
                                               C.c_void_p(rmse.data_ptr()), C.c_void_p(info.data_ptr()), _stream()))
        return npairs, rmse, info

    # ---- the fused scene (include/yoho_fuse.h) ---------------------------------------------------
    def fuse_clouds(self, src, soff, T, voxel, min_count=1, min_frags=1, nrm=None, want_row_of=True, capacity=None):
        """src (S,3) f32: K fragments one behind another, soff (K+1) int32 HOST offsets (soff[0] = 0, strictly increasing, soff[K] = S),
        T (K,3,4) f64 fragment k into the scene frame, nrm (S,3) f32 or None, 1 <= K <= FUSE_MAX_K -> dict(pts (M,3) f32, normals
        (M,3) f32 or None, count (M) int32, nfrag (M) int32, row_of (S) int32 or None, M): the voxel means of the scene in ascending
        voxel key, a voxel kept iff it holds >= min_count points of >= min_frags fragments; row_of[e] the row of point e's voxel or -1
        (yoho_fuse_clouds).  capacity None: a count-only call, ONE read of M, then the sized call.  capacity given: one call and no
        read - the tensors have `capacity` rows, of which the first min(M, capacity) are written, and M is a device int64 tensor."""
        soff = np.ascontiguousarray(np.asarray(soff), dtype=np.int32).reshape(-1)
        K = soff.shape[0] - 1
        if src.dim() != 2 or src.shape[1] != 3 or T.dim() != 3 or tuple(T.shape) != (K, 3, 4) or (nrm is not None and tuple(nrm.shape) != tuple(src.shape)):
            raise ValueError("fuse_clouds: src (S,3), soff (K+1), T (K,3,4), nrm (S,3) or None")
        if K >= 1 and int(soff[-1]) != src.shape[0]:
            raise ValueError(f"fuse_clouds: soff[K]={int(soff[-1])} must be the number of rows of src, {src.shape[0]}")
        dev = src.device
        ps, pT = _dev(src, torch.float32, "src"), _dev(T, torch.float64, "T") if K > 0 else None
        pn = _dev(nrm, torch.float32, "nrm") if nrm is not None else None
        n_out = torch.empty((1,), dtype=torch.int64, device=dev)
        row_of = torch.empty((src.shape[0],), dtype=torch.int32, device=dev) if want_row_of else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None          # noqa: E731

        def run(cap, rows):
            pts = torch.empty((cap, 3), dtype=torch.float32, device=dev)
            out_nrm = torch.empty((cap, 3), dtype=torch.float32, device=dev) if nrm is not None else None
            count = torch.empty((cap,), dtype=torch.int32, device=dev)
            nfrag = torch.empty((cap,), dtype=torch.int32, device=dev)
            _check(self._lib.yoho_fuse_clouds(self._h, ps, _np_ptr(soff), K, pT, pn, float(voxel), int(min_count), int(min_frags), ptr(pts), ptr(out_nrm),
                                              ptr(count), ptr(nfrag), ptr(rows), cap, C.c_void_p(n_out.data_ptr()), _stream()))
            return {"pts": pts, "normals": out_nrm, "count": count, "nfrag": nfrag, "row_of": rows}

        if capacity is not None:
            out = run(int(capacity), row_of)
            out["M"] = n_out
            return out
        run(0, None)
        M = int(n_out.item())
        out = run(M, row_of)
        out["M"] = M
        return out

    def mutual_nn(self, a, b):
        """a (Na,32), b (Nb,32) -> (M,2) int64 mutual nearest neighbours, ascending in a."""
        Na, Nb = a.shape[0], b.shape[0]
        pairs = torch.empty((Na, 2), dtype=torch.int64, device=a.device)
        m = torch.zeros((1,), dtype=torch.int32, device=a.device)
        _check(self._lib.yoho_mutual_nn(self._h, _dev(a, torch.float32, "a"), Na, _dev(b, torch.float32, "b"), Nb,
                                        C.c_void_p(pairs.data_ptr()), C.c_void_p(m.data_ptr()), _stream()))
        return pairs[: int(m.item())]

    def des2r(self, d1, d2, want_cor=False):
        M = d1.shape[0]
        idx = torch.empty((M,), dtype=torch.int64, device=d1.device)
        cor = torch.empty((M, 60), dtype=torch.float32, device=d1.device) if want_cor else None
        _check(self._lib.yoho_des2r(self._h, _dev(d1, torch.float32, "d1"), _dev(d2, torch.float32, "d2"), M,
                                    C.c_void_p(idx.data_ptr()), C.c_void_p(cor.data_ptr()) if want_cor else None, _stream()))
        return (idx, cor) if want_cor else idx

    def des2r_matched(self, e1, e2, match):
        """Des2R(e1[match[:,1]], e2[match[:,0]]) with the rows read in place (match (M,2) int64 cuda, contiguous)."""
        M = match.shape[0]
        idx = torch.empty((M,), dtype=torch.int64, device=e1.device)
        mp = _dev(match, torch.int64, "match")
        _check(self._lib.yoho_des2r_indexed(self._h, _dev(e1, torch.float32, "e1"), C.c_void_p(match.data_ptr() + 8),
                                            _dev(e2, torch.float32, "e2"), mp, 2, M, C.c_void_p(idx.data_ptr()), None, _stream()))
        return idx

    def partII_forward_matched(self, feat0, feat1, eqv0, eqv1, match, pre_idx, check_range=True):
        """partII_forward(feat1[m1], feat0[m0], eqv1[m1], eqv0[m0], pre_idx) with m0, m1 = match[:,0], match[:,1], rows read
        in place.  Default PartII arithmetic mode only (supports_matched)."""
        if check_range:
            q = self.partII_forward_matched(feat0, feat1, eqv0, eqv1, match, pre_idx, check_range=False)
            if self.partII_overflow():
                m0, m1 = match[:, 0], match[:, 1]
                q = self._repeat_wider("partII", lambda: self.partII_forward(feat1[m1], feat0[m0], eqv1[m1], eqv0[m0], pre_idx, check_range=False))
            return q
        M = match.shape[0]
        quat = torch.empty((M, 4), dtype=torch.float32, device=feat0.device)
        m0p, m1p = C.c_void_p(_dev(match, torch.int64, "match").value), C.c_void_p(match.data_ptr() + 8)
        _check(self._lib.yoho_partII_forward_indexed(
            self._h, _dev(feat1, torch.float32, "feat1"), m1p, _dev(feat0, torch.float32, "feat0"), m0p,
            _dev(eqv1, torch.float32, "eqv1"), m1p, _dev(eqv0, torch.float32, "eqv0"), m0p, 2,
            _dev(pre_idx, torch.int64, "pre_idx"), M, C.c_void_p(quat.data_ptr()), _stream()))
        return quat

    def partII_forward(self, before_eqv0, before_eqv1, after_eqv0, after_eqv1, pre_idx, check_range=True):
        if check_range and self.partII_mode in FP16_PARTII_MODES:
            args = (before_eqv0, before_eqv1, after_eqv0, after_eqv1, pre_idx)
            q = self.partII_forward(*args, check_range=False)
            if self.partII_overflow():
                q = self._repeat_wider("partII", lambda: self.partII_forward(*args, check_range=False))
            return q
        M = before_eqv0.shape[0]
        quat = torch.empty((M, 4), dtype=torch.float32, device=before_eqv0.device)
        _check(self._lib.yoho_partII_forward(
            self._h, _dev(before_eqv0, torch.float32, "before_eqv0"), _dev(before_eqv1, torch.float32, "before_eqv1"),
            _dev(after_eqv0, torch.float32, "after_eqv0"), _dev(after_eqv1, torch.float32, "after_eqv1"),
            _dev(pre_idx, torch.int64, "pre_idx"), M, C.c_void_p(quat.data_ptr()), _stream()))
        return quat

    # ---- estimators ------------------------------------------------------------------------
    def hyp_from_quat(self, quat, idx, k0, k1):
        M = quat.shape[0]
        T = torch.empty((M, 3, 4), dtype=torch.float64, device=quat.device)
        _check(self._lib.yoho_hyp_from_quat(self._h, _dev(quat, torch.float32, "quat"), _dev(idx, torch.int64, "idx"),
                                            _dev(k0, torch.float64, "k0"), _dev(k1, torch.float64, "k1"), M,
                                            C.c_void_p(T.data_ptr()), _stream()))
        return T

    def o_score(self, k0, k1, T, order, H, d):
        """Returns (best_h, best_count, counts (H) int32) as device tensors."""
        M = k0.shape[0]
        res = torch.zeros((2,), dtype=torch.int32, device=k0.device)
        counts = torch.empty((H,), dtype=torch.int32, device=k0.device)
        _check(self._lib.yoho_o_score(self._h, _dev(k0, torch.float64, "k0"), _dev(k1, torch.float64, "k1"), M,
                                      _dev(T, torch.float64, "T"), _dev(order, torch.int64, "order") if order is not None else None,
                                      H, float(d), C.c_void_p(res.data_ptr()), C.c_void_p(res.data_ptr() + 4),
                                      C.c_void_p(counts.data_ptr()), _stream()))
        return res, counts

    def c_ransac(self, k0, k1, triples, reflect, d, want_all=False):
        M, I = k0.shape[0], triples.shape[0]
        best_T = torch.empty((3, 4), dtype=torch.float64, device=k0.device)
        res = torch.zeros((2,), dtype=torch.int32, device=k0.device)
        T_all = torch.empty((I, 3, 4), dtype=torch.float64, device=k0.device) if want_all else None
        counts = torch.empty((I,), dtype=torch.int32, device=k0.device) if want_all else None
        _check(self._lib.yoho_c_ransac(self._h, _dev(k0, torch.float64, "k0"), _dev(k1, torch.float64, "k1"), M,
                                       _dev(triples, torch.int64, "triples"),
                                       _dev(reflect, torch.uint8, "reflect") if reflect is not None else None, I, float(d),
                                       C.c_void_p(best_T.data_ptr()), C.c_void_p(res.data_ptr()), C.c_void_p(res.data_ptr() + 4),
                                       C.c_void_p(T_all.data_ptr()) if want_all else None,
                                       C.c_void_p(counts.data_ptr()) if want_all else None, _stream()))
        return best_T, res, T_all, counts

    def c_ransac_device(self, keys0, keys1, dr_index, max_iter, seed, d, match=None, want_triples=False):
        """YOHO-C with the sampling on the device (yoho_c_ransac_device): keys0 / keys1 (.,3) f64 cuda, addressed through
        the columns of match (M,2) int64 if given (else row m = match m), dr_index (M,) int64.
        Returns (best_T (3,4) f64, res int32[2] = (best_iter, best_count), triples (max_iter,3) int64 or None): device tensors."""
        M = dr_index.shape[0]
        best_T = torch.empty((3, 4), dtype=torch.float64, device=keys0.device)
        res = torch.zeros((2,), dtype=torch.int32, device=keys0.device)
        tri = torch.empty((max_iter, 3), dtype=torch.int64, device=keys0.device) if want_triples else None
        if match is not None:
            i0, i1, istride = C.c_void_p(_dev(match, torch.int64, "match").value), C.c_void_p(match.data_ptr() + 8), 2
        else:
            i0, i1, istride = None, None, 1
        _check(self._lib.yoho_c_ransac_device(self._h, _dev(keys0, torch.float64, "keys0"), i0, _dev(keys1, torch.float64, "keys1"), i1,
                                              istride, _dev(dr_index, torch.int64, "dr_index"), M, int(max_iter), int(seed) & (2 ** 64 - 1),
                                              float(d), C.c_void_p(best_T.data_ptr()), C.c_void_p(res.data_ptr()),
                                              C.c_void_p(res.data_ptr() + 4), C.c_void_p(tri.data_ptr()) if want_triples else None, _stream()))
        return best_T, res, tri

    def register_pair(self, feat0, feat1, eqv0, eqv1, inv0, inv1, keys0, keys1, estimator="yohoo", max_iter=1000, inlier_dist=0.09,
                      seed=0, selected=True):
        """One pair of described fragments in one library call (yoho_register_pair: mutual NN -> Des2R -> PartII + vote, or the
        device-sampled YOHO-C); the GIL is released for its whole duration.  feat / eqv (n,32,60) f32, inv (n,32) f32 = inv_np,
        keys (n,3) f64, all cuda.  The YOHO-O vote order is np.random.RandomState(seed & 0xFFFFFFFF)'s shuffle, the YOHO-C sampling
        stream is `seed`: the result equals pipeline.run_pair(..., order_rng=RandomState(seed & 0xFFFFFFFF), seed=seed).
        -> dict(trans (3,4) f64 or eye(4), best_h, best_count, matches, hypotheses, range_flag)"""
        if estimator not in ("yohoo", "yohoc"):
            raise ValueError(f"estimator must be 'yohoo' or 'yohoc', got {estimator!r}")
        res = PairResultC()
        est = 0 if estimator == "yohoo" else 1
        _check(self._lib.yoho_register_pair(
            self._h, _dev(feat0, torch.float32, "feat0") if est == 0 else None, _dev(feat1, torch.float32, "feat1") if est == 0 else None,
            _dev(eqv0, torch.float32, "eqv0"), _dev(eqv1, torch.float32, "eqv1"), _dev(inv0, torch.float32, "inv0"),
            _dev(inv1, torch.float32, "inv1"), _dev(keys0, torch.float64, "keys0"), _dev(keys1, torch.float64, "keys1"),
            eqv0.shape[0], eqv1.shape[0], est, int(max_iter), float(inlier_dist), int(seed) & (2 ** 64 - 1), 1 if selected else 0,
            C.byref(res), _stream()))
        ok = res.matches > 0 and res.best_count > 0
        trans = np.array(res.trans, dtype=np.float64).reshape(3, 4) if ok else np.eye(4)
        return {"trans": trans, "best_h": int(res.best_h), "best_count": int(res.best_count), "matches": int(res.matches),
                "hypotheses": int(res.hypotheses), "range_flag": bool(res.range_flag)}

    def group_gather(self, keys, pts, feat, g, out, want_idx=False):
        K, n = keys.shape[0], pts.shape[0]
        Rg = np.ascontiguousarray(self.tables.R64[g], dtype=np.float64)
        nn_idx = torch.empty((K,), dtype=torch.int64, device=keys.device) if want_idx else None
        _check(self._lib.yoho_group_gather(self._h, _dev(keys, torch.float64, "keys"), K, _dev(pts, torch.float32, "pts"),
                                           _dev(feat, torch.float32, "feat"), n, int(g), _np_ptr(Rg),
                                           _dev(out, torch.float32, "out"), C.c_void_p(nn_idx.data_ptr()) if want_idx else None,
                                           _stream()))
        return nn_idx

    def group_scatter(self, feat, idx, g, out):
        """out[:, :, g] = feat[idx] (feat (n,32) f32, idx (K,) int64, out (K,32,60) f32), in place"""
        if feat.dim() != 2 or feat.shape[1] != 32:
            raise ValueError(f"group_scatter: feat must be (n, 32) (the group feature's width, YOHO_testset.py:153-166), got {tuple(feat.shape)}")
        if idx.dim() != 1 or tuple(out.shape) != (idx.shape[0], 32, 60) or not 0 <= int(g) < 60:
            raise ValueError(f"group_scatter: idx (K,), out (K, 32, 60), 0 <= g < 60; got idx {tuple(idx.shape)}, out {tuple(out.shape)}, g {g}")
        _check(self._lib.yoho_group_scatter(self._h, _dev(feat, torch.float32, "feat"), feat.shape[0], _dev(idx, torch.int64, "idx"), idx.shape[0],
                                            int(g), _dev(out, torch.float32, "out"), _stream()))

    def group_transfer_batch(self, pts, kidx, Rs, ds_list, feat_list, g0, out):
        """The NN feature transfer of a backbone pass in one library call: for copy b, out[:, :, g0 + b] = feat_list[b][nn(R_b
        pts[kidx], ds_list[b])] (fp32 'SquareL2' search, through the hash grid when set_nn_grid is on).  pts (n,3) f64, kidx (K,)
        int64, Rs list of (3,3), ds_list[b] (m_b,3) f32, feat_list[b] (m_b,32) f32, out (K,32,60) f32; all on the device."""
        nb, K = len(Rs), kidx.shape[0]
        if not (1 <= nb <= 64 and len(ds_list) == nb and len(feat_list) == nb):
            raise ValueError("group_transfer_batch: 1..64 copies, one ds / feat tensor per rotation")
        if tuple(out.shape) != (K, 32, 60) or any(f.dim() != 2 or f.shape[1] != 32 or f.shape[0] != d.shape[0] for f, d in zip(feat_list, ds_list)):
            raise ValueError("group_transfer_batch: out (K,32,60), feat (m,32) and ds (m,3) per copy")
        Rh = np.ascontiguousarray(np.stack([np.asarray(R, dtype=np.float64).reshape(3, 3) for R in Rs]))
        dsp = (C.c_void_p * nb)(*[_dev(d, torch.float32, "ds").value for d in ds_list])
        fp = (C.c_void_p * nb)(*[_dev(f, torch.float32, "feat").value for f in feat_list])
        m = (C.c_int * nb)(*[int(d.shape[0]) for d in ds_list])
        q = torch.empty((K, 3), dtype=torch.float32, device=out.device)
        idx = torch.empty((K,), dtype=torch.int64, device=out.device)
        _check(self._lib.yoho_group_transfer_batch(self._h, _dev(pts, torch.float64, "pts"), _dev(kidx, torch.int64, "kidx"), K, _np_ptr(Rh), nb,
                                                   dsp, fp, m, int(g0), _dev(out, torch.float32, "out"), C.c_void_p(q.data_ptr()),
                                                   C.c_void_p(idx.data_ptr()), _stream()))

    def set_gconv_mode(self, mode):
        """'f32' (direct conv, fp32 MFMA), 'bf16x3' (direct conv, fp32-accurate 3-way bf16 split MFMA),
        'fourier' (group-Fourier domain conv, fp32 MFMA) or 'fp16x2' (direct conv, 2-way fp16 split MFMA) for PartI."""
        _check(self._lib.yoho_set_gconv_mode(self._h, GCONV_MODES[mode]))
        self.gconv_mode = mode

    def set_partI_schedule(self, chunk_kp=0, streams=1):
        """PartI pass of the default mode breadth-first (chunk_kp = 0) or depth-first over chunks of chunk_kp keypoints, the
        chunks on one stream or alternating over two (include/yoho_hip.h); bit-identical results."""
        _check(self._lib.yoho_set_partI_schedule(self._h, int(chunk_kp), int(streams)))

    def set_partII_mode(self, mode):
        """'f32', 'bf16x3', 'fp16x2' (13-element cone layer as an implicit GEMM; the direct cone kernel with YOHO_PARTII_CONE=direct), 'cgemm' (the same GEMM whatever that switch says) or 'cgemm8' (cgemm with fp8
        correction products) for PartII (include/yoho_hip.h: yoho_set_partII_mode)."""
        _check(self._lib.yoho_set_partII_mode(self._h, PARTII_MODES[mode]))
        self.partII_mode = mode

    def set_nn_prefilter(self, on=True):
        """mutual_nn on large sets through the MFMA pre-filter (default) or by brute force; identical match lists"""
        _check(self._lib.yoho_set_nn_prefilter(self._h, 1 if on else 0))

    def set_fcgf_sort(self, parity=True, cells=1):
        """internal row orders of the FCGF backbone: transposed convolutions over parity-sorted rows (default on), level-0 rows
        grouped by 8^3-voxel cell (0 never, 1 = default: passes of >= 2^18 voxels, 2 always; + 4: coordinate maps through hash
        tables even when the clouds fit rank-ordered bitmaps - the cell sort only exists on that path); identical outputs in the
        caller's row order either way"""
        _check(self._lib.yoho_set_fcgf_sort(self._h, 1 if parity else 0, int(cells)))

    def set_nn_grid(self, cell):
        """3-D nearest-neighbour searches (nn_search with 3 columns, group_gather) through a hash grid with this cell size
        (0 = brute force).  Same answers for any cell; pass the voxel size the target cloud was down-sampled with."""
        _check(self._lib.yoho_set_nn_grid(self._h, float(cell)))

    def clock_probe(self, microseconds, stream=None, out=None):
        """queue the one-wave clock probe (include/yoho_hip.h) on `stream` (a torch stream; default: the current one);
        returns the (3,) int64 device tensor it fills - shader MHz = t[0] / t[1] * t[2] / 1000 once the stream has run"""
        if out is None:
            out = torch.zeros(3, dtype=torch.int64, device=f"cuda:{self.device}")
            torch.cuda.current_stream().synchronize()        # the fill must not run after the probe (it is on another stream)
        st = stream.cuda_stream if stream is not None else _stream()
        _check(self._lib.yoho_clock_probe(self._h, int(microseconds), out.data_ptr(), st))
        return out

    # ---- profiling hook (bench.py) ------------------------------------------------------------
    def set_profiling(self, on=True):
        _check(self._lib.yoho_set_profiling(self._h, 1 if on else 0))

    PHASES = ("voxelise", "coordinate_maps", "kernel_maps", "conv1", "conv3x3_level0", "conv3x3_level1", "conv3x3_level2", "conv3x3_level3",
              "strided_into_level1", "strided_into_level2", "strided_into_level3", "transposed_to_level0", "transposed_to_level1",
              "transposed_to_level2", "heads_1x1_normalise", "nn_feature_transfer")

    def phase_profile(self, on=True):
        """accumulating phase timer of the raw-cloud path (include/yoho_hip.h: yoho_phase_profile); read with phase_read()"""
        _check(self._lib.yoho_phase_profile(self._h, 1 if on else 0))

    def phase_read(self):
        """-> {phase: {"ms", "mfma_flops", "launches"}} accumulated since the last read (waits for the current stream)"""
        ms, fl, ln = (np.zeros(16, dtype=np.float64) for _ in range(3))
        _check(self._lib.yoho_phase_read(self._h, _np_ptr(ms), _np_ptr(fl), _np_ptr(ln), _stream()))
        return {n: {"ms": float(ms[i]), "mfma_flops": float(fl[i]), "launches": int(ln[i])} for i, n in enumerate(self.PHASES)}

    def kernel_ms(self, which):
        ms = C.c_float(-1.0)
        _check(self._lib.yoho_get_kernel_ms(self._h, int(which), C.byref(ms)))
        return float(ms.value)


_ctx_cache = {}


def streams_overlap(ctx, s1, s2, microseconds=300):
    """True when work queued on the torch streams s1 and s2 runs concurrently.  HIP multiplexes a process's streams over a few hardware
    queues (four by default, dealt round-robin in creation order, the null stream among them): two streams that land on the same queue
    run their kernels one after the other however independent they are - about one stream in four shares the null stream's queue
    (measured: a 20 us kernel on such a stream waits for everything queued on the null stream).  Measured, not assumed: the one-wave
    clock probe (yoho_clock_probe spins for `microseconds`) on both streams, timed together - ~1 x the probe when they overlap, 2 x when
    they share a queue."""
    import time
    buf = torch.zeros((2, 3), dtype=torch.int64, device=f"cuda:{ctx.device}")
    torch.cuda.synchronize(ctx.device)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.clock_probe(microseconds, stream=s1, out=buf[0])
        ctx.clock_probe(microseconds, stream=s2, out=buf[1])
        s1.synchronize()
        s2.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best < 1.6e-6 * microseconds


_POOL_STREAMS = 32           # torch deals its streams round-robin from a pool of this many per device and priority
_lent = {}                   # device -> {cuda_stream handle: stream} concurrent_stream has handed out
_spare = {}                  # device -> {handle: (stream, handles it did not overlap)} drawn and rejected by the overlap probe
_streams_lock = threading.Lock()                   # (the ranks of a sharded run pick their streams from threads of their own)


def _draw(device, taken):
    """a stream of torch's pool whose handle is not in `taken`; None after a full turn of the pool"""
    for _ in range(_POOL_STREAMS):
        s = torch.cuda.Stream(device=device)
        if s.cuda_stream not in taken:
            return s
    return None


def concurrent_stream(ctx, others, tries=8):
    """a torch stream (normal priority) that demonstrably overlaps every stream of `others` (streams_overlap) and that no other
    holder of a stream from this function has: a fresh draw from torch's pool can be a stream handed out before (the backbone lanes,
    the run_many tail, the testset copy stream, the dataset runner's copy and worker streams), and two components would then
    serialise on one stream unnoticed - the probe only knows `others`.  A stream stays registered while an object of it handed out
    here is referenced outside the registry (torch's stream objects cannot be watched by weak references: their deallocation leaves
    them dangling).  Candidates the probe rejected are kept and tried again - unless they failed against one of `others` - before
    `tries` fresh ones are drawn; when none passes, the last one probed is returned, and when every stream of the pool is held, a
    shared one - correct, merely serialised."""
    dev = ctx.device
    with _streams_lock:
        lent, spare = _lent.setdefault(dev, {}), _spare.setdefault(dev, {})
        for h in list(lent):
            if sys.getrefcount(lent[h]) <= 2:      # the registry's reference and the call's: let go of by its holder
                del lent[h]
        cand = None
        for h in list(spare) + [None] * tries:
            if h is None:
                s, bad = _draw(dev, lent.keys() | spare.keys()), set()
                if s is None:                      # every stream of the pool is lent or spare
                    break
            else:
                s, bad = spare[h]
                if any(o.cuda_stream in bad for o in others):
                    continue                       # measured before: it shares a hardware queue with one of `others`
            cand = s
            failed = next((o for o in others if not streams_overlap(ctx, o, s)), None)
            if failed is None:
                break
            bad.add(failed.cuda_stream)
            spare[s.cuda_stream] = (s, bad)
        if cand is None:
            return torch.cuda.Stream(device=dev)
        spare.pop(cand.cuda_stream, None)
        lent[cand.cuda_stream] = cand
        return cand


def get_context(device=None, so3_dir=None, lane=0):
    """Process-wide context per (device, table directory, lane).  lane > 0: a further context with a workspace of its own for work
    queued on another stream while lane 0's runs (the backbone lanes of yoho_extractor / testset_create); it is kept, like lane 0's,
    so that its workspace is sized once per process."""
    dev = torch.cuda.current_device() if device is None else int(device)
    key = (dev, os.path.abspath(so3_dir) if so3_dir else None) + ((int(lane),) if lane else ())
    if key not in _ctx_cache:
        _ctx_cache[key] = Context(dev, so3_dir)
    return _ctx_cache[key]
