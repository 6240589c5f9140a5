"""ctypes binding of libbuffer_hip.so (the C ABI declared in include/buffer_hip.h).

There is no CPU fallback: importing an operator without the built library, or calling one
without a HIP device, raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BUF_LIB_PATH: development aid (tools/ab.sh times two builds of the library in one GPU session); the default is the in-tree build
LIB_PATH = os.environ.get("BUF_LIB_PATH") or os.path.join(_HERE, "libbuffer_hip.so")

BUF_OK = 0


class BufferHipError(RuntimeError):
    pass


class buf_grid_t(C.Structure):
    _fields_ = [
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
        ("ns", C.c_int), ("nb", C.c_int),
        ("cells_per_elem", C.c_int64),
        ("radius", C.c_float),
        ("supports", C.c_void_p),
        ("desc", C.c_void_p), ("s_off", C.c_void_p), ("table", C.c_void_p),
        ("sorted", C.c_void_p), ("order", C.c_void_p), ("scan_tmp", C.c_void_p),
    ]


class buf_voxel_map_t(C.Structure):
    _fields_ = [
        ("buf", C.c_void_p), ("buf_bytes", C.c_size_t),
        ("nclouds", C.c_int), ("nrows", C.c_int), ("n", C.c_int),
        ("max_cells", C.c_int64),
        ("voxel", C.c_double), ("epsilon", C.c_double),
        ("clouds", C.c_void_p), ("table", C.c_void_p), ("rows", C.c_void_p), ("keys", C.c_void_p), ("row_off", C.c_void_p),
    ]


_lib = None

_vp, _i, _f, _i64, _sz = C.c_void_p, C.c_int, C.c_float, C.c_int64, C.c_size_t

_SIGNATURES = {
    "buf_last_error": (C.c_char_p, []),
    "buf_version": (_i, []),
    "buf_device_count": (_i, []),
    "buf_timing_enable": (None, [_i]),
    "buf_timing_collect": (C.c_longlong, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "buf_timing_collect_kernel": (C.c_longlong, [_i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "buf_grid_default_cells": (_i64, [_i, _i]),
    "buf_grid_ws_bytes": (_sz, [_i, _i, _i64]),
    "buf_grid_cell_dims": (_i, [C.POINTER(C.c_double), _f, _i64, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "buf_grid_build": (_i, [C.POINTER(buf_grid_t), _vp, _i, _vp, _i, _f, _i64, _vp, _sz, _vp]),
    "buf_grid_query": (_i, [C.POINTER(buf_grid_t), _vp, _i, _vp, _vp, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "buf_radius_neighbors": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _f, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "buf_grid_subsample_ws_bytes": (_sz, [_i, _i, _i64, _i]),
    "buf_grid_subsample_batch": (_i, [_vp, _i, _vp, _i, _f, _i, _vp, _i, _vp, _vp, _vp, _vp, _i64, _vp, _sz, _vp]),
    "buf_fps_ws_bytes": (_sz, [_i, _i]),
    "buf_fps": (_i, [_vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "buf_gather": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "buf_group": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "buf_ball_query": (_i, [_vp, _vp, _i, _i, _i, _f, _i, _vp, _vp]),
    "buf_three_nn": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "buf_select_patches": (_i, [_vp, _vp, _i, _i, _f, _i, _vp, _vp]),
    "buf_select_patches_batched_ws_bytes": (_sz, [_i, _i]),
    "buf_select_patches_batched": (_i, [_vp, _vp, _i, _vp, _i, _f, _i, _vp, _vp, _sz, _vp]),
    "buf_permute_clouds": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "buf_compact_ws_bytes": (_sz, [_i]),
    "buf_compact_greater": (_i, [_vp, _i, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "buf_knn_ws_bytes": (_sz, [_i, _i, _i]),
    "buf_knn1_ws_bytes": (_sz, [_i, _i, _i]),
    "buf_knn": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "buf_fps_ragged": (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "buf_svd3x3_batched": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "buf_vn_gather_block": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _f, _vp, _vp]),
    "buf_vn_gather_pre_supported": (_i, [_i, _i, _i]),
    "buf_vn_gather_pre_ws_bytes": (_sz, [_i, _i]),
    "buf_vn_gather_block_pre": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _f, _vp, _vp, _sz, _vp]),
    "buf_vn_pointwise": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp]),
    "buf_gather_max": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "buf_vn_std": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "buf_score_head_ws_bytes": (_sz, [_i, _i]),
    "buf_score_head": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _f,
                            _vp, _vp, _sz, _vp]),
    "buf_patch_voxelize_ws_bytes": (_sz, [_i]),
    "buf_patch_voxelize": (_i, [_vp, _vp, _i, _i, _f, _vp, _i, _i, _vp, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _sz, _vp]),
    "buf_cylindrical_net_wg": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_cylindrical_net_wg_form": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "buf_cylindrical_net_wg_all": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_cylindrical_net_wg_all_flags": (_i, [_vp, _vp, _vp, _vp]),
    "buf_cylindrical_net_w25": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_cylindrical_net_w25_flags": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "buf_cylindrical_net_split_safe_w25": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_winograd_f25_tile_weights": (_i, [_vp, _i, _i, _vp]),
    "buf_cylindrical_net_w25t": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "buf_cylindrical_net_split_safe_w25t": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_cyl_row6_tile_taps": (_i, [_vp, _i, _i, _vp]),
    "buf_cylindrical_net_wg_supports": (_i, [_vp, _vp]),
    "buf_cylindrical_net_wg_flags": (_i, [_vp, _vp, _vp]),
    "buf_cylindrical_net_split_safe": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_cylindrical_net_split_safe_form": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_cost_volume_net_split_safe": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_cylindrical_net_split_safe_all": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_cylindrical_net_split": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_cylindrical_net_split_head": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_split_gemm_count": (C.c_longlong, [_i, _i, _i, _i]),
    "buf_split_tile_gemm": (_i, [_vp, _i, _i, _i, _i, _vp]),
    "buf_cost_volume_net_split": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "buf_cost_volume_net_split_gather": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "buf_split_filter_count": (C.c_longlong, [_i, _i]),
    "buf_split_tile_filters": (_i, [_vp, _i, _i, _vp]),
    "buf_winograd_tile_weights": (_i, [_vp, _i, _i, _vp]),
    "buf_winograd_f24_tile_weights": (_i, [_vp, _i, _i, _vp]),
    "buf_winograd_group": (_i, [_i, _i]),
    "buf_cost_winograd_group": (_i, [_i]),
    "buf_winograd_tile_filters": (_i, [_vp, _i, _i, _i, _i, _vp]),
    "buf_voxel_downsample_ws_bytes": (_sz, [_i, _i64]),
    "buf_voxel_downsample": (_i, [_vp, _vp, _i, _i, C.c_double, _vp, _vp, _vp, _i64, _vp, _sz, _vp]),
    "buf_voxel_downsample_batch_ws_bytes": (_sz, [_i, _i, _i64]),
    "buf_voxel_downsample_batch": (_i, [_vp, _i, _i, _vp, _i, C.c_double, _vp, _vp, _i64, _vp, _sz, _vp]),
    "buf_knn_normals": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "buf_icp_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "buf_icp_batched": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _i, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp,
                             _vp, _sz, _vp]),
    "buf_gicp_batched": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _f, C.c_double, _vp, _i, C.c_double, C.c_double, _vp, _vp, _vp, _vp,
                              _vp, _vp, _sz, _vp]),
    "buf_pair_stats_ws_bytes": (_sz, [_i, _i, _i, _i, _i64]),
    "buf_pair_stats": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _f, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "buf_pose_graph_ws_bytes": (_sz, [_i, _i, _i, _i]),
    "buf_pose_graph_optimize": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_double, C.c_double, C.c_double,
                                     _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "buf_fpfh_ws_bytes": (_sz, [_i]),
    "buf_fpfh": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "buf_iss_keypoints": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, C.c_double, C.c_double, _i, _vp, _vp, _vp, _vp]),
    "buf_row_normals": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "buf_grid_knn": (_i, [C.POINTER(buf_grid_t), _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "buf_outlier_statistical_ws_bytes": (_sz, [_i]),
    "buf_outlier_statistical": (_i, [_vp, _i, _i, _vp, _i, C.c_double, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "buf_feature_match_ws_bytes": (_sz, [C.c_longlong, C.c_longlong, _i]),
    "buf_feature_match": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "buf_fgr_ws_bytes": (_sz, [_i, _i, _i]),
    "buf_fgr_batched": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, C.c_double, _i, _i, C.c_double, C.c_double, _i, C.c_double, _i, _i,
                             _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "buf_sc2_ws_bytes": (_sz, [_vp, _i, _i]),
    "buf_sc2_batched": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_double, C.c_double, C.c_double, _i, _i, C.c_double, _i, _i,
                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "buf_clique_ws_bytes": (_sz, [_vp, _i, _i, _i]),
    "buf_clique_batched": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, C.c_double, C.c_double, C.c_double, C.c_double, _i, _i, C.c_double, _i,
                                _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "buf_voxel_map_bytes": (_sz, [_i, _i, _i64]),
    "buf_voxel_map_ws_bytes": (_sz, [_i, _i, _i64]),
    "buf_voxel_map_build": (_i, [C.POINTER(buf_voxel_map_t), _vp, _vp, _vp, _i, C.c_double, C.c_double, _i64, _vp, _sz, _vp, _sz, _vp]),
    "buf_voxel_map_export": (_i, [C.POINTER(buf_voxel_map_t), _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_vgicp_ws_bytes": (_sz, [_i, _i]),
    "buf_vgicp_batched": (_i, [C.POINTER(buf_voxel_map_t), _vp, _vp, _vp, _vp, _i, _i, _vp, _i, C.c_double, C.c_double, _vp, _vp, _vp,
                               _vp, _vp, _vp, _sz, _vp]),
    "buf_match_metrics":(_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _f, _f, _f, _vp, _vp, _vp]),
    "buf_row_linear": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "buf_segment_instance_norm_ws_bytes": (_sz, [_i, _i]),
    "buf_segment_instance_norm": (_i, [_vp, _i, _i, _vp, _i, _f, _vp, _vp, _sz, _vp]),
    "buf_descriptor_head": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "buf_cost_volume_net": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "buf_cost_volume_net_gather": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "buf_cost_volume_net_w24": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "buf_cost_volume_net_w24_gather": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "buf_cost_volume_net_split_safe_w24": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_cost_volume_net_w24b": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "buf_cost_volume_net_w24b_gather": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "buf_cost_volume_net_split_safe_w24b": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_hypotheses_score": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "buf_ransac_ws_bytes": (_sz, [_i]),
    "buf_ransac_kabsch": (_i, [_vp, _vp, _vp, _i, _i, C.c_uint64, _f, _f, _vp, _vp, _vp, _sz, _vp]),
    "buf_ransac_masked_ws_bytes": (_sz, [_i, _i]),
    "buf_ransac_kabsch_masked": (_i, [_vp, _vp, _vp, _i, _i, C.c_uint64, _f, _f, _vp, _vp, _vp, _sz, _vp]),
    "buf_post_refine": (_i, [_vp, _vp, _vp, _i, _f, _i, _vp, _vp, _vp]),
    "buf_recover_poses_ws_bytes": (_sz, [_i, _i, _i]),
    "buf_recover_poses_batched": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _f, _i, _f, _f, _f, _i, _vp, _vp, _sz, _vp]),
}


def exported_symbols():
    """Names every build of the library must export (checked by the CPU test-suite)."""
    return sorted(_SIGNATURES)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BufferHipError(
                f"{LIB_PATH} is missing: build it with `python -m buffer_amd.build` "
                "(hipcc --offload-arch=gfx950). buffer_amd has no CPU fallback.")
        # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so).  Loading it first makes
        # our library bind to that same runtime instead of pulling a second one from /opt/rocm, so
        # torch's allocator/streams and our kernels share one context.
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc, what=""):
    if rc != BUF_OK:
        msg = lib().buf_last_error().decode(errors="replace")
        raise BufferHipError(f"{what} failed ({rc}): {msg}")
