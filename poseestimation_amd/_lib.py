"""ctypes binding of libso3proj.so (the C ABI declared in include/so3proj.h).

No CPU fallback: if the shared library is missing or a tensor is not on a HIP device the call
raises.  The library is looked up in-tree only (next to this file), so the driver sees the native
code that was actually loaded.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libso3proj.so")

# name -> (restype, argtypes); must list every symbol include/so3proj.h declares.
_P, _I64, _I32, _INT, _U32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_uint32
RADIANS, PREZEROED, EXACT_F64, GRAD_SCALAR, F64_MATH = 1, 2, 4, 8, 16     # include/so3proj.h: SO3_RADIANS, SO3_PREZEROED, SO3_EXACT_F64, SO3_GRAD_SCALAR, SO3_F64_MATH
SYMBOLS = {
    "so3_version": (_INT, []),
    "so3_last_error": (ctypes.c_char_p, []),
    "so3_last_kernel": (ctypes.c_char_p, []),
    "so3_project_fwd_f32": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_project_fwd_bf16": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_project_fwd_segments_f32": (_INT, [_P, _P, _P, _INT, _P]),
    "so3_capture_fusion": (_INT, [_INT]),
    "so3_capture_fused_launches": (_I64, []),
    "so3_capture_fusion_would_fuse": (_INT, [_P, _P, _P, _INT, _INT, _INT, _INT, _INT, _INT, _P, _P, _I64]),
    "so3_project_bwd_f32": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_project_bwd_bf16": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_project_fwd_f64": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_project_bwd_f64": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_frob_fwd_bwd_v2_f32": (_INT, [_P, _P, _P, _P, _P, _P, _P, _U32, _I64, _P]),
    "so3_frob_fwd_bwd_v2_bf16": (_INT, [_P, _P, _P, _P, _P, _P, _P, _U32, _I64, _P]),
    "so3_frob_loss_v2_f32": (_INT, [_P, _P, _P, _P, _P, _P, _U32, _I64, _P]),
    "so3_angle_error_v2": (_INT, [_P, _P, _P, _P, _P, _P, _U32, _I64, _P]),
    "so3_project_angle_error_v2_f32": (_INT, [_P, _P, _P, _P, _P, _P, _P, _U32, _I64, _P]),
    "so3_geodesic_f32": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_geodesic_eps_f32": (_INT, [_P, _P, _P, _P, _P, _INT, ctypes.c_float, _P, _I64, _P]),
    "so3_geodesic_eps_f64": (_INT, [_P, _P, _P, _P, _P, _INT, ctypes.c_double, _I64, _P]),
    "so3_angle_bwd_f32": (_INT, [_P, _P, _P, ctypes.c_double, ctypes.c_double, _U32, _P, _P, _I64, _P]),
    "so3_angle_bwd_f64": (_INT, [_P, _P, _P, ctypes.c_double, ctypes.c_double, _U32, _P, _P, _I64, _P]),
    "so3_angle_error_v2_f64": (_INT, [_P, _P, _P, _P, _P, _P, _U32, _I64, _P]),
    "so3_geodesic_f64": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_frob_loss_v2_f64": (_INT, [_P, _P, _P, _P, _P, _P, _U32, _I64, _P]),
    "so3_project_fwd_diag_f32": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_scale_f32": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_scale_bf16": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_reduce_workspace_bytes": (ctypes.c_size_t, []),
    "so3_se3_update_f32": (_INT, [_P, _P, _P, ctypes.c_float, ctypes.c_float, _I64, _P]),
    "so3_se3_update_bwd_f32": (_INT, [_P, _P, _P, _P, ctypes.c_float, ctypes.c_float, _I64, _P]),
    "so3_ortho6d_fwd_f32": (_INT, [_P, _P, _I64, _P]),
    "so3_ortho6d_bwd_f32": (_INT, [_P, _P, _P, _I64, _P]),
    **{"so3_%s_fwd_f32" % h: (_INT, [_P, _P, _I64, _P]) for h in ("quat", "euler", "ortho5d", "expmap")},
    **{"so3_%s_bwd_f32" % h: (_INT, [_P, _P, _P, _I64, _P]) for h in ("quat", "euler", "ortho5d", "expmap")},
    **{"so3_%s_fwd_f32" % h: (_INT, [_P, _P, _I64, _P]) for h in ("mat_to_quat", "logmap", "mat_to_euler")},
    **{"so3_%s_bwd_f32" % h: (_INT, [_P, _P, _P, _I64, _P]) for h in ("mat_to_quat", "logmap", "mat_to_euler")},
    "so3_relative_log_fwd_f32": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_relative_log_bwd_f32": (_INT, [_P, _P, _P, _P, _P, _I64, _P]),
    "so3_rotate_clouds_f32": (_INT, [_P, _P, _P, _INT, _I64, _I32, _P]),
    "so3_pc_normalize_f32": (_INT, [_P, _P, _P, _P, _I64, _I32, _P]),
    "so3_add_l1_f32": (_INT, [_P, _P, _P, _P, _P, _P, ctypes.c_float, _I64, _I32, _P]),
    "so3_add_l1_disentangled_f32": (_INT, [_P, _P, _P, _P, _P, ctypes.c_float, _I64, _I32, _P]),
    "so3_add_l2_f32": (_INT, [_P, _P, _P, _P, _P, _P, ctypes.c_float, _I64, _I32, _P]),
    "so3_add_s_fwd_f32": (_INT, [_P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P]),
    "so3_add_s_bwd_f32": (_INT, [_P, _P, _P, _P, _P, ctypes.c_float, _P, _I64, _I32, _P]),
    "so3_cloud_diameter_f32": (_INT, [_P, _P, _P, _I64, _I32, _P]),
    "so3_angle_stats_workspace_bytes": (ctypes.c_size_t, []),
    "so3_angle_stats": (_INT, [_P, _P, _I32, _P, _P, _I64, _P]),
    "so3_kabsch_f32": (_INT, [_P, _P, _P, _P, _I64, _I32, _P]),
    "so3_kabsch_bwd_f32": (_INT, [_P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P]),
    "so3_rigid_align_f32": (_INT, [_P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P]),
    "so3_rigid_align_bwd_f32": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _I32, _P]),
    "so3_nearest_f32": (_INT, [_P, _P, _I64, _P, _P, _I64, _I32, _I32, _P]),
    "so3_icp_workspace_bytes": (ctypes.c_size_t, [_I64, _I32]),
    "so3_icp_f32": (_INT, [_P, _P, _I64, _P, _P, ctypes.c_float, _I32, _P, _P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _P]),
    "so3_icp_plane_workspace_bytes": (ctypes.c_size_t, [_I64, _I32]),
    "so3_icp_plane_f32": (_INT, [_P, _P, _P, _I64, _P, _P, ctypes.c_float, ctypes.c_float, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _P]),
    "so3_chamfer_workspace_bytes": (ctypes.c_size_t, [_I64, _I32, _I32]),
    "so3_chamfer_fwd_f32": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32, _I64, _I32, _I32, _P]),
    "so3_chamfer_bwd_f32": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32, _I64, _I32, _I32, _P]),
    "so3_chamfer_normals_workspace_bytes": (ctypes.c_size_t, [_I64, _I32, _I32]),
    "so3_chamfer_normals_fwd_f32": (_INT, [_P] * 15 + [_U32, _I64, _I32, _I32, _P]),
    "so3_chamfer_normals_bwd_f32": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32, _I64, _I32, _I32, _P]),
    "so3_knn_f32": (_INT, [_P, _P, _I64, _P, _P, _P, _P, _I32, _I64, _I32, _I32, _P]),
    "so3_knn_bwd_f32": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I64, _I32, _I32, _P]),
    "so3_local_frames_f32": (_INT, [_P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I64, _I32, _I32, _P]),
    "so3_spfh_f32": (_INT, [_P, _P, _P, _P, _P, _P, _I32, _I64, _I32, _P]),
    "so3_fpfh_f32": (_INT, [_P, _P, _P, _P, _P, _P, _I32, _I64, _I32, _P]),
    "so3_ransac_score_f32": (_INT, [_P, _P, _P, _P, _P, _P, ctypes.c_float, ctypes.c_float, _P, _P, _P, _I64, _I32, _I32, _I32, _P]),
    "so3_ransac_select_f32": (_INT, [_P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_float, _P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _P]),
    "so3_fps_f32": (_INT, [_P, _P, _P, _I64, _I32, _I32, _P]),
    "so3_ball_query_f32": (_INT, [_P, _P, ctypes.c_float, _I32, _P, _P, _I64, _I32, _I32, _P]),
    "so3_three_nn_f32": (_INT, [_P, _P, _P, _P, _P, _I64, _I32, _I32, _P]),
    "so3_three_interpolate_f32": (_INT, [_P, _P, _P, _P, _I32, _I64, _I32, _I32, _I32, _P]),
    "so3_three_interpolate_bwd_f32": (_INT, [_P, _P, _P, _P, _I32, _I64, _I32, _I32, _I32, _P]),
    "so3_group_points_f32": (_INT, [_P, _P, _P, _P, _P, _I32, _I32, _I64, _I32, _I32, _I32, _I32, _P]),
    "so3_group_points_bwd_f32": (_INT, [_P, _P, _P, _P, _P, _I32, _I32, _I64, _I32, _I32, _I32, _I32, _P]),
    "so3_rotate_clouds_bwd_f32": (_INT, [_P, _P, _P, _P, _P, _INT, _I64, _I32, _P]),
    "so3_rotations_axis_angle_f32": (_INT, [_P, _P, _P, _I64, _P]),
    "so3_kabsch_synth_f32": (_INT, [_P, _P, ctypes.c_float, ctypes.c_uint32, _P, _P, _I64, _I32, _P]),
    "so3_sym_angle_error_f32": (_INT, [_P, _P, _P, _P, _I32, _I32, _P, _P, _P, _U32, _I64, _P]),
    "so3_sym_frob_loss_f32": (_INT, [_P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P, _U32, _I64, _P]),
    "so3_sym_add_f32": (_INT, [_P, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, ctypes.c_float, _U32, _I64, _I32, _P]),
}

SYM_ADD_L2, SYM_ADD_L1, SYM_ADD_MAX = 0, 1, 2      # include/so3proj.h: SO3_SYM_ADD_L2, SO3_SYM_ADD_L1, SO3_SYM_ADD_MAX (so3_sym_add_f32's flags)
CHAMFER_UNSQUARED, CHAMFER_SINGLE = 1, 2           # include/so3proj.h: SO3_CHAMFER_UNSQUARED, SO3_CHAMFER_SINGLE
CHAMFER_SIGNED_COSINE = 4                         # include/so3proj.h: SO3_CHAMFER_SIGNED_COSINE (so3_chamfer_normals_*_f32 only)
KNN_MAX_K = 64                                    # include/so3proj.h: SO3_KNN_MAX_K
ADD_S_MAX_N = 1 << 20                             # include/so3proj.h: SO3_ADD_S_MAX_N
RANSAC_MAX_HYPOTHESES = 1 << 20                   # include/so3proj.h: SO3_RANSAC_MAX_HYPOTHESES
FPS_MAX_N = 16384                                 # include/so3proj.h: SO3_FPS_MAX_N
THREE_MAX_D = 65536                               # include/so3proj.h: SO3_THREE_MAX_D
GROUP_MAX_K = 65536                               # include/so3proj.h: SO3_GROUP_MAX_K
ABI_VERSION = 210                                 # include/so3proj.h: SO3PROJ_VERSION this binding's argument lists belong to

_lock = threading.Lock()
_lib = None


class So3ProjError(RuntimeError):
    """A C-ABI call returned non-zero."""


def load():
    """dlopen libso3proj.so and declare signatures.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    f"{LIB_PATH} not found: the HIP extension has not been built. "
                    "Run `python -m poseestimation_amd.build` (needs hipcc; cross-compiles gfx950 "
                    "without a GPU). There is no CPU fallback.")
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SYMBOLS.items():
                fn = getattr(lib, name)      # AttributeError here = header/library mismatch
                fn.restype = res
                fn.argtypes = args
            built = lib.so3_version()
            if built != ABI_VERSION:      # a stale in-tree build: its argument lists are not the ones declared above
                raise ImportError(f"{LIB_PATH} reports ABI version {built}, this binding was written for {ABI_VERSION}: "
                                  "rebuild with `python -m poseestimation_amd.build --force`")
            _lib = lib
    return _lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().so3_last_error().decode("utf-8", "replace")
        raise So3ProjError(f"{what} failed with code {code}: {msg}")
