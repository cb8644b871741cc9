"""Loader for libuhc_amd.so (the HIP product library).  There is NO fallback: if the library is
missing or does not load, importing the compute path raises."""
from __future__ import annotations

import ctypes as C
import os

from ._capi import UhcCtrlDesc, UhcEnvDesc, UhcModelDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UHC_LIB") or os.path.join(_HERE, "csrc", "libuhc_amd.so")
_lib = None

# every symbol include/uhc_amd.h declares
SYMBOLS = [
    "uhc_last_error", "uhc_abi_version", "uhc_build_flags", "uhc_model_create", "uhc_model_free", "uhc_model_nM",
    "uhc_batch_create", "uhc_batch_free", "uhc_batch_set_stream", "uhc_batch_sync", "uhc_batch_set_rfc_scale",
    "uhc_batch_field", "uhc_batch_set_state", "uhc_batch_simulate", "uhc_batch_forward", "uhc_batch_set_timing",
    "uhc_batch_kernel_time", "uhc_batch_give_ups", "uhc_batch_set_overflow_mode", "uhc_batch_set_solver", "uhc_batch_set_kernel_path",
    "uhc_env_create", "uhc_env_free", "uhc_env_obs_dim", "uhc_env_field", "uhc_env_set_bank", "uhc_env_assign",
    "uhc_env_reset", "uhc_env_step", "uhc_env_set_next", "uhc_env_auto_reset", "uhc_env_set_clip_models", "uhc_env_set_end_reward", "uhc_env_set_obj_pose",
    "uhc_rollout_act", "uhc_rollout_record", "uhc_filter_scratch_doubles", "uhc_filter_push", "uhc_filter_apply",
    "uhc_expert_frames", "uhc_eval_record", "uhc_eval_metrics", "uhc_smpl_qpos",
    "uhc_env_live_begin", "uhc_env_live_push", "uhc_env_live_view", "uhc_env_live_end",
    "uhc_surface_create", "uhc_surface_free", "uhc_surface_metrics", "uhc_eval_record_pose",
    "uhc_qpos_smpl", "uhc_smpl6d_qpos",
    "uhc_env_live_slide", "uhc_env_live_window",
    "uhc_smpl_mesh_create", "uhc_smpl_mesh_free", "uhc_smpl_mesh",
    "uhc_policy_create", "uhc_policy_free", "uhc_policy_dims", "uhc_policy_set_filter", "uhc_policy_set_params", "uhc_policy_act",
    "uhc_policy_save", "uhc_policy_load",
]


class UhcError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime; it must be the one already resident when this library
    # resolves libamdhip64 (two runtimes in one process cannot both see the device)
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise UhcError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950).  uhc_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    P = C.c_void_p
    L.uhc_last_error.restype = C.c_char_p
    L.uhc_abi_version.restype = C.c_int32
    if hasattr(L, "uhc_build_flags"):  # (ABI 10; tools/ A/B runs load older builds through UHC_LIB)
        L.uhc_build_flags.restype = C.c_int32
    L.uhc_model_create.argtypes = [C.POINTER(UhcModelDesc), C.POINTER(P)]
    L.uhc_model_free.argtypes = [P]
    L.uhc_model_free.restype = None
    L.uhc_model_nM.argtypes = [P]
    L.uhc_batch_create.argtypes = [C.POINTER(P), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                   C.POINTER(UhcCtrlDesc), C.POINTER(P)]
    L.uhc_batch_free.argtypes = [P]
    L.uhc_batch_free.restype = None
    L.uhc_batch_set_stream.argtypes = [P, P]
    L.uhc_batch_sync.argtypes = [P]
    L.uhc_batch_set_rfc_scale.argtypes = [P, C.c_double]
    L.uhc_batch_field.argtypes = [P, C.c_int32, C.POINTER(P), C.POINTER(C.c_int64)]
    L.uhc_batch_set_state.argtypes = [P, P, C.c_int32, P, P]
    L.uhc_batch_simulate.argtypes = [P, P, P, P]
    L.uhc_batch_forward.argtypes = [P]
    L.uhc_batch_set_timing.argtypes = [P, C.c_int32]
    L.uhc_batch_set_overflow_mode.argtypes = [P, C.c_int32]
    L.uhc_batch_set_solver.argtypes = [P, C.c_int32, C.c_int32]
    L.uhc_batch_set_kernel_path.argtypes = [P, C.c_int32]
    L.uhc_batch_kernel_time.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.uhc_batch_give_ups.argtypes = [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.uhc_env_create.argtypes = [P, C.POINTER(UhcEnvDesc), C.POINTER(P)]
    L.uhc_env_free.argtypes = [P]
    L.uhc_env_free.restype = None
    L.uhc_env_obs_dim.argtypes = [P]
    L.uhc_env_field.argtypes = [P, C.c_int32, C.POINTER(P), C.POINTER(C.c_int64)]
    L.uhc_env_set_bank.argtypes = [P, P, C.c_int64, P, P, C.c_int32]
    L.uhc_env_assign.argtypes = [P, P, C.c_int32, P, P, P]
    L.uhc_env_reset.argtypes = [P, P, C.c_int32, P]
    L.uhc_env_set_next.argtypes = [P, P, C.c_int32, P, P, P, P]
    L.uhc_env_auto_reset.argtypes = [P]
    L.uhc_env_set_clip_models.argtypes = [P, P]
    L.uhc_env_set_obj_pose.argtypes = [P, P, C.c_int64]
    L.uhc_env_set_end_reward.argtypes = [P, C.c_double]
    L.uhc_env_step.argtypes = [P, P, P]
    I, D = C.c_int32, C.c_double
    L.uhc_rollout_act.argtypes = [P, I, I, P, I, I, P, P, P, P, P, P, P, P]
    L.uhc_rollout_record.argtypes = [P, I, I, P, P, P, P, P, P, I, I, P, P, P, P, P, P]
    L.uhc_filter_scratch_doubles.argtypes = [I, I]
    L.uhc_filter_scratch_doubles.restype = C.c_int64
    L.uhc_filter_push.argtypes = [P, P, I, I, P, P, P, P, P]
    L.uhc_filter_apply.argtypes = [P, P, I, I, P, P, P, I, I, D, P, P]
    if hasattr(L, "uhc_expert_frames"):  # (ABI 11)
        L.uhc_expert_frames.argtypes = [P, I, C.POINTER(I), C.POINTER(I), P, P, I, P, C.c_int64, P, P, I, P, D, P]
        L.uhc_expert_frames.restype = I
    if hasattr(L, "uhc_eval_record"):  # (additive within ABI 11)
        L.uhc_eval_record.argtypes = [P] + [I] * 9 + [P] * 18
        L.uhc_eval_metrics.argtypes = [P, I, I, I, I, P, P, P, P, P, C.c_int64, P, P, P, C.POINTER(I)]
        L.uhc_eval_record.restype = L.uhc_eval_metrics.restype = I
    if hasattr(L, "uhc_smpl_qpos"):  # (additive within ABI 11)
        L.uhc_smpl_qpos.argtypes = [P, I, C.POINTER(I), P, I, P, P, C.c_int64, P, P, I, P, P]
        L.uhc_smpl_qpos.restype = I
    if hasattr(L, "uhc_env_live_begin"):  # (additive within ABI 11)
        L.uhc_env_live_begin.argtypes = [P, I, I, C.POINTER(I), C.POINTER(I), P, P, I, D, P]
        L.uhc_env_live_push.argtypes = [P, P, I, P, P, P, P]
        L.uhc_env_live_view.argtypes = [P, C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(I)]
        L.uhc_env_live_end.argtypes = [P]
        L.uhc_env_live_begin.restype = L.uhc_env_live_push.restype = L.uhc_env_live_view.restype = L.uhc_env_live_end.restype = I
    if hasattr(L, "uhc_surface_create"):  # (additive within ABI 11)
        L.uhc_surface_create.argtypes = [I, I, I, P, P, P, C.POINTER(P)]
        L.uhc_surface_free.argtypes = [P]
        L.uhc_surface_free.restype = None
        L.uhc_surface_metrics.argtypes = [P, P, I, P, P, I, P, P, C.c_int64, P, C.c_int64, C.c_int64, D, P, P, P, C.POINTER(I)]
        L.uhc_eval_record_pose.argtypes = [P, I, I, I, I, P, P, P, P, P, P]
        L.uhc_surface_create.restype = L.uhc_surface_metrics.restype = L.uhc_eval_record_pose.restype = I
    if hasattr(L, "uhc_qpos_smpl"):  # (additive within ABI 11)
        L.uhc_qpos_smpl.argtypes = [P, I, C.POINTER(I), I, P, I, P, C.c_int64, I, I, P, P, P, P, P, P, C.POINTER(I)]
        L.uhc_smpl6d_qpos.argtypes = [P, I, C.POINTER(I), P, I, P, C.c_int64, P, P, I, P, P]
        L.uhc_qpos_smpl.restype = L.uhc_smpl6d_qpos.restype = I
    if hasattr(L, "uhc_env_live_slide"):  # (additive within ABI 11)
        L.uhc_env_live_slide.argtypes = [P, I]
        L.uhc_env_live_window.argtypes = [P, C.POINTER(P), C.POINTER(P)]
        L.uhc_env_live_slide.restype = L.uhc_env_live_window.restype = I
    if hasattr(L, "uhc_smpl_mesh"):  # (additive within ABI 11)
        L.uhc_smpl_mesh_create.argtypes = [I, I, P, P, P, P, P, P, C.POINTER(P)]
        L.uhc_smpl_mesh_free.argtypes = [P]
        L.uhc_smpl_mesh_free.restype = None
        L.uhc_smpl_mesh.argtypes = [P, P, I, P, P, I, P, P, P, C.c_int64, P, C.c_int64, C.c_int64, D, P, P, P, P, P, P, C.POINTER(I)]
        L.uhc_smpl_mesh_create.restype = L.uhc_smpl_mesh.restype = I
    if hasattr(L, "uhc_policy_act"):  # (additive within ABI 11)
        PI, PP = C.POINTER(I), C.POINTER(P)
        L.uhc_policy_create.argtypes = [I, I, I, I, I, PI, PI, PI, PP, PP, PP]
        L.uhc_policy_free.argtypes = [P]
        L.uhc_policy_free.restype = None
        L.uhc_policy_dims.argtypes = [P, PI, PI, PI, PI, PI, C.POINTER(C.c_int64)]
        L.uhc_policy_set_filter.argtypes = [P, D, P, P, I, I, D]
        L.uhc_policy_set_params.argtypes = [P, P, PP, PP, I]
        L.uhc_policy_act.argtypes = [P, P, I, P, C.c_int64, P, P, P]
        L.uhc_policy_save.argtypes = [P, C.c_char_p]
        L.uhc_policy_load.argtypes = [C.c_char_p, I, PP]
        for f in ("create", "dims", "set_filter", "set_params", "act", "save", "load"):
            getattr(L, "uhc_policy_" + f).restype = I
    _lib = L
    return L


def check(rc: int):
    if rc != 0:
        raise UhcError(lib().uhc_last_error().decode())
