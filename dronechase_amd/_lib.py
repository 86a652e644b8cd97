"""ctypes binding of dronechase_amd/libthreatengage.so (the C ABI of include/threatengage.h).

There is no CPU fallback: if the HIP library is missing or fails to load, importing callers get a
RuntimeError that says how to build it."""
from __future__ import annotations

import ctypes as C
import os

from . import config as K

_LIB = None
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libthreatengage.so")

# every symbol include/threatengage.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "te_config_default", "te_create", "te_destroy", "te_reset", "te_observe", "te_step", "te_random_actions",
    "te_state_words", "te_get_state", "te_set_state", "te_algorithmic_bytes_per_env_step", "te_profile_begin",
    "te_profile_end", "te_debug_stamps", "te_abi_version", "te_last_error", "te_step_stacked", "te_observe_stacked", "te_observe_ally", "te_set_ally_actions", "te_wingman_info", "te_calculate_rounds", "te_observe_wingman", "te_set_wingman_actions", "te_drive_wingman", "te_quad_preset", "te_step_students", "te_set_persistent_obs",
    "te_policy_shape_check", "te_policy_param_words_shaped", "te_policy_act_shaped", "te_drive_wingman_shaped",
    "te_policy_grad_workspace_bytes_shaped", "te_policy_ppo_grad_shaped",
    "te_policy_bf16_words", "te_policy_pack_bf16", "te_policy_act_bf16", "te_drive_wingman_bf16",
    "te_policy_bf16_grad_words", "te_policy_pack_bf16_grad", "te_policy_grad_bf16_workspace_bytes", "te_policy_ppo_grad_bf16",
    "te_policy_param_words", "te_policy_act", "te_policy_grad_workspace_bytes", "te_policy_ppo_grad", "te_kernel_plan",
    "te_policy_opt_state_bytes", "te_policy_adam_step", "te_policy_adam_step_bf16", "te_policy_ppo_epoch",
    "te_rollout_gae", "te_adv_stats_workspace_bytes", "te_adv_stats",
    "te_monitor_bytes", "te_monitor_layout", "te_monitor_init", "te_monitor_step", "te_monitor_stats",
    "te_sphere_encode_param_words", "te_sphere_encode", "te_sphere_encode_grad_workspace_bytes", "te_sphere_encode_grad",
    "te_sphere_bf16_words", "te_sphere_pack_bf16", "te_sphere_encode_bf16",
    "te_dataset_layout", "te_dataset_init", "te_dataset_append", "te_dataset_gather",
)


class TEError(RuntimeError):
    pass


class MonitorOffsets(C.Structure):
    """te_monitor_offsets: byte offsets of the arrays inside an episode-monitor buffer (include/threatengage.h)."""
    _fields_ = [(n, C.c_size_t) for n in ("bytes", "n_rows", "rows", "ret", "len", "episodes", "last_ret", "last_len", "rec_info", "rec_ret", "rec_len")]


class DatasetGeom(C.Structure):
    """te_dataset_geom: the shape of an imitation dataset (include/threatengage.h)."""
    _fields_ = [(n, C.c_int32) for n in ("capacity", "max_append_rows", "n_spheres", "channels")]


class DatasetOffsets(C.Structure):
    """te_dataset_offsets: byte offsets of the header, the append scratch and the rings inside a dataset buffer (include/threatengage.h)."""
    _fields_ = [(n, C.c_size_t) for n in ("bytes", "header", "dst", "stacked", "mask", "inertial", "last_action", "teacher")]


class PolicyShape(C.Structure):
    """te_policy_shape: the policy's LIDAR channels, trunk width and head widths (include/threatengage.h)."""
    _fields_ = [("lidar_channels", C.c_int32), ("features_dim", C.c_int32), ("n_hidden", C.c_int32), ("hidden", C.c_int32 * 4)]


class PpoEpochArgs(C.Structure):
    """te_ppo_epoch_args: everything te_policy_ppo_epoch reads, in the header's order (include/threatengage.h).  The call checks
    struct_size against its own sizeof."""
    _fields_ = ([("struct_size", C.c_size_t), ("shape", PolicyShape)]
                + [(n, C.c_void_p) for n in ("params", "weights_bf16", "weights_bf16_t", "lidar", "inertial", "last_action", "action",
                                             "old_logp", "adv", "ret", "perm")]
                + [("n_perm", C.c_int64), ("batch", C.c_int32), ("clip_range", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float),
                   ("grad", C.c_void_p), ("state", C.c_void_p), ("state_bytes", C.c_size_t),
                   ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                   ("max_grad_norm", C.c_float), ("grad_scale", C.c_float),
                   ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("adv_workspace", C.c_void_p), ("adv_workspace_bytes", C.c_size_t),
                   ("adv_mean_std", C.c_void_p), ("stats", C.c_void_p), ("sums", C.c_void_p)])


def load() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m dronechase_amd.build` (needs hipcc, gfx950). "
            "dronechase_amd has no CPU or PyTorch fallback.")
    # ONE HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same soname as /opt/rocm's).  Loaded after torch,
    # libthreatengage.so binds to the copy torch already mapped and shares its device context; loaded BEFORE torch, it would pull
    # in /opt/rocm's copy, torch would then bring its own, and the first runtime reports "no ROCm-capable device" at te_create.
    import torch  # noqa: F401  (device memory / streams plumbing of every caller anyway)
    L = C.CDLL(LIB_PATH)
    vp, i32, u64 = C.c_void_p, C.c_int32, C.c_uint64
    L.te_last_error.restype = C.c_char_p
    L.te_abi_version.restype = C.c_int
    L.te_config_default.argtypes = [C.POINTER(K.Config), i32]
    L.te_quad_preset.argtypes = [C.POINTER(K.Config), i32]
    L.te_create.argtypes = [C.POINTER(K.Config), i32, C.POINTER(vp)]
    L.te_destroy.argtypes = [vp]
    L.te_destroy.restype = None
    L.te_reset.argtypes = [vp, vp, vp]
    L.te_observe.argtypes = [vp, vp, vp, vp, vp]
    L.te_step.argtypes = [vp] + [vp] * 10 + [vp]
    L.te_step_stacked.argtypes = [vp] + [vp] * 12 + [vp]
    L.te_observe_stacked.argtypes = [vp] + [vp] * 4 + [vp]
    L.te_step_students.argtypes = [vp] + [vp] * 8 + [vp]
    L.te_observe_ally.argtypes = [vp] + [vp] * 4 + [vp]
    L.te_set_ally_actions.argtypes = [vp, vp, vp]
    L.te_wingman_info.argtypes = [vp, vp, vp]
    L.te_calculate_rounds.argtypes = [C.c_int32, C.c_int32]
    L.te_observe_wingman.argtypes = [vp, C.c_int32] + [vp] * 4 + [vp]
    L.te_set_wingman_actions.argtypes = [vp, C.c_int32, vp, vp]
    L.te_drive_wingman.argtypes = [vp, i32, vp, i32] + [vp] * 4 + [vp]
    L.te_random_actions.argtypes = [vp, vp, u64, u64, vp]
    L.te_state_words.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.te_get_state.argtypes = [vp, vp, C.c_size_t, vp]
    L.te_set_state.argtypes = [vp, vp, C.c_size_t, vp]
    L.te_algorithmic_bytes_per_env_step.argtypes = [C.POINTER(K.Config), C.POINTER(C.c_size_t)]
    L.te_kernel_plan.argtypes = [C.POINTER(K.Config), C.c_char_p, C.c_size_t]
    L.te_debug_stamps.argtypes = [vp, C.POINTER(C.c_uint64), i32]
    L.te_profile_begin.argtypes = [vp, i32]
    L.te_set_persistent_obs.argtypes = [vp, i32]
    L.te_profile_end.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(i32)]
    L.te_policy_param_words.argtypes = [i32, C.POINTER(C.c_size_t)]
    L.te_policy_act.argtypes = [vp, i32, i32] + [vp] * 9 + [vp]
    shape = C.POINTER(PolicyShape)
    L.te_policy_shape_check.argtypes = [shape]
    L.te_policy_param_words_shaped.argtypes = [shape, C.POINTER(C.c_size_t)]
    L.te_policy_act_shaped.argtypes = [vp, shape, i32] + [vp] * 9 + [vp]
    L.te_policy_bf16_words.argtypes = [shape, C.POINTER(C.c_size_t)]
    L.te_policy_pack_bf16.argtypes = [vp, shape, vp, vp]
    L.te_policy_act_bf16.argtypes = [vp, vp, shape, i32] + [vp] * 9 + [vp]
    L.te_drive_wingman_shaped.argtypes = [vp, i32, vp, shape] + [vp] * 4 + [vp]
    L.te_drive_wingman_bf16.argtypes = [vp, i32, vp, vp, shape] + [vp] * 4 + [vp]
    L.te_policy_grad_workspace_bytes.argtypes = [i32, i32, C.POINTER(C.c_size_t)]
    f32 = C.c_float
    L.te_policy_ppo_grad.argtypes = [vp, i32, i32] + [vp] * 9 + [f32, f32, f32, vp, vp, vp, C.c_size_t, vp]
    L.te_policy_grad_workspace_bytes_shaped.argtypes = [shape, i32, C.POINTER(C.c_size_t)]
    L.te_policy_ppo_grad_shaped.argtypes = [vp, shape, i32] + [vp] * 9 + [f32, f32, f32, vp, vp, vp, C.c_size_t, vp]
    L.te_policy_bf16_grad_words.argtypes = [shape, C.POINTER(C.c_size_t)]
    L.te_policy_pack_bf16_grad.argtypes = [vp, shape, vp, vp]
    L.te_policy_grad_bf16_workspace_bytes.argtypes = [shape, i32, C.POINTER(C.c_size_t)]
    L.te_policy_ppo_grad_bf16.argtypes = [vp, vp, vp, shape, i32] + [vp] * 9 + [f32, f32, f32, vp, vp, vp, C.c_size_t, vp]
    L.te_policy_opt_state_bytes.argtypes = [C.c_size_t, C.POINTER(C.c_size_t)]
    L.te_policy_adam_step.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t] + [C.c_double] * 4 + [f32, f32, vp]
    L.te_policy_adam_step_bf16.argtypes = [vp, vp, vp, C.c_size_t, shape, vp, vp] + [C.c_double] * 4 + [f32, f32, vp]
    L.te_policy_ppo_epoch.argtypes = [C.POINTER(PpoEpochArgs), vp]
    L.te_rollout_gae.argtypes = [i32, i32] + [vp] * 4 + [C.c_double, C.c_double, vp, vp, vp]
    L.te_adv_stats_workspace_bytes.argtypes = [C.c_int64, C.POINTER(C.c_size_t)]
    L.te_adv_stats.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_size_t, vp]
    mon = [vp, C.c_size_t, i32, i32]
    L.te_monitor_bytes.argtypes = [i32, i32, C.POINTER(C.c_size_t)]
    L.te_monitor_layout.argtypes = [i32, i32, C.POINTER(MonitorOffsets)]
    L.te_monitor_init.argtypes = mon + [vp]
    L.te_monitor_step.argtypes = mon + [vp, vp, vp, vp]
    L.te_monitor_stats.argtypes = mon + [vp, i32, vp]
    L.te_sphere_encode_param_words.argtypes = [i32, C.POINTER(C.c_size_t)]
    L.te_sphere_encode.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    L.te_sphere_encode_grad_workspace_bytes.argtypes = [i32, i32, i32, C.POINTER(C.c_size_t)]
    L.te_sphere_encode_grad.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.te_sphere_bf16_words.argtypes = [i32, C.POINTER(C.c_size_t)]
    L.te_sphere_pack_bf16.argtypes = [vp, i32, vp, vp]
    L.te_sphere_encode_bf16.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
    ds = [vp, C.c_size_t, C.POINTER(DatasetGeom)]
    L.te_dataset_layout.argtypes = [C.POINTER(DatasetGeom), C.POINTER(DatasetOffsets)]
    L.te_dataset_init.argtypes = ds + [vp]
    L.te_dataset_append.argtypes = ds + [i32] + [vp] * 6 + [vp]
    L.te_dataset_gather.argtypes = ds + [i32, vp, u64, u64, i32, f32] + [vp] * 6 + [vp]
    if L.te_abi_version() != K.TE_ABI_VERSION:
        raise RuntimeError("libthreatengage.so ABI version differs from dronechase_amd.config")
    _LIB = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc:
        raise TEError(f"{what}: {load().te_last_error().decode()}")


def call(name: str, *args) -> None:
    """The ABI entry `name` with `args`; a non-zero return is a TEError that names the entry."""
    check(getattr(load(), name)(*args), name)


def call_on(device, name: str, *args) -> None:
    """call() for the entries that act on the current device and take the stream last (te_policy_*, te_rollout_gae, te_adv_stats,
    te_monitor_*, te_sphere_encode*, te_dataset_*): on `device`, on PyTorch's current stream of it."""
    import torch
    with torch.cuda.device(device):
        call(name, *args, torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def require_f32(who: str, name: str, t, shape, device, shown=None) -> None:
    """Every float array of the policy's ABI calls: contiguous float32 of `shape` on `device` (`shown`: the shape as the message spells it)."""
    import torch
    if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous float32 {shown or shape} tensor on {device}")


def require_bytes(who: str, name: str, t, shape, device):
    """A mask of the sphere encoder's and the dataset's ABI calls: contiguous uint8 or bool of `shape` on `device`; returns it as bytes."""
    import torch
    if tuple(t.shape) != tuple(shape) or t.dtype not in (torch.uint8, torch.bool) or t.device != device or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous uint8 or bool {list(shape)} tensor on {device}")
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def require_index(who: str, index, device) -> None:
    """The minibatch index of te_policy_ppo_grad and te_adv_stats: None (every row), or contiguous 1-D int64 on `device`."""
    import torch
    if index is not None and (index.dim() != 1 or index.dtype != torch.int64 or index.device != device or not index.is_contiguous()):
        raise ValueError(f"{who}: index must be a contiguous 1-D int64 tensor on {device}")


def default_config(task, **overrides) -> K.Config:
    """te_config_default(task) with keyword overrides (`quad__mass=...` reaches into te_quad_params; `quad_preset=1` swaps the
    whole quadrotor table with te_quad_preset before the other overrides apply)."""
    t = K.TASKS[task] if isinstance(task, str) else int(task)
    cfg = K.Config()
    rc = load().te_config_default(C.byref(cfg), t)
    if rc:
        raise ValueError(f"unknown task {task!r}")
    if "quad_preset" in overrides:
        if load().te_quad_preset(C.byref(cfg), int(overrides.pop("quad_preset"))):
            raise ValueError("unknown quad_preset")
    return K.apply_overrides(cfg, **overrides)


def kernel_plan(cfg: K.Config) -> dict:
    """te_kernel_plan: {role: kernel name} that te_create would launch for `cfg` under the current TE_* environment knobs (no device needed)."""
    buf = C.create_string_buffer(1024)
    check(load().te_kernel_plan(C.byref(cfg), buf, len(buf)), "te_kernel_plan")
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


def algorithmic_bytes_per_env_step(cfg: K.Config) -> int:
    out = C.c_size_t()
    check(load().te_algorithmic_bytes_per_env_step(C.byref(cfg), C.byref(out)), "te_algorithmic_bytes_per_env_step")
    return int(out.value)
