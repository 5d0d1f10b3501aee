"""ctypes binding of the C ABI (include/mpc_mi355x.h) - the only way Python reaches the HIP kernels: the entry points that
take an engine handle through `MPCEngine`'s methods, the handle-less ones (environment step, policy step, rollout glue,
evaluation accounting, perception, episode traces, tracker, plan metrics, actuator, delay compensation) through `call` / `caller`, by parameter
name, in the order of `SIGNATURES`, `EVALUATION_SIGNATURES`, `TRACKER_SIGNATURES`, `PLAN_SIGNATURES` and
`ACTUATION_SIGNATURES`.

There is no CPU fallback: if the shared library is missing, or no MI355X is visible, construction fails
loudly (`EngineError`).  Host numpy arrays are copied by the library; torch device tensors are passed
zero-copy as raw device pointers on the caller's stream (`solve_batch_torch`).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _build
from .reference_path import reference_states

FLAG_COLLISION_COST = 1
FLAG_DEVICE_PTRS = 2
FLAG_NO_SYNC = 4
FLAG_WARM_START = 8      # not in the reference: start from given / previous controls instead of zeros
FLAG_DETECT_ONLY = 16    # mpc_predict_batch: _check_collision alone (advance the detector records, no solve)
FLAG_DETECTED = 32       # mpc_predict_batch: _solve after such a call for the same observation
FLAG_THROUGHPUT = 64     # several batches in flight: always the build for four resident waves per SIMD
FLAG_STRICT_DISCONTINUITY = 128   # a solve that ends on the d = 1 discontinuity of the collision cost is reported unsolved (status 8)

STATUS_CONVERGED = 0
STATUS_MAX_ITER = 1
STATUS_FACTORIZATION = 2
STATUS_INFEASIBLE_START = 3
STATUS_STALLED = 4
STATUS_CONVERGED_ON_KINK = 5     # include/mpc_mi355x.h
STATUS_ACCEPTABLE = 6            # IPOPT's "Solved To Acceptable Level" (acceptable_tol 1e-6 for 15 iterations; casadi: success)
STATUS_ACCEPTABLE_ON_KINK = 7
STATUS_KINK_UNSOLVED = 8         # FLAG_STRICT_DISCONTINUITY: would be 5 or 7, counted as not solved


def converged(status):
    """Solved (MPC_STATUS_IS_SOLVED): 0; 5 on the d = 1 discontinuity of the collision cost; 6 / 7 IPOPT's acceptable level."""
    return (status == STATUS_CONVERGED) | ((status >= STATUS_CONVERGED_ON_KINK) & (status <= STATUS_ACCEPTABLE_ON_KINK))


class EngineError(RuntimeError):
    pass


class _Config(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("horizon", ctypes.c_int32), ("dt", ctypes.c_double),
                ("max_iter", ctypes.c_int32), ("device", ctypes.c_int32), ("tol", ctypes.c_double),
                ("w_distance", ctypes.c_double), ("w_collision", ctypes.c_double),
                ("ltv_passes", ctypes.c_int32), ("stall_window", ctypes.c_int32)]


class PerceptionParams(ctypes.Structure):
    """mpc_perception of include/mpc_mi355x.h (csrc/mpc_perception.hpp has the model)."""
    _fields_ = [("struct_size", ctypes.c_int32), ("occlusion", ctypes.c_int32), ("min_points", ctypes.c_int32),
                ("env_offset", ctypes.c_int32), ("range", ctypes.c_double), ("p_drop", ctypes.c_double),
                ("sigma_pos", ctypes.c_double), ("sigma_vel", ctypes.c_double), ("sigma_head", ctypes.c_double),
                ("seed", ctypes.c_uint64)]


class ActuatorParams(ctypes.Structure):
    """mpc_actuator of include/mpc_mi355x.h (csrc/mpc_actuator.hpp has the model); the per-channel fields take a pair."""
    _fields_ = [("struct_size", ctypes.c_int32), ("delay", ctypes.c_int32), ("env_offset", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("dt", ctypes.c_double), ("p_hold", ctypes.c_double)] + \
        [(name, ctypes.c_double * 2) for name in ("gain", "offset", "sigma", "alpha", "rate", "lo", "hi")] + \
        [("seed", ctypes.c_uint64)]


class CompensatorParams(ctypes.Structure):
    """mpc_compensator of include/mpc_mi355x.h (csrc/mpc_compensate.hpp has the model); the per-channel fields take a pair."""
    _fields_ = [("struct_size", ctypes.c_int32), ("steps", ctypes.c_int32), ("dt", ctypes.c_double)] + \
        [(name, ctypes.c_double * 2) for name in ("alpha", "rate", "lo", "hi")]


# The handle-less entry points: every parameter of the prototype in include/mpc_mi355x.h, in its order, as name:kind - i32
# (int32_t), u64 (uint64_t), f64 (double), ptr (any pointer, the stream included), perception (const mpc_perception *),
# actuator (const mpc_actuator *), compensator (const mpc_compensator *).
# load_library builds their argtypes from this table and `caller` orders its named arguments by it; tests/test_abi.py holds
# it against the header.
_POLICY_IN = "obs:ptr w1:ptr b1:ptr w2:ptr b2:ptr wh:ptr bh:ptr"
_POLICY_OUT = "actions:ptr values:ptr log_probs:ptr"
_SYNTH_IN = ("device:i32 B:i32 K:i32 dt:f64 spawn_probability:f64 seed:u64 env_offset:i32 ref_xy:ptr M:i32 action:ptr ego:ptr "
             "opos:ptr ospeed:ptr ohead:ptr oactive:ptr")
_SYNTH_OUT = ("t:ptr rng_counter:ptr obs:ptr terminal_obs:ptr reward:ptr done:ptr truncated:ptr crashed:ptr arrived:ptr "
              "reset_all:i32 stream:ptr")
_CONTROL = (f"device:i32 B:i32 H2:i32 {_POLICY_IN} std_:ptr c0:ptr noise:ptr noise_seed:u64 env_offset:i32 noise_step:ptr "
            f"{_POLICY_OUT} control:ptr stream:ptr")
_RECORDS = "state_i32:ptr state_f64:ptr rec_i32:ptr rec_f64:ptr"
_KINDS = dict(i32=ctypes.c_int32, u64=ctypes.c_uint64, f64=ctypes.c_double, ptr=ctypes.c_void_p,
              perception=ctypes.POINTER(PerceptionParams), actuator=ctypes.POINTER(ActuatorParams),
              compensator=ctypes.POINTER(CompensatorParams))
SIGNATURES = {name: tuple(tuple(word.split(":")) for word in text.split()) for name, text in dict(
    mpc_synth_env_step=f"{_SYNTH_IN} {_SYNTH_OUT}",
    mpc_synth_env_step_idm=f"{_SYNTH_IN} oroute:ptr oprog:ptr otarget:ptr {_SYNTH_OUT}",
    mpc_policy_act=f"device:i32 B:i32 A:i32 H2:i32 {_POLICY_IN} std_:ptr c0:ptr noise:ptr noise_seed:u64 env_offset:i32 "
                   f"noise_step:ptr version_v1:i32 clip:i32 {_POLICY_OUT} mpc_weights:ptr mpc_ref_speed:ptr stream:ptr",
    mpc_policy_act_sde=f"device:i32 B:i32 A:i32 H2:i32 {_POLICY_IN} sde_std:ptr sde_noise:ptr noise_seed:u64 env_offset:i32 "
                       f"sde_epoch:ptr sde_step:ptr sde_sample_freq:i32 version_v1:i32 clip:i32 {_POLICY_OUT} "
                       "mpc_weights:ptr mpc_ref_speed:ptr stream:ptr",
    mpc_policy_control=_CONTROL,
    mpc_policy_control_tile=f"tile:i32 {_CONTROL}",
    mpc_rollout_record="device:i32 T:i32 B:i32 A:i32 cols:i32 keep_terminal:i32 row:ptr mpc_actions_buf:ptr pos_dev:ptr "
                       "ticket:ptr last_obs:ptr last_starts:ptr actions:ptr values:ptr log_probs:ptr mpc_act:ptr "
                       "mpc_status:ptr new_obs:ptr reward:ptr done:ptr terminal_obs:ptr truncated:ptr crashed:ptr "
                       "arrived:ptr counts:ptr dones_out:ptr step_counter:ptr stream:ptr",
    mpc_rollout_finish="device:i32 T:i32 B:i32 A:i32 cols:i32 keep_terminal:i32 row:ptr last_values:ptr dones:ptr "
                       "terminal_values:ptr gamma:f64 gae_lambda:f64 advantages:ptr returns:ptr stream:ptr",
    mpc_episode_stats="device:i32 B:i32 Q:i32 reset:i32 done:ptr truncated:ptr crashed:ptr arrived:ptr reward:ptr ego:ptr "
                      f"status:ptr iters:ptr {_RECORDS} recorded:ptr step_counter:ptr stream:ptr",
    mpc_drive_metrics="device:i32 B:i32 R:i32 Q:i32 M:i32 reset:i32 dt:f64 terminal_obs:ptr obs:ptr action:ptr done:ptr "
                      f"ref_xy:ptr {_RECORDS} stream:ptr",
    mpc_interaction_metrics="device:i32 B:i32 K:i32 Q:i32 M:i32 reset:i32 dt:f64 ego:ptr opos:ptr ospeed:ptr ohead:ptr "
                            f"oactive:ptr oroute:ptr oprog:ptr otarget:ptr done:ptr ref_xy:ptr conflict:ptr {_RECORDS} "
                            "stream:ptr",
    mpc_perceive="device:i32 B:i32 R:i32 S:i32 reset:i32 params:perception obs_true:ptr occluders:ptr obs_seen:ptr "
                 "row_class:ptr counts:ptr ctr:ptr stream:ptr").items()}
# The entry points of the evaluation that came after that table: the same spelling, the same service through `caller` /
# `call`; tests/test_episode_trace_cpu.py holds this one against the header.
EVALUATION_SIGNATURES = {name: tuple(tuple(word.split(":")) for word in text.split()) for name, text in dict(
    mpc_episode_trace="device:i32 B:i32 R:i32 Q:i32 W:i32 C:i32 keep:i32 reset:i32 terminal_obs:ptr obs:ptr seen:ptr "
                      "action:ptr reward:ptr done:ptr truncated:ptr crashed:ptr arrived:ptr status:ptr iters:ptr "
                      "state_i32:ptr ring_scene:ptr ring_seen:ptr ring_act:ptr ring_reward:ptr ring_i32:ptr slot:ptr "
                      "kept_scene:ptr kept_seen:ptr kept_act:ptr kept_reward:ptr kept_i32:ptr index:ptr counts:ptr "
                      "stream:ptr").items()}
# The tracker of the evaluation (csrc/mpc_tracker.hpp), likewise; tests/test_tracker_cpu.py holds this one against the header.
TRACKER_SIGNATURES = {name: tuple(tuple(word.split(":")) for word in text.split()) for name, text in dict(
    mpc_track_rows="device:i32 B:i32 R:i32 reset:i32 dt:f64 gate:f64 coast:i32 alpha_pos:f64 alpha_vel:f64 obs_meas:ptr "
                   "done:ptr obs_out:ptr row_slot:ptr row_miss:ptr track_f64:ptr track_i32:ptr counts:ptr stream:ptr").items()}
# The plan metrics and the plan planes of the traces (csrc/mpc_plan.hpp), likewise; tests/test_plan_cpu.py holds this one against
# the header.
PLAN_SIGNATURES = {name: tuple(tuple(word.split(":")) for word in text.split()) for name, text in dict(
    mpc_plan_metrics="device:i32 B:i32 N:i32 R:i32 Q:i32 reset:i32 order:i32 dt:f64 gap:f64 lead0:i32 lead1:i32 lead2:i32 "
                     "lead3:i32 plan_X:ptr plan_U:ptr status:ptr acted:ptr terminal_obs:ptr done:ptr state_i32:ptr "
                     "state_f64:ptr ring_xy:ptr ring_valid:ptr rec_i32:ptr rec_f64:ptr stream:ptr",
    mpc_plan_trace="device:i32 B:i32 N:i32 Q:i32 W:i32 C:i32 reset:i32 plan_X:ptr plan_U:ptr done:ptr slot:ptr state_i32:ptr "
                   "ring_X:ptr ring_U:ptr kept_X:ptr kept_U:ptr stream:ptr").items()}
# The actuator model of the evaluation (csrc/mpc_actuator.hpp), likewise; tests/test_actuator_cpu.py holds this one against the
# header.
ACTUATION_SIGNATURES = {name: tuple(tuple(word.split(":")) for word in text.split()) for name, text in dict(
    mpc_actuate="device:i32 B:i32 reset:i32 params:actuator command:ptr done_prev:ptr applied:ptr state_f64:ptr age:ptr "
                "ctr:ptr counts:ptr sums:ptr stream:ptr").items()}
_TABLES = (SIGNATURES, EVALUATION_SIGNATURES, TRACKER_SIGNATURES, PLAN_SIGNATURES, ACTUATION_SIGNATURES)
# The delay compensation of the evaluation (csrc/mpc_compensate.hpp), likewise, in a table of its own beside _TABLES;
# tests/test_compensate_cpu.py holds this one against the header.
COMPENSATION_SIGNATURES = {name: tuple(tuple(word.split(":")) for word in text.split()) for name, text in dict(
    mpc_compensate="device:i32 B:i32 R:i32 reset:i32 params:compensator obs:ptr command:ptr done:ptr out:ptr pred:ptr "
                   "ring:ptr prev:ptr age:ptr pring:ptr counts:ptr sums:ptr stream:ptr").items()}
# The sensing latency of the evaluation (csrc/mpc_latency.hpp) and the compensator that knows of it, likewise, in a table of
# their own; tests/test_latency_cpu.py holds this one against the header.
LATENCY_SIGNATURES = {name: tuple(tuple(word.split(":")) for word in text.split()) for name, text in dict(
    mpc_delay_scene="device:i32 B:i32 R:i32 reset:i32 steps:i32 obs:ptr done:ptr out:ptr stale:ptr frames:ptr age:ptr "
                    "counts:ptr sums:ptr stream:ptr",
    mpc_compensate_stale="device:i32 B:i32 R:i32 reset:i32 params:compensator latency:i32 obs:ptr command:ptr done:ptr "
                         "out:ptr pred:ptr ring:ptr prev:ptr age:ptr pring:ptr counts:ptr sums:ptr stream:ptr").items()}
_ALL_TABLES = _TABLES + (COMPENSATION_SIGNATURES, LATENCY_SIGNATURES)

_EXPORTS = ["mpc_version", "mpc_last_error", "mpc_default_config", "mpc_default_config_sized", "mpc_create", "mpc_destroy",
            "mpc_set_reference", "mpc_solve_batch", "mpc_workspace_bytes", "mpc_predict_batch", "mpc_predict_batch_plan",
            "mpc_reset_env_state", "mpc_reset_env_mask", "mpc_get_env_state", "mpc_get_last_inputs", "mpc_get_launch_order",
            "mpc_ltv_solve_batch", "mpc_ltv_predict_batch", "mpc_ltv_predict_batch_plan", "mpc_env_state_bytes", "mpc_save_env_state",
            "mpc_set_env_state", "mpc_reserve_envs", "mpc_synth_env_step", "mpc_synth_env_step_idm", "mpc_set_diagnostics", "mpc_get_last_paths", "mpc_policy_act", "mpc_policy_act_sde", "mpc_policy_control", "mpc_policy_control_tile", "mpc_rollout_record", "mpc_rollout_finish", "mpc_episode_stats", "mpc_drive_metrics", "mpc_interaction_metrics", "mpc_episode_trace", "mpc_plan_metrics", "mpc_plan_trace", "mpc_perceive", "mpc_track_rows", "mpc_actuate", "mpc_compensate", "mpc_compensate_stale", "mpc_delay_scene", "mpc_eval_nlp", "mpc_streams_overlap"]
ABI_VERSION = 8          # MPC_ABI_VERSION of include/mpc_mi355x.h this binding is written for
MAX_OTHERS = 16
_lib = None


def load_library(path: str | None = None):
    """dlopen libmpc_mi355x.so (building it first when hipcc is present and the sources are newer)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    if path is None and os.environ.get("MPC_EXPERIMENT_LIB"):
        path = os.environ["MPC_EXPERIMENT_LIB"]     # development aid: an experimental build of the same ABI (tools/)
        import sys
        print(f"[mpc engine] MPC_EXPERIMENT_LIB: loading {path} instead of the in-tree library", file=sys.stderr)
    if path is None:
        path = _build.LIB_PATH
        if _build.is_stale():
            try:
                _build.build()
            except RuntimeError as e:  # no hipcc on this machine: a prebuilt .so must travel with the tree
                if not os.path.exists(path):
                    raise EngineError(f"libmpc_mi355x.so is missing and cannot be built: {e}") from e
    if not os.path.exists(path):
        raise EngineError(f"{path} not found: the MI355X engine has no fallback path")
    # PyTorch-ROCm bundles its own libamdhip64.so.7; two HIP runtimes in one process break whichever comes
    # second.  Importing torch first makes the loader resolve our NEEDED libamdhip64.so.7 to that same copy,
    # so the engine, torch tensors/streams and RCCL all share one runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    vp, dp, ip = ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p
    lib.mpc_version.restype = ctypes.c_int
    if lib.mpc_version() != ABI_VERSION:        # whichever path the library came from: argument lists below are ABI-specific
        raise EngineError(f"{path} reports ABI {lib.mpc_version()}, this binding is written for ABI {ABI_VERSION}")
    lib.mpc_last_error.restype = ctypes.c_char_p
    lib.mpc_default_config.argtypes = [ctypes.POINTER(_Config)]
    lib.mpc_default_config.restype = None
    lib.mpc_default_config_sized.argtypes = [ctypes.POINTER(_Config), ctypes.c_int32]
    lib.mpc_default_config_sized.restype = ctypes.c_int
    lib.mpc_create.argtypes = [ctypes.POINTER(_Config), ctypes.POINTER(vp)]
    lib.mpc_create.restype = ctypes.c_int
    lib.mpc_destroy.argtypes = [vp]
    lib.mpc_destroy.restype = None
    lib.mpc_set_reference.argtypes = [vp, dp, ctypes.c_int32]
    lib.mpc_set_reference.restype = ctypes.c_int
    lib.mpc_solve_batch.argtypes = [vp, ctypes.c_int32, dp, ip, dp, dp, vp, dp, ctypes.c_int32, ctypes.c_uint32,
                                    dp, dp, dp, ip, ip, vp]
    lib.mpc_solve_batch.restype = ctypes.c_int
    lib.mpc_workspace_bytes.argtypes = [vp, ctypes.c_int32, ctypes.c_int32]
    lib.mpc_workspace_bytes.restype = ctypes.c_int64
    lib.mpc_predict_batch.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int32, dp, dp, ctypes.c_uint32, dp, ip, ip, vp]
    lib.mpc_predict_batch.restype = ctypes.c_int
    lib.mpc_predict_batch_plan.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int32, dp, dp, ctypes.c_uint32, dp, dp, dp, ip, ip, vp]
    lib.mpc_predict_batch_plan.restype = ctypes.c_int
    lib.mpc_ltv_solve_batch.argtypes = [vp, ctypes.c_int32, dp, ctypes.c_uint32, dp, dp, dp, ip, ip, ip, vp]
    lib.mpc_ltv_solve_batch.restype = ctypes.c_int
    lib.mpc_ltv_predict_batch.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int32, ctypes.c_uint32, dp, ip, ip, vp]
    lib.mpc_ltv_predict_batch.restype = ctypes.c_int
    lib.mpc_ltv_predict_batch_plan.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int32, ctypes.c_uint32, dp, dp, dp, ip, ip, vp]
    lib.mpc_ltv_predict_batch_plan.restype = ctypes.c_int
    lib.mpc_reset_env_state.argtypes = [vp, ip, ctypes.c_int32, vp]
    lib.mpc_reset_env_state.restype = ctypes.c_int
    lib.mpc_reset_env_mask.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_uint32, vp]
    lib.mpc_reset_env_mask.restype = ctypes.c_int
    lib.mpc_get_env_state.argtypes = [vp, ctypes.c_int32, ip, ip, ip, ip, ip, dp]
    lib.mpc_get_env_state.restype = ctypes.c_int
    lib.mpc_env_state_bytes.argtypes = []
    lib.mpc_env_state_bytes.restype = ctypes.c_int64
    lib.mpc_save_env_state.argtypes = [vp, ctypes.c_int32, vp]
    lib.mpc_save_env_state.restype = ctypes.c_int
    lib.mpc_set_env_state.argtypes = [vp, ctypes.c_int32, vp]
    lib.mpc_set_env_state.restype = ctypes.c_int
    lib.mpc_reserve_envs.argtypes = [vp, ctypes.c_int32]
    lib.mpc_reserve_envs.restype = ctypes.c_int
    lib.mpc_get_last_inputs.argtypes = [vp, ctypes.c_int32, dp, ip, dp, vp, dp, ip]
    lib.mpc_get_last_inputs.restype = ctypes.c_int
    lib.mpc_get_launch_order.argtypes = [vp, ctypes.c_int32, ip, ip]
    lib.mpc_get_launch_order.restype = ctypes.c_int
    lib.mpc_set_diagnostics.argtypes = [vp, ctypes.c_int32]
    lib.mpc_set_diagnostics.restype = ctypes.c_int
    lib.mpc_get_last_paths.argtypes = [vp, ctypes.c_int32, dp, ip, vp]
    lib.mpc_get_last_paths.restype = ctypes.c_int
    for name, sig in [item for table in _ALL_TABLES for item in table.items()]:
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = [_KINDS[kind] for _, kind in sig], ctypes.c_int
    lib.mpc_eval_nlp.argtypes = [vp, ctypes.c_int32] + [vp] * 5 + [ctypes.c_int32, ctypes.c_uint32] + [vp] * 4
    lib.mpc_eval_nlp.restype = ctypes.c_int
    lib.mpc_streams_overlap.argtypes = [ctypes.c_int32, vp, vp, vp]
    lib.mpc_streams_overlap.restype = ctypes.c_int
    _lib = lib
    return lib


def _stream_handle(stream):
    return None if stream is None else ctypes.c_void_p(getattr(stream, "cuda_stream", stream))


def _caller(name, sig):
    """`def name(*, lib=None, <the parameters of sig>)` written out and compiled: the entry point called positionally in
    sig's order, each argument converted by its kind.  A function per entry point instead of a loop over the table because
    an eager step makes three such calls: Python binds the keywords to the names itself, and raises the TypeError that
    names the entry point and the missing or unexpected parameter."""
    convert = dict(i32="{0}", u64="{0}", f64="{0}", ptr="None if {0} is None else c_void_p({0}.data_ptr())",
                   perception="None if {0} is None else byref({0})", actuator="None if {0} is None else byref({0})",
                   compensator="None if {0} is None else byref({0})")
    args = ", ".join("_stream_handle(stream)" if n == "stream" else convert[kind].format(n) for n, kind in sig)
    scope = dict(c_void_p=ctypes.c_void_p, byref=ctypes.byref, _stream_handle=_stream_handle, EngineError=EngineError,
                 load_library=load_library)
    exec(f"def {name}(*, lib=None, {', '.join(n for n, _ in sig)}):\n"
         f"    if lib is None:\n"
         f"        lib = load_library()\n"
         f"    rc = lib.{name}({args})\n"
         f"    if rc != 0:\n"
         f"        raise EngineError(f'{name} failed ({{rc}}): {{lib.mpc_last_error().decode()}}')\n", scope)
    return scope[name]


_CALLERS = {name: _caller(name, sig) for table in _ALL_TABLES for name, sig in table.items()}


def caller(name: str):
    """The handle-less entry point `name` as a function of keywords alone: every one of SIGNATURES[name] (or
    EVALUATION_SIGNATURES[name], TRACKER_SIGNATURES[name], PLAN_SIGNATURES[name], ACTUATION_SIGNATURES[name], COMPENSATION_SIGNATURES[name], LATENCY_SIGNATURES[name]) and no other (TypeError
    naming the entry point and the parameter otherwise, before anything is called).  Python ints and floats pass through;
    a pointer is a torch tensor (its address; a bool tensor's bytes are the uint8 the kernels read) or None; `stream` is a
    torch stream, its raw handle or None; `params` of mpc_perceive a PerceptionParams, of mpc_actuate an ActuatorParams, of mpc_compensate and mpc_compensate_stale a CompensatorParams.  Enqueue only; EngineError with the
    library's text when the entry point refuses.  lib: the library, load_library() by default."""
    return _CALLERS[name]


def call(name: str, *, lib=None, **named) -> None:
    """caller(name)(lib=lib, **named).  Collecting the keywords and handing them on costs about as much again as the
    conversion itself, so what runs once per step calls caller(name) directly."""
    _CALLERS[name](lib=lib, **named)


def current_stream(device):
    """torch's current stream on a GPU `device`, which the enqueue-only calls run on; None for the CPU (no stream to name)."""
    import torch
    return torch.cuda.current_stream(device) if device.type == "cuda" else None


def perceive(device: int, B: int, R: int, S: int, reset: bool, params: dict, obs_true, occluders, obs_seen, row_class,
             counts, ctr, stream) -> None:
    """mpc_perceive on device tensors (None where optional): `params` holds the fields of mpc_perception but struct_size.  Enqueue only; EngineError with the library's text when it refuses the arguments."""
    caller("mpc_perceive")(device=device, B=B, R=R, S=S, reset=1 if reset else 0,
         params=PerceptionParams(struct_size=ctypes.sizeof(PerceptionParams), **params), obs_true=obs_true,
         occluders=occluders, obs_seen=obs_seen, row_class=row_class, counts=counts, ctr=ctr, stream=stream)


def streams_overlap(a, b, device: int = 0) -> bool:
    """True if kernels enqueued on the torch streams `a` and `b` run side by side (mpc_streams_overlap: two streams that the HIP
    runtime put on one hardware queue serialise)."""
    lib = load_library()
    out = ctypes.c_int32(-1)
    rc = lib.mpc_streams_overlap(int(device), ctypes.c_void_p(a.cuda_stream), ctypes.c_void_p(b.cuda_stream), ctypes.byref(out))
    if rc != 0:
        raise EngineError(f"mpc_streams_overlap failed ({rc}): {lib.mpc_last_error().decode()}")
    return out.value == 1


def concurrent_streams(n: int, device=0, candidates: int = 32):
    """`n` torch streams on which independent batches really are in flight together: torch hands out the streams of its pool
    round robin, the runtime spreads them over GPU_MAX_HW_QUEUES hardware queues as it sees fit, and two that share a queue
    serialise (2.6 against 3.45 M solves/s with 8 batches of 4096 in flight, tools/gpu_queues.py) - so every candidate is
    probed against the streams already chosen and kept only if it overlaps with each.  Raises if fewer than `n` of the
    `candidates` qualify (set GPU_MAX_HW_QUEUES >= n before the process touches the GPU)."""
    import torch
    dev = torch.device("cuda", device) if isinstance(device, int) else device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    chosen, seen = [], set()
    for _ in range(candidates):
        s = torch.cuda.Stream(dev)
        if s.cuda_stream in seen:
            continue
        seen.add(s.cuda_stream)
        if all(streams_overlap(s, c, idx) for c in chosen):
            chosen.append(s)
            if len(chosen) == n:
                return chosen
    raise EngineError(f"only {len(chosen)} of {len(seen)} streams run concurrently on device {idx}; "
                      f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', '(unset: 4)')}")


def _ptr(a):
    """Raw address of a numpy array (host) or a torch tensor (device); None stays None."""
    if a is None:
        return None
    return ctypes.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def _obs_array(obs):
    obs = np.ascontiguousarray(obs, dtype=np.float32)
    if obs.ndim != 3 or obs.shape[2] != 8:
        raise ValueError(f"obs must be [B, vehicles_count, 8], got {obs.shape}")
    return obs


def _host_out(key, B):
    """Host arrays an entry point fills: `key` (u0 or act) [B, 2], status [B], iters [B]."""
    return {key: np.empty((B, 2)), "status": np.empty(B, dtype=np.int32), "iters": np.empty(B, dtype=np.int32)}


def _stream(dev):
    """torch's current stream on `dev`, which the *_torch methods enqueue on."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_tensors(dev, *specs):
    """specs (name, tensor or None, dtype[, shape]): each tensor contiguous, of that dtype (and shape), on device `dev`."""
    for name, t, dt_, *shape in specs:
        if t is None:
            continue
        if t.dtype != dt_ or not t.is_contiguous() or not t.is_cuda or t.device != dev or \
                (shape and tuple(t.shape) != shape[0]):
            raise ValueError(f"{name}: expected contiguous {dt_} tensor{f' {shape[0]}' if shape else ''} on {dev}")


def _torch_out(out, key, B, dev):
    """The caller's `out`, or fresh device tensors: `key` (u0 or act) [B, 2] float64, status [B] and iters [B] int32."""
    if out is not None:
        return out
    import torch
    return {key: torch.empty((B, 2), dtype=torch.float64, device=dev),
            "status": torch.empty(B, dtype=torch.int32, device=dev), "iters": torch.empty(B, dtype=torch.int32, device=dev)}


PLAN_ORDER_NLP, PLAN_ORDER_LTV = 0, 1     # `order` of mpc_plan_metrics: x, y, theta, v / x, y, v, yaw


def _torch_plan(out, order, B, N, dev):
    """`out` with the plan's tensors: plan_U [B, N, 2] and plan_X [B, N + 1, 4] float64 (zeros at first, then reused like act)
    and plan_order."""
    import torch
    if out.get("plan_U") is None or tuple(out["plan_U"].shape) != (B, N, 2) or out["plan_U"].device != dev:
        out["plan_U"] = torch.zeros((B, N, 2), dtype=torch.float64, device=dev)
        out["plan_X"] = torch.zeros((B, N + 1, 4), dtype=torch.float64, device=dev)
    out["plan_order"] = order
    return out


class MPCEngine:
    """One engine per (process, GPU).  `solve_batch` replaces B calls of `PureMPC_Agent._solve`."""

    def __init__(self, horizon: int = 20, dt: float = 0.1, max_iter: int = 100, tol: float = 1e-8,
                 w_distance: float = 10.0, w_collision: float = 1.0, device: int = 0, ref_table=None,
                 ltv_passes: int = 1, stall_window: int = 0):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        cfg = _Config()
        # the sized variant: a _Config that no longer matches the library's mpc_config is refused, not overrun
        rc = self._lib.mpc_default_config_sized(ctypes.byref(cfg), ctypes.sizeof(cfg))
        if rc != 0:
            raise EngineError(f"mpc_default_config_sized failed ({rc}): {self._lib.mpc_last_error().decode()}")
        cfg.horizon, cfg.dt, cfg.max_iter, cfg.tol = int(horizon), float(dt), int(max_iter), float(tol)
        cfg.w_distance, cfg.w_collision, cfg.device = float(w_distance), float(w_collision), int(device)
        cfg.stall_window = int(stall_window)  # 0 = off: see include/mpc_mi355x.h
        cfg.ltv_passes = int(ltv_passes)     # iterative-linear agent only: trip count of agents/pure_mpc_linear.py:189
        rc = self._lib.mpc_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc != 0:
            self._h = ctypes.c_void_p()
            raise EngineError(f"mpc_create failed ({rc}): {self._lib.mpc_last_error().decode()}")
        self.horizon, self.dt, self.device = int(horizon), float(dt), int(device)
        self.set_reference(reference_states(dt) if ref_table is None else ref_table)

    def _check(self, rc, what):
        if rc != 0:
            raise EngineError(f"{what} failed ({rc}): {self._lib.mpc_last_error().decode()}")

    def set_reference(self, ref_table):
        ref = np.ascontiguousarray(ref_table, dtype=np.float64)
        if ref.ndim != 2 or ref.shape[1] != 4:
            raise ValueError(f"reference table must be [M, 4], got {ref.shape}")
        self.ref_table = ref
        self._check(self._lib.mpc_set_reference(self._h, _ptr(ref), ref.shape[0]), "mpc_set_reference")

    def workspace_bytes(self, B, V=0):
        """LDS bytes per workgroup for a batch of B (V > 0: collision-cost variant with V vehicles)."""
        return int(self._lib.mpc_workspace_bytes(self._h, int(B), int(V)))

    # ------------------------------------------------------------------ host (numpy) path
    def solve_batch(self, state, ego_index, weights, is_collide, vref=None, others=None, collision_cost=False,
                    want_trajectories=True, u_init=None, strict_discontinuity=False):
        """Solve B instances given host arrays; returns dict(u0, U, X, status, iters).
        u_init [B, N, 2] (optional, not in the reference): initial controls instead of the cold start.
        strict_discontinuity (MPC_FLAG_STRICT_DISCONTINUITY): a solve that ends on the d = 1 discontinuity of the collision
        cost is reported as not solved (status 8) with its last iterate, as the reference's IPOPT would report it."""
        N = self.horizon
        state = np.ascontiguousarray(state, dtype=np.float64)
        if state.ndim != 2 or state.shape[1] != 4:
            raise ValueError(f"state must be [B, 4], got {state.shape}")
        B = state.shape[0]
        ego_index = np.ascontiguousarray(ego_index, dtype=np.int32).reshape(B)
        weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(B, 3)
        is_collide = np.ascontiguousarray(is_collide, dtype=np.uint8).reshape(B)
        if vref is not None:
            vref = np.ascontiguousarray(vref, dtype=np.float64)
            if vref.shape != (B, N + 1):
                raise ValueError(f"vref must be [B, N+1] = {(B, N + 1)}, got {vref.shape}")
        V = 0
        if others is not None:
            others = np.ascontiguousarray(others, dtype=np.float64)
            if others.ndim != 3 or others.shape[0] != B or others.shape[2] != 4:
                raise ValueError(f"others must be [B, V, 4], got {others.shape}")
            V = others.shape[1]
        o = _host_out("u0", B)
        U = np.empty((B, N, 2)) if want_trajectories else None
        X = np.empty((B, N + 1, 4)) if want_trajectories else None
        flags = (FLAG_COLLISION_COST if collision_cost else 0) | (FLAG_STRICT_DISCONTINUITY if strict_discontinuity else 0)
        if u_init is not None:
            U = np.array(u_init, dtype=np.float64, order="C")       # in: initial controls, out: solution
            if U.shape != (B, N, 2):
                raise ValueError(f"u_init must be [B, N, 2] = {(B, N, 2)}, got {U.shape}")
            flags |= FLAG_WARM_START
        rc = self._lib.mpc_solve_batch(self._h, B, _ptr(state), _ptr(ego_index), _ptr(vref), _ptr(weights),
                                       _ptr(is_collide), _ptr(others), V, flags, _ptr(o["u0"]), _ptr(U), _ptr(X),
                                       _ptr(o["status"]), _ptr(o["iters"]), None)
        self._check(rc, "mpc_solve_batch")
        return dict(o, U=U, X=X)

    # ------------------------------------------------------------------ device (torch) path
    def solve_batch_torch(self, state, ego_index, weights, is_collide, vref=None, others=None,
                          collision_cost=False, out=None, sync=False, throughput=False, strict_discontinuity=False):
        """Zero-copy solve on torch CUDA(=HIP) tensors, enqueued on torch's current stream.

        dtypes: state/weights/vref/others float64, ego_index int32, is_collide uint8; all contiguous and on
        this engine's device.  Returns dict(u0, status, iters) of device tensors (reused when `out` given)."""
        import torch
        B = state.shape[0]
        dev = state.device
        _check_tensors(dev, ("state", state, torch.float64), ("ego_index", ego_index, torch.int32),
                       ("weights", weights, torch.float64), ("is_collide", is_collide, torch.uint8),
                       ("vref", vref, torch.float64), ("others", others, torch.float64))
        out = _torch_out(out, "u0", B, dev)
        V = 0 if others is None else int(others.shape[1])
        flags = FLAG_DEVICE_PTRS | (FLAG_COLLISION_COST if collision_cost else 0) | (0 if sync else FLAG_NO_SYNC) | \
            (FLAG_THROUGHPUT if throughput else 0) | \
            (FLAG_STRICT_DISCONTINUITY if strict_discontinuity else 0)     # throughput: several batches in flight (MPC_FLAG_THROUGHPUT)
        rc = self._lib.mpc_solve_batch(self._h, B, _ptr(state), _ptr(ego_index), _ptr(vref), _ptr(weights), _ptr(is_collide),
                                       _ptr(others), V, flags, _ptr(out["u0"]), _ptr(out.get("U")), _ptr(out.get("X")),
                                       _ptr(out["status"]), _ptr(out["iters"]), _stream(dev))
        self._check(rc, "mpc_solve_batch")
        return out

    # ------------------------------------------------------------------ observation-level path
    def detect_batch(self, obs):
        """`_check_collision` alone (agents/pure_mpc.py:552-676) for obs[B, vehicles_count, 8]: advances the detector
        records; `env_state` serves the result.  Follow with `predict_batch(..., detected=True)` for the same obs."""
        obs = _obs_array(obs)
        B, rows = obs.shape[:2]
        rc = self._lib.mpc_predict_batch(self._h, B, _ptr(obs), rows, None, None, FLAG_DETECT_ONLY, None, None, None, None)
        self._check(rc, "mpc_predict_batch")

    def predict_batch(self, obs, weights, ref_speed=None, collision_cost=False, warm_start=False, detected=False,
                      strict_discontinuity=False, plan=False):
        """obs[B, vehicles_count, 8] float32 -> dict(act[B, 2], status, iters): parsing, collision detector (with the
        per-environment memory kept inside the engine), speed-profile rewrite and solve, all on the device.
        warm_start (not in the reference): each environment starts from its previous solution advanced one stage.
        detected: `detect_batch` has already advanced the records for this observation.
        plan=True (mpc_predict_batch_plan): also plan_U [B, N, 2], plan_X [B, N + 1, 4] (x, y, theta, v) - the controls and
        states the solve ended with - and plan_order 0."""
        obs = _obs_array(obs)
        B, rows = obs.shape[:2]
        weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(B, 3)
        rs = None if ref_speed is None else np.ascontiguousarray(ref_speed, dtype=np.float64).reshape(B)
        o = _host_out("act", B)
        flags = (FLAG_COLLISION_COST if collision_cost else 0) | (FLAG_WARM_START if warm_start else 0) | \
            (FLAG_DETECTED if detected else 0) | (FLAG_STRICT_DISCONTINUITY if strict_discontinuity else 0)
        if plan:
            o.update(plan_U=np.zeros((B, self.horizon, 2)), plan_X=np.zeros((B, self.horizon + 1, 4)), plan_order=PLAN_ORDER_NLP)
        rc = self._lib.mpc_predict_batch_plan(self._h, B, _ptr(obs), rows, _ptr(weights), _ptr(rs), flags, _ptr(o["act"]),
                                              _ptr(o.get("plan_U")), _ptr(o.get("plan_X")), _ptr(o["status"]),
                                              _ptr(o["iters"]), None)
        self._check(rc, "mpc_predict_batch_plan")
        return o

    def predict_batch_torch(self, obs, weights, ref_speed=None, collision_cost=False, out=None, sync=False,
                            warm_start=False, throughput=False, strict_discontinuity=False, plan=False):
        """Zero-copy variant on torch device tensors (obs float32 [B, R, 8], weights float64 [B, 3], ref_speed float64
        [B] or None), enqueued on torch's current stream.  Returns dict(act, status, iters) of device tensors.
        plan=True (mpc_predict_batch_plan): `out` gains plan_U [B, N, 2], plan_X [B, N + 1, 4] (x, y, theta, v), reused
        across calls like act, and plan_order 0; plan=False is the same launches without them."""
        import torch
        B, rows = int(obs.shape[0]), int(obs.shape[1])
        dev = obs.device
        _check_tensors(dev, ("obs", obs, torch.float32), ("weights", weights, torch.float64),
                       ("ref_speed", ref_speed, torch.float64))
        if obs.dim() != 3 or obs.shape[2] != 8 or tuple(weights.shape) != (B, 3):
            raise ValueError("obs must be [B, vehicles_count, 8] and weights [B, 3]")
        out = _torch_out(out, "act", B, dev)
        flags = FLAG_DEVICE_PTRS | (FLAG_COLLISION_COST if collision_cost else 0) | (0 if sync else FLAG_NO_SYNC) | \
            (FLAG_WARM_START if warm_start else 0) | (FLAG_THROUGHPUT if throughput else 0) | \
            (FLAG_STRICT_DISCONTINUITY if strict_discontinuity else 0)   # throughput: several groups in flight
        if not plan:
            rc = self._lib.mpc_predict_batch(self._h, B, _ptr(obs), rows, _ptr(weights), _ptr(ref_speed), flags,
                                             _ptr(out["act"]), _ptr(out["status"]), _ptr(out["iters"]), _stream(dev))
            self._check(rc, "mpc_predict_batch")
            return out
        out = _torch_plan(out, PLAN_ORDER_NLP, B, self.horizon, dev)
        rc = self._lib.mpc_predict_batch_plan(self._h, B, _ptr(obs), rows, _ptr(weights), _ptr(ref_speed), flags,
                                              _ptr(out["act"]), _ptr(out["plan_U"]), _ptr(out["plan_X"]), _ptr(out["status"]),
                                              _ptr(out["iters"]), _stream(dev))
        self._check(rc, "mpc_predict_batch_plan")
        return out

    def eval_nlp(self, ego_index, weights, is_collide, X, U, vref=None, others=None, collision_cost=False):
        """Diagnostics (mpc_eval_nlp): objective f [B] and model successors x_next [B, N, 4] of the points (X [B, N+1, 4],
        U [B, N, 2]) as the solve kernel's own code evaluates them."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        U = np.ascontiguousarray(U, dtype=np.float64)
        B, N = U.shape[0], self.horizon
        if X.shape != (B, N + 1, 4) or U.shape != (B, N, 2):
            raise ValueError(f"X must be [B, {N + 1}, 4] and U [B, {N}, 2], got {X.shape} and {U.shape}")
        ego = np.ascontiguousarray(ego_index, dtype=np.int32)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        c = np.ascontiguousarray(is_collide, dtype=np.uint8)
        if ego.shape != (B,) or w.shape != (B, 3) or c.shape != (B,):
            raise ValueError("ego_index [B], weights [B, 3], is_collide [B] expected")
        vr = None if vref is None else np.ascontiguousarray(vref, dtype=np.float64)
        if vr is not None and vr.shape != (B, N + 1):
            raise ValueError(f"vref must be [B, {N + 1}]")
        oth = None if others is None else np.ascontiguousarray(others, dtype=np.float64)
        if oth is not None and (oth.ndim != 3 or oth.shape[0] != B or oth.shape[2] != 4):
            raise ValueError("others must be [B, V, 4]")
        V = 0 if oth is None else oth.shape[1]
        f, xn = np.empty(B), np.empty((B, N, 4))
        rc = self._lib.mpc_eval_nlp(self._h, B, _ptr(ego), _ptr(vr), _ptr(w), _ptr(c), _ptr(oth), V,
                                    FLAG_COLLISION_COST if collision_cost else 0, _ptr(X), _ptr(U), _ptr(f), _ptr(xn))
        self._check(rc, "mpc_eval_nlp")
        return f, xn

    # ------------------------------------------------------------------ iterative-linear MPC (pure_mpc_linear.py)
    def ltv_solve_batch(self, state, U, want_traj=False):
        """B calls of IterativeLinearMPC_Agent._solve.  state[B, 4] = x, y, v, yaw; U[B, N, 2] = stored profile (oa, od).
        Returns dict(u0, U (new profile; the old one where status != 0), status, iters, target_index[, X])."""
        state = np.ascontiguousarray(state, dtype=np.float64)
        B, N = state.shape[0], self.horizon
        if state.shape != (B, 4):
            raise ValueError(f"state must be [B, 4], got {state.shape}")
        U = np.array(U, dtype=np.float64, order="C", copy=True)
        if U.shape != (B, N, 2):
            raise ValueError(f"U must be [B, {N}, 2], got {U.shape}")
        o = _host_out("u0", B)
        X = np.empty((B, N + 1, 4)) if want_traj else None
        target = np.empty(B, dtype=np.int32)
        rc = self._lib.mpc_ltv_solve_batch(self._h, B, _ptr(state), 0, _ptr(o["u0"]), _ptr(U), _ptr(X), _ptr(o["status"]),
                                           _ptr(o["iters"]), _ptr(target), None)
        self._check(rc, "mpc_ltv_solve_batch")
        out = dict(o, U=U, target_index=target)
        if want_traj:
            out["X"] = X
        return out

    def ltv_solve_batch_torch(self, state, U, out=None, sync=False):
        """Zero-copy variant: state float64 [B, 4] and U float64 [B, N, 2] device tensors; U is updated in place.
        Returns dict(u0, status, iters) of device tensors."""
        import torch
        B, N, dev = int(state.shape[0]), self.horizon, state.device
        _check_tensors(dev, ("state", state, torch.float64, (B, 4)), ("U", U, torch.float64, (B, N, 2)))
        out = _torch_out(out, "u0", B, dev)
        rc = self._lib.mpc_ltv_solve_batch(self._h, B, _ptr(state), FLAG_DEVICE_PTRS | (0 if sync else FLAG_NO_SYNC),
                                           _ptr(out["u0"]), _ptr(U), None, _ptr(out["status"]), _ptr(out["iters"]), None,
                                           _stream(dev))
        self._check(rc, "mpc_ltv_solve_batch")
        return out

    def ltv_predict_batch(self, obs, plan=False):
        """obs[B, vehicles_count, 8] float32 -> dict(act, status, iters): Agent.predict of the iterative-linear agent
        with the per-environment stored profile kept inside the engine.  plan=True (mpc_ltv_predict_batch_plan): also plan_U
        [B, N, 2] (the stored profile after the call), plan_X [B, N + 1, 4] (x, y, v, yaw; zeros where the kernel writes none:
        an infeasible start) and plan_order 1."""
        obs = _obs_array(obs)
        B, rows = obs.shape[:2]
        o = _host_out("act", B)
        if plan:
            o.update(plan_U=np.zeros((B, self.horizon, 2)), plan_X=np.zeros((B, self.horizon + 1, 4)), plan_order=PLAN_ORDER_LTV)
        rc = self._lib.mpc_ltv_predict_batch_plan(self._h, B, _ptr(obs), rows, 0, _ptr(o["act"]), _ptr(o.get("plan_U")),
                                                  _ptr(o.get("plan_X")), _ptr(o["status"]), _ptr(o["iters"]), None)
        self._check(rc, "mpc_ltv_predict_batch_plan")
        return o

    def ltv_predict_batch_torch(self, obs, out=None, sync=False, plan=False):
        """Zero-copy variant on a float32 device tensor [B, R, 8], enqueued on torch's current stream.  plan=True
        (mpc_ltv_predict_batch_plan): `out` gains plan_U [B, N, 2], plan_X [B, N + 1, 4] (x, y, v, yaw; rows of an infeasible
        start keep what they held), reused across calls like act, and plan_order 1."""
        import torch
        if obs.dtype != torch.float32 or not obs.is_contiguous() or not obs.is_cuda or obs.dim() != 3 or obs.shape[2] != 8:
            raise ValueError("obs: expected contiguous float32 device tensor [B, vehicles_count, 8]")
        B, rows, dev = int(obs.shape[0]), int(obs.shape[1]), obs.device
        out = _torch_out(out, "act", B, dev)
        flags = FLAG_DEVICE_PTRS | (0 if sync else FLAG_NO_SYNC)
        if not plan:
            rc = self._lib.mpc_ltv_predict_batch(self._h, B, _ptr(obs), rows, flags, _ptr(out["act"]), _ptr(out["status"]),
                                                 _ptr(out["iters"]), _stream(dev))
            self._check(rc, "mpc_ltv_predict_batch")
            return out
        out = _torch_plan(out, PLAN_ORDER_LTV, B, self.horizon, dev)
        rc = self._lib.mpc_ltv_predict_batch_plan(self._h, B, _ptr(obs), rows, flags, _ptr(out["act"]), _ptr(out["plan_U"]),
                                                  _ptr(out["plan_X"]), _ptr(out["status"]), _ptr(out["iters"]), _stream(dev))
        self._check(rc, "mpc_ltv_predict_batch_plan")
        return out

    def reset_env_state(self, env_ids=None):
        """Episode boundaries: fresh detector state for the given environments (None = all)."""
        if env_ids is None:
            rc = self._lib.mpc_reset_env_state(self._h, None, -1, None)
        else:
            ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
            rc = self._lib.mpc_reset_env_state(self._h, _ptr(ids), ids.size, None)
        self._check(rc, "mpc_reset_env_state")

    def reset_env_mask_torch(self, done, warm_only=False):
        """Same from a uint8 device mask [B], enqueued on torch's current stream; warm_only: forget just the warm-start
        memory of those environments and keep their detector state."""
        import torch
        if done.dtype != torch.uint8 or not done.is_contiguous() or not done.is_cuda:
            raise ValueError("done: expected contiguous uint8 device tensor")
        rc = self._lib.mpc_reset_env_mask(self._h, int(done.numel()), _ptr(done),
                                          FLAG_DEVICE_PTRS | FLAG_NO_SYNC | (FLAG_WARM_START if warm_only else 0),
                                          _stream(done.device))
        self._check(rc, "mpc_reset_env_mask")

    def env_state(self, B):
        """Detector state of environments 0..B-1 (host copies): is_collide, ego_index, collision_memory, stop_index,
        conflict_index[B, 16] (-1 = none), conflict_points[B, 16, 2] (NaN = none)."""
        o = dict(is_collide=np.empty(B, np.int32), ego_index=np.empty(B, np.int32),
                 collision_memory=np.empty(B, np.int32), stop_index=np.empty(B, np.int32),
                 conflict_index=np.empty((B, MAX_OTHERS), np.int32), conflict_points=np.empty((B, MAX_OTHERS, 2)))
        rc = self._lib.mpc_get_env_state(self._h, B, _ptr(o["is_collide"]), _ptr(o["ego_index"]),
                                         _ptr(o["collision_memory"]), _ptr(o["stop_index"]), _ptr(o["conflict_index"]),
                                         _ptr(o["conflict_points"]))
        self._check(rc, "mpc_get_env_state")
        return o

    def save_env_state(self, B) -> np.ndarray:
        """Checkpoint of the detector records of environments 0..B-1: opaque bytes [B, record size]."""
        buf = np.zeros((B, int(self._lib.mpc_env_state_bytes())), dtype=np.uint8)
        self._check(self._lib.mpc_save_env_state(self._h, B, _ptr(buf)), "mpc_save_env_state")
        return buf

    def load_env_state(self, records: np.ndarray):
        """Put back what `save_env_state` returned (this or another engine)."""
        records = np.ascontiguousarray(records, dtype=np.uint8)
        if records.ndim != 2 or records.shape[1] != int(self._lib.mpc_env_state_bytes()):
            raise ValueError("records: expected [B, mpc_env_state_bytes()] uint8")
        self._check(self._lib.mpc_set_env_state(self._h, records.shape[0], _ptr(records)), "mpc_set_env_state")

    def reserve_envs(self, B):
        """Size the per-environment buffers now (required before capturing a step for B environments in a hipGraph)."""
        self._check(self._lib.mpc_reserve_envs(self._h, int(B)), "mpc_reserve_envs")

    def last_inputs(self, B, vehicles_count):
        """The problem data the last predict_batch derived from its observations (host copies)."""
        N, V = self.horizon, max(int(vehicles_count) - 1, 1)
        o = dict(state=np.empty((B, 4)), ego_index=np.empty(B, np.int32), vref=np.empty((B, N + 1)),
                 is_collide=np.empty(B, np.uint8), others=np.empty((B, V, 4)), nveh=np.empty(B, np.int32))
        rc = self._lib.mpc_get_last_inputs(self._h, B, _ptr(o["state"]), _ptr(o["ego_index"]), _ptr(o["vref"]),
                                           _ptr(o["is_collide"]), _ptr(o["others"]), _ptr(o["nveh"]))
        self._check(rc, "mpc_get_last_inputs")
        return o

    def launch_order(self, B):
        """Launch order of the last ordered solve of B instances (host copies): order [B] (workgroup p solved instance
        order[p]) and tier [B] (0 = the seat tier, 1..4)."""
        o = dict(order=np.empty(B, np.int32), tier=np.empty(B, np.int32))
        self._check(self._lib.mpc_get_launch_order(self._h, B, _ptr(o["order"]), _ptr(o["tier"])), "mpc_get_launch_order")
        return o

    def set_diagnostics(self, on=True):
        """Keep the detector's polylines of every following predict_batch (`last_paths`); parity tests only."""
        self._check(self._lib.mpc_set_diagnostics(self._h, 1 if on else 0), "mpc_set_diagnostics")

    def last_paths(self, B, vehicles_count):
        """Polylines of the last predict_batch: ego_path[B, 31, 2], ego_len[B] (0 where the environment replayed its
        collision memory), agent_paths[B, V, 31, 2] float32."""
        V = max(int(vehicles_count) - 1, 1)
        o = dict(ego_path=np.zeros((B, 31, 2)), ego_len=np.zeros(B, np.int32), agent_paths=np.zeros((B, V, 31, 2), np.float32))
        rc = self._lib.mpc_get_last_paths(self._h, B, _ptr(o["ego_path"]), _ptr(o["ego_len"]), _ptr(o["agent_paths"]))
        self._check(rc, "mpc_get_last_paths")
        return o

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.mpc_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
