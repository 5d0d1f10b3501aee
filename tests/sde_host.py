"""TEST INFRASTRUCTURE - the gSDE policy step of csrc/mpc_rollout_glue.hpp compiled for the host
(tests/cpu_sde_glue_harness.cpp) behind numpy wrappers, and SB3-layout checkpoints rebuilt from tests/golden/sb3_policies.npz."""
import ctypes
import io
import json
import os
import subprocess
import zipfile

import numpy as np

import conftest

_lib = None
FIXTURE = os.path.join(conftest.GOLDEN, "sb3_policies.npz")
NAMES = ("ppo_v0", "a2c_v0", "ppo_v1")


def load():
    global _lib
    if _lib is None:
        out = os.path.join(conftest.BUILD_DIR, "libcpu_sde_glue.so")
        src = os.path.join(conftest.ROOT, "tests", "cpu_sde_glue_harness.cpp")
        deps = [os.path.join(conftest.ROOT, "mpc-rl_for_avs_amd", "csrc", f) for f in ("mpc_rollout_glue.hpp", "mpc_synth_env.hpp",
                                                                                      "mpc_core.hpp")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            flags = [f for f in conftest.HOST_CXXFLAGS if f != "-ffp-contract=off"]      # fmaf is explicit in this source
            subprocess.run(["g++"] + flags + ["-o", out, src], check=True)
        _lib = ctypes.CDLL(out)
        _lib.glue_policy_act_sde.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 9 + [ctypes.c_uint64, ctypes.c_int] + \
            [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5
        _lib.glue_policy_act_sde.restype = ctypes.c_int
        _lib.glue_sde_noise.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p]
        _lib.glue_sde_noise.restype = None
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def sde_noise(seed, env, epoch, H, A, step=0, freq=-1):
    """Z [H, A] the kernel draws for environment `env` at (epoch, step, sde_sample_freq)."""
    out = np.zeros(H * A, np.float32)
    load().glue_sde_noise(int(seed) & 0xFFFFFFFFFFFFFFFF, int(env), int(epoch), int(step), int(freq), H * A, _p(out))
    return out.reshape(H, A)


def policy_act_sde(pol, obs, Z=None, version="v0", clip=True, draw=None):
    """ActorCritic(use_sde=True).act through the kernel's code: obs [B, 10, 8], Z [B, H, A] float32 numpy -> dict.
    draw = (seed, env_offset, epoch, step, freq): the kernel's own draws instead (returned as o["Z"])."""
    pol.refresh_fused()
    f = {k: np.ascontiguousarray(v.detach().cpu().numpy(), np.float32) for k, v in pol._fz.items()}
    B, A, H2 = obs.shape[0], pol.action_dim, f["b1"].size
    obs = np.ascontiguousarray(obs.reshape(B, -1), np.float32)
    Z = np.zeros((B, H2 // 2, A), np.float32) if Z is None else np.ascontiguousarray(Z, np.float32)
    o = dict(actions=np.zeros((B, A), np.float32), values=np.zeros(B, np.float32), log_probs=np.zeros(B, np.float32),
             weights=np.full((B, 3), np.nan), ref_speed=np.full(B, np.nan))
    v1 = version == "v1"
    ep = None if draw is None else np.array([draw[2]], np.int64)
    st = None if draw is None else np.array([draw[3]], np.int64)
    rc = load().glue_policy_act_sde(B, A, H2, _p(obs), _p(f["w1"]), _p(f["b1"]), _p(f["w2"]), _p(f["b2"]), _p(f["wh"]), _p(f["bh"]),
                                    _p(f["std"]), _p(Z), 0 if draw is None else int(draw[0]), 0 if draw is None else int(draw[1]),
                                    _p(ep), _p(st), -1 if draw is None else int(draw[4]), 1 if v1 else 0, 1 if clip else 0,
                                    _p(o["actions"]), _p(o["values"]), _p(o["log_probs"]), _p(o["weights"]) if v1 else None,
                                    None if v1 else _p(o["ref_speed"]))
    assert rc == 0
    o["Z"] = Z
    return o


def fixture(name):
    """(state dict of numpy arrays, data dict) of one checkpoint of the fixture."""
    d = np.load(FIXTURE)
    sd = {k.split("__", 1)[1]: d[k] for k in d.files if k.startswith(name + "__") and not k.endswith("__data")}
    return sd, json.loads(str(d[name + "__data"]))


def write_sb3_zip(path, sd, data, with_policy=True):
    """A minimal SB3-layout checkpoint: `data` (JSON) and `policy.pth` (torch.save of the state dict)."""
    import torch
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("data", json.dumps(data))
        if with_policy:
            buf = io.BytesIO()
            torch.save({k: torch.as_tensor(v) for k, v in sd.items()}, buf)
            z.writestr("policy.pth", buf.getvalue())
    return str(path)


def sb3_zip(tmp_path, name):
    sd, data = fixture(name)
    return write_sb3_zip(os.path.join(str(tmp_path), name + ".zip"), sd, data)
