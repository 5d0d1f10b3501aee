"""The C-ABI shared library: it loads, exports every symbol include/mpc_mi355x.h declares, and refuses to
run without a GPU (CPU only - no compute calls here)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _header_text():
    """include/mpc_mi355x.h without its comments"""
    text = open(os.path.join(ROOT, "include", "mpc_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared_symbols():
    return sorted(set(re.findall(r"\b(mpc_[a-z_]+)\s*\(", _header_text())))


def _prototype(name):
    """[(parameter name, kind)] of `name`'s prototype in the header, kinds as engine.SIGNATURES spells them."""
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header_text())
    assert m, f"{name}: no prototype in include/mpc_mi355x.h"
    out = []
    for decl in m.group(1).split(","):
        ctype, pname = re.fullmatch(r"\s*(.*?)(\w+)\s*", decl, flags=re.S).groups()
        ctype = " ".join(ctype.replace("*", " * ").split())
        if ctype.endswith("*"):
            kind = "perception" if ctype == "const mpc_perception *" else "ptr"
        else:
            kind = {"int32_t": "i32", "uint64_t": "u64", "double": "f64"}[ctype]      # any other type: the table has no kind for it
        out.append((pname, kind))
    return out


I32, U64, F64, VP = ctypes.c_int32, ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p
_SYNTH_HEAD = [I32, I32, I32, F64, F64, U64, I32, VP, I32]


def _argtypes_before_the_table():
    """The argtypes lists load_library wrote out by hand (as counts) before SIGNATURES, element for element."""
    from mpc_rl_for_avs_amd.engine import PerceptionParams
    control = [I32] * 3 + [VP] * 10 + [U64, I32, VP] + [VP] * 5
    return dict(
        mpc_synth_env_step=_SYNTH_HEAD + [VP] * 15 + [I32, VP],
        mpc_synth_env_step_idm=_SYNTH_HEAD + [VP] * 18 + [I32, VP],
        mpc_policy_act=[I32] * 4 + [VP] * 10 + [U64, I32, VP] + [I32] * 2 + [VP] * 6,
        mpc_policy_act_sde=[I32] * 4 + [VP] * 9 + [U64, I32, VP, VP] + [I32] * 3 + [VP] * 6,
        mpc_policy_control=control,
        mpc_policy_control_tile=[I32] + control,
        mpc_rollout_record=[I32] * 6 + [VP] * 22,
        mpc_rollout_finish=[I32] * 6 + [VP] * 4 + [F64] * 2 + [VP] * 3,
        mpc_episode_stats=[I32] * 4 + [VP] * 14 + [VP],
        mpc_drive_metrics=[I32] * 6 + [F64] + [VP] * 9 + [VP],
        mpc_interaction_metrics=[I32] * 6 + [F64] + [VP] * 15 + [VP],
        mpc_perceive=[I32] * 5 + [ctypes.POINTER(PerceptionParams)] + [VP] * 6 + [VP])


def test_signature_table_is_the_header():
    """engine.SIGNATURES, which orders engine.call's named arguments, against the prototypes: the same parameter names in the
    same order, every kind the C type's, and the argtypes built from it the lists the binding had before the table."""
    from mpc_rl_for_avs_amd import engine
    before = _argtypes_before_the_table()
    assert sorted(engine.SIGNATURES) == sorted(before) and len(before) == 12
    lib = engine.load_library()
    for name, sig in engine.SIGNATURES.items():
        assert list(sig) == _prototype(name), name
        assert len({n for n, _ in sig}) == len(sig), name
        assert list(getattr(lib, name).argtypes) == before[name], name
        assert getattr(lib, name).restype is ctypes.c_int, name


class RecordingLib:
    """Stands in for the shared library: every mpc_* attribute records its positional arguments and returns `rc`."""

    def __init__(self, rc=0, error=b"the stub's text"):
        self.rc, self.error, self.calls = rc, error, []

    def mpc_last_error(self):
        return self.error

    def __getattr__(self, name):
        if not name.startswith("mpc_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return self.rc
        return entry

    def named(self, i=-1):
        """(entry point, {parameter name: argument}) of call i, by the header's order - not by engine.SIGNATURES."""
        name, args = self.calls[i]
        names = [n for n, _ in _prototype(name)]
        assert len(args) == len(names), name
        return name, dict(zip(names, args))


def address(a):
    return None if a is None else a.value


def test_call_marshals_by_name():
    import torch
    from mpc_rl_for_avs_amd import engine
    lib = RecordingLib()
    T, B = 2, 3
    row, last = torch.zeros(T * B * 85), torch.zeros(B)
    dones = torch.zeros(B, dtype=torch.bool)
    adv, ret = torch.zeros(T, B), torch.zeros(T, B)
    kw = dict(stream=None, returns=ret, advantages=adv, gae_lambda=0.95, gamma=0.99, terminal_values=None, dones=dones,
              last_values=last, row=row, keep_terminal=0, cols=85, A=1, B=B, T=T, device=0)      # in reverse on purpose
    engine.call("mpc_rollout_finish", lib=lib, **kw)
    (name, args), = lib.calls
    assert name == "mpc_rollout_finish" and args[:6] == (0, T, B, 1, 85, 0) and args[10:12] == (0.99, 0.95)
    assert [address(a) for a in args[6:10]] == [row.data_ptr(), last.data_ptr(), dones.view(torch.uint8).data_ptr(), None]
    assert args[9] is None and args[14] is None                     # None stays None, the stream's included
    assert [address(a) for a in args[12:14]] == [adv.data_ptr(), ret.data_ptr()]
    assert all(isinstance(a, ctypes.c_void_p) for a in args[6:9] + args[12:14])
    # a stream (a torch stream by its handle, or the handle itself) and the perception struct
    class Stream:
        cuda_stream = 0x1234
    p = engine.PerceptionParams(struct_size=ctypes.sizeof(engine.PerceptionParams), p_drop=0.25)
    engine.call("mpc_perceive", lib=lib, device=0, B=B, R=10, S=0, reset=1, params=p, obs_true=ret, occluders=None,
                obs_seen=row, row_class=dones, counts=last, ctr=adv, stream=Stream())
    _, d = lib.named()
    assert address(d["obs_true"]) == ret.data_ptr() and address(d["stream"]) == 0x1234 and d["occluders"] is None
    engine.call("mpc_rollout_finish", lib=lib, **dict(kw, stream=0x5678))
    assert address(lib.calls[-1][1][14]) == 0x5678
    assert ctypes.cast(d["params"], ctypes.POINTER(engine.PerceptionParams)).contents.p_drop == 0.25
    # a missing and an unknown keyword: TypeError naming the entry point and the parameter, nothing called
    lib.calls.clear()
    short = {k: v for k, v in kw.items() if k != "gamma"}
    with pytest.raises(TypeError, match=r"mpc_rollout_finish.*missing.*'gamma'"):
        engine.call("mpc_rollout_finish", lib=lib, **short)
    with pytest.raises(TypeError, match=r"mpc_rollout_finish.*unexpected.*'lam'"):
        engine.call("mpc_rollout_finish", lib=lib, lam=1.0, **kw)
    with pytest.raises(TypeError, match=r"mpc_rollout_finish.*('gamma'|'lam')"):
        engine.call("mpc_rollout_finish", lib=lib, lam=1.0, **short)
    assert lib.calls == []
    # a refusal: EngineError (a RuntimeError) with the entry point called and the library's text
    bad = RecordingLib(rc=-1, error=b"sde_epoch and sde_noise both given")
    sde = {n: None if k == "ptr" else 0 for n, k in engine.SIGNATURES["mpc_policy_act_sde"]}
    with pytest.raises(engine.EngineError, match=r"^mpc_policy_act_sde failed \(-1\): sde_epoch and sde_noise both given$"):
        engine.call("mpc_policy_act_sde", lib=bad, **sde)
    assert issubclass(engine.EngineError, RuntimeError) and [c[0] for c in bad.calls] == ["mpc_policy_act_sde"]
    with pytest.raises(engine.EngineError, match=r"^mpc_rollout_finish failed \(-1\): "):
        engine.call("mpc_rollout_finish", lib=bad, **kw)


def test_library_exports_every_declared_symbol():
    from mpc_rl_for_avs_amd import engine
    lib = engine.load_library()
    names = _declared_symbols()
    assert {"mpc_create", "mpc_destroy", "mpc_set_reference", "mpc_solve_batch", "mpc_last_error",
            "mpc_version", "mpc_default_config", "mpc_workspace_bytes"} <= set(names)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mpc_mi355x.h but not exported"
    import __graft_entry__ as g
    assert lib.mpc_version() == g.abi_version_of_header() == 8
    assert sorted(engine._EXPORTS) == names


def test_default_config_and_argument_checks():
    from mpc_rl_for_avs_amd import engine
    lib = engine.load_library()
    cfg = engine._Config()
    lib.mpc_default_config(ctypes.byref(cfg))
    assert (cfg.horizon, cfg.max_iter, cfg.device) == (20, 100, 0)
    assert cfg.dt == 0.1 and cfg.tol == 1e-8 and cfg.w_distance == 10.0 and cfg.w_collision == 1.0
    assert cfg.struct_size == ctypes.sizeof(engine._Config)
    h = ctypes.c_void_p()
    cfg.horizon = 0
    assert lib.mpc_create(ctypes.byref(cfg), ctypes.byref(h)) == -1          # MPC_ERR_INVALID_ARG
    assert b"horizon" in lib.mpc_last_error()
    cfg.horizon = 20
    cfg.struct_size = 4
    assert lib.mpc_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert lib.mpc_solve_batch(None, 1, None, None, None, None, None, None, 0, 0, None, None, None, None, None,
                               None) == -1
    # the entry points of round 4 refuse bad arguments before they touch a device
    assert lib.mpc_eval_nlp(None, 1, None, None, None, None, None, 0, 0, None, None, None, None) == -1
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mpc_rollout_finish(0, 0, 4, 1, 85, 0, p, p, p, None, 0.99, 0.95, p, p, None) == -1      # T = 0
    assert b"1 <= T" in lib.mpc_last_error()
    assert lib.mpc_rollout_finish(0, 9000, 4, 1, 85, 0, p, p, p, None, 0.99, 0.95, p, p, None) == -1   # T > 8192
    assert lib.mpc_rollout_finish(0, 8, 4, 1, 84, 0, p, p, p, None, 0.99, 0.95, p, p, None) == -1      # row layout
    assert lib.mpc_rollout_finish(0, 8, 4, 1, 85, 0, None, p, p, None, 0.99, 0.95, p, p, None) == -1   # null row
    # mpc_rollout_record(device, T, B, A, cols, keep_terminal, 21 pointers, stream): 85 = 80 + A + 4, 166 = 85 + 80 + 1 columns
    def record(T=8, B=4, A=1, cols=85, keep=0, null=()):
        names = ("row", "mpc_actions_buf", "pos_dev", "ticket", "last_obs", "last_starts", "actions", "values", "log_probs",
                 "mpc_act", "mpc_status", "new_obs", "reward", "done", "terminal_obs", "truncated", "crashed", "arrived", "counts",
                 "dones_out", "step_counter")
        assert set(null) <= set(names)
        return lib.mpc_rollout_record(0, T, B, A, cols, keep, *[None if n in null else p for n in names], None)
    assert record(T=0) == -1 and b"mpc_rollout_record: bad size" in lib.mpc_last_error()
    assert record(A=0, cols=84) == -1 and record(A=9, cols=93) == -1                                   # action_dim 1..8
    assert record(cols=84) == -1 and record(cols=86) == -1                                             # row layout, keep_terminal 0
    assert record(keep=1, cols=165) == -1 and record(keep=1, cols=167) == -1 and record(keep=1, cols=85) == -1   # ... and 1
    for name in ("row", "pos_dev", "ticket", "counts"):
        assert record(null=(name,)) == -1 and b"mpc_rollout_record: null pointer" in lib.mpc_last_error(), name
    assert record(keep=1, cols=166, null=("terminal_obs",)) == -1 and record(keep=1, cols=166, null=("truncated",)) == -1
    assert b"null pointer" in lib.mpc_last_error()
    assert record(B=0) == 0 and record(B=0, keep=1, cols=166) == 0                                     # nothing to do: no device call
    assert record(B=0, null=("terminal_obs", "truncated", "step_counter")) == 0                        # optional without keep_terminal
    assert lib.mpc_policy_act(0, 4, 0, 128, *([p] * 10), 0, 0, None, 0, 1, p, p, p, None, p, None) == -1   # action_dim 0
    assert lib.mpc_policy_act(0, 4, 3, 128, *([p] * 10), 0, 0, None, 1, 1, p, p, p, None, None, None) == -1  # v1 without weights out
    assert lib.mpc_streams_overlap(0, None, None, None) == -1                 # nowhere to put the answer


def test_sized_default_config_refuses_a_short_struct():
    """A binding that still declares an older (shorter) mpc_config is refused and NOT written to."""
    from mpc_rl_for_avs_amd import engine
    lib = engine.load_library()

    class Old(ctypes.Structure):                       # the 48-byte layout of ABI 1
        _fields_ = engine._Config._fields_[:-2]
    buf = (ctypes.c_uint8 * 64)(*([0xAB] * 64))        # the object plus what lies behind it
    old = Old.from_buffer(buf)
    rc = lib.mpc_default_config_sized(ctypes.cast(ctypes.byref(old), ctypes.POINTER(engine._Config)), ctypes.sizeof(Old))
    assert rc == -1 and b"48 bytes" in lib.mpc_last_error()
    assert bytes(buf) == b"\xab" * 64                  # untouched, in particular behind the 48 bytes
    cfg = engine._Config()
    assert lib.mpc_default_config_sized(ctypes.byref(cfg), ctypes.sizeof(cfg)) == 0
    assert cfg.struct_size == ctypes.sizeof(cfg) == 56 and cfg.ltv_passes == 1 and cfg.stall_window == 0


def test_graft_entry_build_returns():
    """The documented build command (README / INTEGRATION.md: `import __graft_entry__ as g; g.build()`) must not raise."""
    import __graft_entry__ as g
    g.build()


def test_integration_md_binding_matches_the_library():
    """The ctypes stub INTEGRATION.md tells a maintainer to paste (Option B): its `_Cfg` must have the library's
    mpc_config layout, field for field like engine._Config, and its default-config call must succeed."""
    from mpc_rl_for_avs_amd import engine, _build
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^class _Cfg\(ctypes\.Structure\):.*?\n(?=\ndef )", text, re.S | re.M)
    assert m, "INTEGRATION.md no longer holds the _Cfg snippet"
    ns = {"ctypes": ctypes}
    exec(m.group(0), ns)
    Cfg = ns["_Cfg"]
    assert [(n, t) for n, t in Cfg._fields_] == [(n, t) for n, t in engine._Config._fields_]
    lib = engine.load_library()
    cfg = Cfg()
    call = re.search(r"_lib\.(mpc_default_config\w*)\(ctypes\.byref\(cfg\)(, ctypes\.sizeof\(cfg\))?\)", text)
    assert call and call.group(1) == "mpc_default_config_sized" and call.group(2), "the stub must use the sized call"
    fn = getattr(lib, call.group(1))
    fn.argtypes = None
    assert fn(ctypes.byref(cfg), ctypes.sizeof(cfg)) == 0
    assert cfg.struct_size == ctypes.sizeof(Cfg) and cfg.horizon == 20 and cfg.ltv_passes == 1
    assert f'ctypes.CDLL("{os.path.basename(_build.LIB_PATH)}")' in text


def test_no_gpu_fails_loudly():
    """Without a HIP device the engine must raise, never fall back to a CPU path."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from mpc_rl_for_avs_amd import engine
    with pytest.raises(engine.EngineError, match="no HIP device"):
        engine.MPCEngine()
    from mpc_rl_for_avs_amd.pure_mpc import PureMPC_Agent

    class Env:
        config = {"simulation_frequency": 30, "policy_frequency": 10, "observation": {"vehicles_count": 10}}
    with pytest.raises(engine.EngineError):
        PureMPC_Agent(Env(), dict(horizon=20, render=False, weight_speed=1, weight_control=1, weight_input_diff=1))


def test_product_never_imports_oracle():
    """The shipped package must not reference the oracle (test infrastructure) anywhere."""
    pkg = os.path.join(ROOT, "mpc-rl_for_avs_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not any(w in text for w in ("oracle_lib", "nlp_spec", "mpc_oracle", "ltv_oracle")), f


def _c_client():
    """tests/abi_client.c compiled with gcc: the ABI used from plain C (dlopen, no Python objects, no torch)."""
    import subprocess
    exe = os.path.join(ROOT, "tests", "_build", "abi_client")
    src = os.path.join(ROOT, "tests", "abi_client.c")
    hdr = os.path.join(ROOT, "include", "mpc_mi355x.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-o", exe, src, "-ldl", "-lm"], check=True)
    return exe


def test_c_client_without_gpu():
    """The header compiles as C, every entry point the client binds resolves, argument errors come back as codes, and
    without a device mpc_create says MPC_ERR_NO_DEVICE (with one it succeeds)."""
    import subprocess
    from mpc_rl_for_avs_amd import _build
    _build.build()
    r = subprocess.run([_c_client(), _build.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "create rc=" in r.stdout


@pytest.mark.gpu
def test_c_client_solves_on_gpu():
    """Known answers through the ABI from plain C: NLP on the straight part of the path, state outside its bounds,
    the iterative-linear QP."""
    import subprocess
    from mpc_rl_for_avs_amd import _build
    _build.build()
    r = subprocess.run([_c_client(), _build.LIB_PATH, "solve"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "create rc=0" in r.stdout and "solve ok" in r.stdout
