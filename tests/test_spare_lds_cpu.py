"""The spare LDS region of the latency builds (csrc/mpc_wave.hpp: CTX::kSpareLds) on the host: the solver built twice on the
host context, region off and on, must walk through bit-identical iterates.  The host build has one floating-point contraction
rule (none), so a difference here is a logic error - a cached position that is mis-indexed, read before it is written or placed
where something else lives - and not a matter of how a compiler fused a multiply-add.  Every LDS access of both builds is bounds-checked."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import BUILD_DIR, HOST_CXXFLAGS, ROOT


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(BUILD_DIR, "libcpu_wave_spare.so")
    src = os.path.join(ROOT, "tests", "cpu_wave_spare_harness.cpp")
    deps = [src, os.path.join(ROOT, "tests", "host_wave_ctx.hpp")] + \
        [os.path.join(ROOT, "mpc-rl_for_avs_amd", "csrc", f) for f in ("mpc_core.hpp", "mpc_wave.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++"] + HOST_CXXFLAGS + ["-o", out, src], check=True)
    lib = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    for f in (lib.wave_solve_batch_common, lib.wave_solve_batch_spare):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, ctypes.c_int, vp,
                      ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    lib.wave_spare_doubles.argtypes = [ctypes.c_int] * 3
    return lib


def _solve(fn, ref, inp, cc, N=20, max_iter=100, nveh=None, tol=1e-8):
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    state = np.ascontiguousarray(inp["state"], np.float64)
    B = state.shape[0]
    ego = np.ascontiguousarray(inp["ego_index"], np.int32)
    w = np.ascontiguousarray(inp["weights"], np.float64)
    c = np.ascontiguousarray(inp["is_collide"], np.uint8)
    vr = np.ascontiguousarray(inp["vref"], np.float64)
    oth = None if inp.get("others") is None else np.ascontiguousarray(inp["others"], np.float64)
    nv = None if nveh is None else np.ascontiguousarray(nveh, np.int32)
    ref = np.ascontiguousarray(ref, np.float64)
    out = dict(u0=np.zeros((B, 2)), U=np.zeros((B, N, 2)), X=np.zeros((B, N + 1, 4)), status=np.zeros(B, np.int32),
               iters=np.zeros(B, np.int32), kkt=np.zeros(B))
    rc = fn(B, N, 0.1, P(ref), ref.shape[0], P(state), P(ego), P(vr), P(w), P(c), P(oth), 0 if oth is None else oth.shape[1],
            P(nv), 1 if cc else 0, 10.0, 1.0, tol, max_iter, *(P(out[k]) for k in ("u0", "U", "X", "status", "iters", "kkt")))
    assert rc == 0
    return out


def _same(lib, ref, inp, cc, **kw):
    """Both builds on the same inputs; every output equal as bit patterns (the KKT error of a run that ends early may be inf)."""
    a = _solve(lib.wave_solve_batch_common, ref, inp, cc, **kw)
    b = _solve(lib.wave_solve_batch_spare, ref, inp, cc, **kw)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    return a


def _take(inp, idx):
    return {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


def test_the_region_is_sized_as_documented(lib):
    """Two words per vehicle and node; nothing without the collision cost, nothing without the switch (lds_doubles' default)."""
    assert lib.wave_spare_doubles(1, 20, 8) == 2 * 8 * 21
    assert lib.wave_spare_doubles(1, 16, 9) == 2 * 9 * 17
    assert lib.wave_spare_doubles(0, 20, 0) == 0
    # eight workgroups of the latency build per CU (two waves per SIMD) must fit the CU's 160 KiB at the benchmark's shape
    assert 8 * (77 * 21 + 43 + 32 + lib.wave_spare_doubles(1, 20, 8)) * 8 <= 160 * 1024


@pytest.mark.parametrize("cc", [True, False])
def test_a_batch_is_bit_identical(lib, ref_table, cc):
    from mpc_rl_for_avs_amd import synth
    inp = synth.solver_inputs(64, 8, seed=11)
    out = _same(lib, ref_table, inp, cc)
    assert ((out["status"] == 0) | (out["status"] >= 5)).mean() > 0.9 and out["iters"].max() > 20


def test_horizon_16_and_ragged_vehicle_counts(lib, ref_table):
    """P.V differs per instance while the LDS is sized for the batch's V: the region starts behind the vehicles present."""
    from mpc_rl_for_avs_amd import synth
    inp = synth.solver_inputs(24, 9, seed=12, N=16)
    nveh = np.arange(24) % 11 - 1          # -1 .. 9: below zero and at kMaxOthers of the synthetic scenes
    _same(lib, ref_table, inp, True, N=16, nveh=nveh)


@pytest.mark.parametrize("V", [0, 1])
def test_few_vehicles(lib, ref_table, V):
    from mpc_rl_for_avs_amd import synth
    inp = synth.solver_inputs(8, 8, seed=13)
    _same(lib, ref_table, inp, True, nveh=np.full(8, V))


def test_negative_cost_weights_climb_the_ladder(lib, ref_table):
    """A negative weight makes the stage cost non-convex: the sweep is retried with growing delta_w, several attempts per
    iteration, each with its own assembly phase."""
    from mpc_rl_for_avs_amd import synth
    inp = _take(synth.solver_inputs(64, 8, seed=11), np.arange(4))
    inp["weights"] = np.array([[-0.8, 0.5, -0.6], [0.7, -0.9, 0.4], [-0.3, -0.3, -0.3], [0.2, 0.9, -1.0]])
    inp["is_collide"] = np.zeros(4, np.uint8)
    out = _same(lib, ref_table, inp, True)
    assert out["iters"].min() >= 3


def test_a_wall_becomes_active(lib, ref_table):
    """A slow vehicle across the ego's path: a trial crosses d = 1, the node gets its wall constraint, and the solve ends on
    it (status 5 or 7) or keeps pressing against it - the wall terms read the cached positions in every phase."""
    from mpc_rl_for_avs_amd import synth
    base = synth.solver_inputs(64, 8, seed=11)
    found = 0
    for b in range(16):
        inp = _take(base, np.arange(b, b + 1))
        x, y, th, v = inp["state"][0]
        ahead = max(v, 2.0) * 0.8
        oth = inp["others"].copy()
        oth[0, 0] = [x + ahead * np.cos(th) + 0.3 * np.sin(th), y + ahead * np.sin(th) - 0.3 * np.cos(th), 0.2, th + 1.5]
        inp["others"] = oth
        inp["is_collide"] = np.zeros(1, np.uint8)
        out = _same(lib, ref_table, inp, True)
        found += int(out["status"][0] in (5, 7))
    assert found >= 1


def test_iteration_cap_of_three(lib, ref_table):
    from mpc_rl_for_avs_amd import synth
    inp = synth.solver_inputs(16, 8, seed=14)
    out = _same(lib, ref_table, inp, True, max_iter=3)
    assert (out["iters"] == 3).any()
