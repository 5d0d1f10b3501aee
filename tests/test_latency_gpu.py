"""The sensing latency of the closed-loop evaluation and the compensator that knows of it, on the GPU: the mpc_delay_scene and
mpc_compensate_stale kernels against their host builds on the streams of tests/test_latency_cpu.py under that module's
yardstick (a partial group, a group past the end, a lane without a row, lane 15 with row 16; four environments of one wave
with four different look-aheads, the divergent trip count), the library's refusals, the captured evaluation step against the
eager one, and a latency of 0 against an evaluation without the stage."""
import ctypes

import numpy as np
import pytest

from test_compensate_cpu import PARAMS, assert_runs_agree
from test_compensate_gpu import _assert_same, _assert_same_traces, _dev, _eval, _pure
from test_latency_cpu import (STAGGER_AT, T_COMP, T_LAT, assert_frames_are_of_this_episode, assert_latency_runs_agree,
                              episode_starts, frame_stream, lat_class, lat_host, stale_class, stale_host, stale_stream)

pytestmark = pytest.mark.gpu

SIZES_B = [1, 3, 4, 5, 9]                                    # a partial group; either side of a full wave; two waves and a part
SIZES_R = [1, 2, 16, 17]                                     # the ego alone; one lane with a row; lane 15 without; lane 15 with row 16


@pytest.mark.parametrize("steps", [0, 1, 3, 7])
@pytest.mark.parametrize("R", SIZES_R)
@pytest.mark.parametrize("B", SIZES_B)
def test_latency_kernel_is_the_host_build(B, R, steps):
    import torch
    assert T_LAT > 16
    launches = frame_stream(B, R)
    got = lat_class(launches, B, R, steps, device=_dev(), backend="hip")
    torch.cuda.synchronize(_dev())
    assert_latency_runs_agree(got, lat_host(launches, B, R, steps), "kernel vs host build")
    assert_frames_are_of_this_episode(launches, got[0], got[1], B, steps)


@pytest.mark.parametrize("d,L", [(0, 3), (1, 2), (3, 4), (1, 6)])
@pytest.mark.parametrize("R", SIZES_R)
@pytest.mark.parametrize("B", SIZES_B)
def test_stale_kernel_is_the_host_build(B, R, d, L):
    import torch
    assert T_COMP > 16
    kw = dict(PARAMS["on"], steps=d, latency=L)               # lag, rate limit and limits on; a NaN and an infinite command
    launches = stale_stream(B, R, d, L, "on")
    assert any(np.isnan(s["command"]).any() for s in launches if "command" in s)
    got = stale_class(launches, B, R, kw, device=_dev(), backend="hip")
    torch.cuda.synchronize(_dev())
    assert_runs_agree(got, stale_host(launches, B, R, kw), "kernel vs host build", 1)


@pytest.mark.parametrize("d,L", [(0, 3), (2, 3), (1, 6)])
@pytest.mark.parametrize("B", [4, 9])
def test_stale_kernel_with_four_different_look_aheads_in_one_wave(B, d, L):
    """the divergent trip count: on launch STAGGER_AT the four environments of a wave are 0, 1, 2 and 8 launches into their
    episodes, so their rollouts take d, d + 1, d + 2 and d + 3 steps"""
    import torch
    R = 17
    kw = dict(PARAMS["on"], steps=d, latency=L)
    launches = stale_stream(B, R, d, L, "on", staggered=True)
    first = episode_starts(launches, B)
    assert (STAGGER_AT - first[STAGGER_AT][:4]).tolist() == [0, 1, 2, 8] and L >= 3
    got = stale_class(launches, B, R, kw, device=_dev(), backend="hip")
    torch.cuda.synchronize(_dev())
    assert_runs_agree(got, stale_host(launches, B, R, kw), "kernel vs host build, staggered", 1)


def test_kernels_refuse_invalid_arguments_and_launch_nothing():
    import torch
    from mpc_rl_for_avs_amd import engine
    lib = engine.load_library()
    dev = _dev()
    B, R = 4, 10
    z = lambda *sh, dt: torch.zeros(sh, dtype=dt, device=dev)
    obs, out = z(B, R, 8, dt=torch.float32), torch.full((B, R, 8), 7.0, dtype=torch.float32, device=dev)
    obs[:, 0, 0] = 1.0
    done, stale, frames = z(B, dt=torch.uint8), z(B, dt=torch.int32), z(8, B, R, 8, dt=torch.float32)
    age, counts, sums = z(B, dt=torch.int32), z(B, dt=torch.int64), z(3, B, dt=torch.float64)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def delay(B=B, R=R, reset=0, steps=2, obs=obs, done=done, out=out, stale=stale, frames=frames, age=age, counts=counts,
              sums=sums):
        return lib.mpc_delay_scene(0, B, R, reset, steps, p(obs), p(done), p(out), p(stale), p(frames), p(age), p(counts),
                                   p(sums), stream)

    for kw, word in ((dict(B=-1), b"B"), (dict(R=0), b"R"), (dict(R=18), b"R"), (dict(steps=-1), b"steps"), (dict(steps=8), b"steps"),
                     (dict(obs=None), b"obs"), (dict(out=None), b"out"), (dict(frames=None), b"frames"), (dict(age=None), b"age"),
                     (dict(counts=None), b"counts"), (dict(sums=None), b"sums"), (dict(out=obs), b"out must not be obs")):
        assert delay(**kw) == -1, kw                               # MPC_ERR_INVALID_ARG
        text = lib.mpc_last_error()
        assert b"mpc_delay_scene" in text and word in text, (kw, text)
    torch.cuda.synchronize(dev)
    assert (out == 7.0).all().item() and not age.any().item() and not counts.any().item()      # nothing was launched
    assert delay(reset=1, done=None) == 0 and delay() == 0 and delay(done=None, stale=None) == 0 and delay(B=0) == 0
    torch.cuda.synchronize(dev)
    assert age.cpu().tolist() == [3] * B and stale.cpu().tolist() == [1] * B and not (out == 7.0).any().item()

    cmd, pred = z(B, 2, dt=torch.float64), z(B, 4, dt=torch.float64)
    ring, pring, prev = z(8, B, 2, dt=torch.float64), z(8, B, 2, dt=torch.float64), z(B, 2, dt=torch.float64)
    cage, ccounts, csums = z(B, dt=torch.int32), z(B, dt=torch.int64), z(2, B, dt=torch.float64)
    out.fill_(7.0)
    inf, nan = float("inf"), float("nan")
    pair = lambda v: (ctypes.c_double * 2)(*v)

    def comp(latency=2, cmd=cmd, out=out, ring=ring, reset=0, **q):
        q = dict(dict(steps=1, dt=0.1, alpha=(1, 1), rate=(inf, inf), lo=(-inf, -inf), hi=(inf, inf)), **q)
        par = engine.CompensatorParams(struct_size=ctypes.sizeof(engine.CompensatorParams),
                                       **{k: pair(v) if isinstance(v, tuple) else v for k, v in q.items()})
        return lib.mpc_compensate_stale(0, B, R, reset, ctypes.byref(par), latency, p(obs), p(cmd), p(done), p(out), p(pred),
                                        p(ring), p(prev), p(cage), p(pring), p(ccounts), p(csums), stream)

    for kw, word in ((dict(latency=-1), b"latency"), (dict(latency=7), b"latency"), (dict(steps=4, latency=4), b"latency"),
                     (dict(steps=8, latency=0), b"steps"), (dict(dt=nan), b"dt"), (dict(alpha=(nan, 1.0)), b"alpha"),
                     (dict(cmd=None), b"command"), (dict(ring=None), b"ring"), (dict(out=obs), b"out must not be obs")):
        assert comp(**kw) == -1, kw
        text = lib.mpc_last_error()
        assert b"mpc_compensate_stale" in text and word in text, (kw, text)
    torch.cuda.synchronize(dev)
    assert (out == 7.0).all().item() and not cage.any().item()
    assert comp(reset=1, cmd=None) == 0 and comp() == 0 and comp(steps=3, latency=4) == 0 and comp(steps=0, latency=0) == 0
    torch.cuda.synchronize(dev)
    assert cage.cpu().tolist() == [3] * B and not (out == 7.0).any().item()


@pytest.fixture(scope="module")
def agent():
    return _pure()


def test_graph_and_eager_evaluations_with_latency_and_delay_are_bit_identical(agent):
    kw = dict(latency=2, actuation=dict(delay=1, tau=(0.1, 0.2)), compensation=True)
    g = _eval(agent, 64, use_graph=True, **kw)
    e = _eval(agent, 64, use_graph=False, **kw)
    _assert_same(g.records, e.records)
    _assert_same(g.drive, e.drive)
    _assert_same_traces(g.traces, e.traces)
    assert g.traces.seen.tobytes() == e.traces.seen.tobytes()
    print("compensation totals:", g.compensation, "latency totals:", g.latency)
    assert g.compensation == e.compensation and g.latency == e.latency and g.steps == e.steps
    assert g.compensation["scored"] > 0 and 0.0 < g.compensation["pos_err_max"] <= 1e-3
    assert g.latency["frames"] == 64 * (g.steps + 1) and 1.0 < g.latency["stale_mean"] < 2.0 and g.latency["ego_lag_max"] > 0.0


def test_latency_zero_is_the_evaluation_without_the_stage(agent):
    plain = _eval(agent, 64, use_graph=True, latency=None)
    res = _eval(agent, 64, use_graph=True, latency=0)
    _assert_same(res.records, plain.records)
    _assert_same(res.drive, plain.drive)
    _assert_same_traces(res.traces, plain.traces)
    assert res.steps == plain.steps and plain.latency is None
    assert res.latency["stale_mean"] == 0.0 == res.latency["ego_lag_max"] and res.latency["frames"] == 64 * (res.steps + 1)
