"""The device preamble (mpc_preamble.hpp: observation parsing, collision detector with memory, speed-profile rewrite)
compiled for the host, against the numpy mirror of the reference (tests/host_preamble.py, pinned by the reference's own numpy
outputs in tests/golden/reference_numpy.npz) and against those golden vectors directly.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import preamble_cases
from conftest import GOLDEN, ROOT
from test_host import CFG, Env, FakeEngine


@pytest.fixture(scope="module")
def pre():
    return load_pre()


def load_pre():
    import conftest
    out = os.path.join(conftest.BUILD_DIR, "libcpu_preamble.so")
    src = os.path.join(ROOT, "tests", "cpu_preamble_harness.cpp")
    deps = [src, os.path.join(ROOT, "tests", "host_wave_ctx.hpp")] + [os.path.join(ROOT, "mpc-rl_for_avs_amd", "csrc", f) for f in ("mpc_core.hpp", "mpc_preamble.hpp", "mpc_preamble_wave.hpp", "mpc_wave.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++"] + conftest.HOST_CXXFLAGS + ["-o", out, src], check=True)
    lib = ctypes.CDLL(out)
    lib.preamble_ego_future.restype = ctypes.c_int
    lib.preamble_ego_future.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                        ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    lib.preamble_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_double] + [ctypes.c_void_p] * 8
    lib.preamble_wave_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_double] + [ctypes.c_void_p] * 8 + [ctypes.c_int] + \
        [ctypes.c_void_p] * 3
    return lib


class DevicePreamble:
    """The harness as a stateful object: same call pattern as mpc_predict_batch up to the solve."""

    def __init__(self, lib, ref, N=20, dt=0.1, wave=False):
        """wave=False: the one-thread-per-environment form (mpc_preamble.hpp: preamble_env); wave=True: the form the HIP
        kernel runs, one wave per environment (mpc_preamble_wave.hpp), its 64 lanes emulated by loops."""
        self.lib, self.ref, self.N, self.dt, self.wave = lib, np.ascontiguousarray(ref, np.float64), N, dt, wave
        self.words = lib.preamble_env_state_ints()
        self.env = np.zeros((0, self.words), np.int32)
        self.paths = None

    def __call__(self, obs, ref_speed=None):
        B, rows = obs.shape[:2]
        if self.env.shape[0] < B:
            self.env = np.concatenate([self.env, np.zeros((B - self.env.shape[0], self.words), np.int32)])
        V = max(rows - 1, 1)
        o = dict(state=np.zeros((B, 4)), ego_index=np.zeros(B, np.int32), vref=np.zeros((B, self.N + 1)),
                 is_collide=np.zeros(B, np.uint8), others=np.zeros((B, V, 4)), nveh=np.zeros(B, np.int32))
        obs = np.ascontiguousarray(obs, np.float32)
        rs = None if ref_speed is None else np.ascontiguousarray(ref_speed, np.float64).reshape(B)
        p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        if self.wave:
            self.paths = dict(ego_path=np.zeros((B, 31, 2)), ego_len=np.zeros(B, np.int32), agent_paths=np.zeros((B, V, 31, 2), np.float32))
            rc = self.lib.preamble_wave_batch(B, p(obs), rows, p(self.ref), self.ref.shape[0], self.N, self.dt, p(rs),
                                              p(self.env), p(o["state"]), p(o["ego_index"]), p(o["vref"]), p(o["is_collide"]),
                                              p(o["others"]), p(o["nveh"]), 1, p(self.paths["ego_path"]),
                                              p(self.paths["ego_len"]), p(self.paths["agent_paths"]))
        else:
            rc = self.lib.preamble_batch(B, p(obs), rows, p(self.ref), self.ref.shape[0], self.N, self.dt, p(rs),
                                         p(self.env), p(o["state"]), p(o["ego_index"]), p(o["vref"]), p(o["is_collide"]),
                                         p(o["others"]), p(o["nveh"]))
        assert rc == 0
        o["memory"] = self.env[:B, 0].copy()
        o["conflict"] = self.env[:B, 8:24].copy()
        o["n_conflict"] = self.env[:B, 3].copy()
        o["stop_index"] = self.env[:B, 6] - 1
        return o


def host_inputs(agent, obs, ref_speed=None):
    """What the host mirror feeds the engine for the same observations (agents/pure_mpc.py:68-117)."""
    B = obs.shape[0]
    while len(agent._states) < B:
        agent._states.append(type(agent._states[0])())
    egos, others = [], []
    for b in range(B):
        e, o = agent._vehicles_from_obs(obs[b])
        agent._check_collision_env(agent._states[b], e, o)
        egos.append(e)
        others.append(o)
    rs = None if ref_speed is None else np.asarray(ref_speed, np.float64).reshape(B, 1)
    agent.collision_cost = True
    inp = agent.build_solver_inputs(agent._states[:B], egos, others, None, rs)
    inp["nveh"] = np.array([len(o) for o in others], np.int32)
    inp["memory"] = np.array([s.collision_memory for s in agent._states[:B]])
    inp["conflict"] = [[-1 if c is None else c for c in s.conflict_index] for s in agent._states[:B]]
    return inp


def test_ego_future_matches_reference_golden(pre, ref_table):
    g = np.load(os.path.join(GOLDEN, "reference_numpy.npz"))
    ref = np.ascontiguousarray(ref_table)
    for key in ("ego_future", "ego_future32"):
        if f"{key}_in" not in g.files:
            continue
        for row, want, n_want in zip(g[f"{key}_in"], g[f"{key}_out"], g[f"{key}_len"]):
            x, y, sp, vref = row
            out = np.full((31, 2), np.nan)
            if key == "ego_future":      # speed was a Python float there: the ramp ran in float64; only the cases that
                if np.float32(sp) != sp or sp < vref:    # start at or above the reference speed are type-independent
                    continue
            n = pre.preamble_ego_future(ref.ctypes.data, ref.shape[0], np.float32(x), np.float32(y), np.float32(sp),
                                        float(vref), 0.1, out.ctypes.data)
            assert n == n_want
            assert np.array_equal(out[:n], want[:n]), key


def test_stop_profile_matches_reference_golden(pre, ref_table):
    """np.linspace(ego_speed, 0, n) of agents/pure_mpc.py:712-716 in float32, through the whole preamble."""
    g = np.load(os.path.join(GOLDEN, "reference_numpy.npz"))
    dev = DevicePreamble(pre, ref_table)
    for (ego_index, conflict, speed), want in zip(g["stop_profile32_in"], g["stop_profile32_out"]):
        e, c = int(ego_index), int(conflict)
        obs = np.zeros((1, 10, 8), np.float32)
        obs[0, 0, 0] = 1
        obs[0, 0, 1:3] = ref_table[e, :2]
        obs[0, 0, 3] = np.float32(speed)                 # |v| = speed exactly
        obs[0, 0, 5] = ref_table[e, 3]
        dev.env = np.zeros((1, dev.words), np.int32)     # put the detector into its memory window with that conflict
        dev.env[0, 0] = 3
        dev.env[0, 1] = 1
        dev.env[0, 2] = 1
        dev.env[0, 24] = c
        dev.env[0, 25:40] = -1
        got = dev(obs)
        assert got["ego_index"][0] == e and got["is_collide"][0] == 1
        idx = np.minimum(e + np.arange(21), 84)
        assert np.array_equal(got["vref"][0], want[idx])


@pytest.mark.parametrize("wave", [False, True])
@pytest.mark.parametrize("V", [0, 3, 9])
def test_preamble_sequence_matches_host_mirror(pre, ref_table, V, wave):
    from mpc_rl_for_avs_amd import synth
    from host_preamble import HostPreambleAgent as PureMPC_Agent
    agent = PureMPC_Agent(Env(), dict(CFG), engine=FakeEngine())
    dev = DevicePreamble(pre, ref_table, wave=wave)
    B, T = 96, 14
    rng = np.random.default_rng(5 + V)
    n_coll = 0
    for t in range(T):
        obs = synth.make_obs_batch(B, V, seed=1000 * V + t)
        if V >= 3:
            drop = rng.uniform(size=B) < 0.3                 # some environments see fewer vehicles this step
            obs[drop, 2:, 0] = 0
        if t % 5 == 4:
            obs[:, 0, 5] += np.float32(2 * np.pi) * (rng.uniform(size=B) < 0.2)   # headings beyond pi are wrapped
        rs = rng.uniform(0, 40, B) if t == 9 else None
        want = host_inputs(agent, obs, rs)
        got = dev(obs, rs)
        assert np.array_equal(got["ego_index"], want["ego_index"])
        assert np.array_equal(got["is_collide"], want["is_collide"])
        assert np.array_equal(got["nveh"], want["nveh"])
        assert np.array_equal(got["memory"], want["memory"])
        for b in range(B):
            nc = got["n_conflict"][b]
            assert list(got["conflict"][b, :nc]) == list(want["conflict"][b]), (t, b)
        assert np.array_equal(got["state"], want["state"])
        assert np.array_equal(got["vref"], want["vref"])
        if want["others"] is not None:
            for b in range(B):
                nv = want["nveh"][b]
                assert np.array_equal(got["others"][b, :nv], want["others"][b, :nv])
        n_coll += int(want["is_collide"].sum())
        if t == 6:                                           # episode ends for a third of the environments
            ids = np.where(rng.uniform(size=B) < 0.33)[0]
            agent.reset_env_state(ids)
            dev.env[ids] = 0
    if V > 0:
        assert n_coll > B                                    # the detector actually fired


@pytest.mark.parametrize("wave", [False, True])
def test_preamble_collinear_and_degenerate_cases(pre, ref_table, wave):
    """Same-lane traffic (collinear overlap of the two paths), a stopped ego, the end of the path."""
    from host_preamble import HostPreambleAgent as PureMPC_Agent
    agent = PureMPC_Agent(Env(), dict(CFG), engine=FakeEngine())
    dev = DevicePreamble(pre, ref_table, wave=wave)
    obs = np.zeros((6, 10, 8), np.float32)
    obs[:, 0, 0] = 1
    ego = [(2.0, 45.0, 0.0, -8.0, -np.pi / 2), (2.0, 30.0, 0.0, 0.0, -np.pi / 2), (-36.2, -2.2, -9.0, 0.0, np.pi),
           (2.0, 40.0, 0.0, -5.0, -np.pi / 2), (2.0, 20.0, 0.0, -11.0, -np.pi / 2), (-20.0, -2.2, -3.0, 0.0, -3.2)]
    for b, (x, y, vx, vy, h) in enumerate(ego):
        obs[b, 0, 1:6] = (x, y, vx, vy, h)
    oth = [(2.0, 35.0, 0.0, -4.0, -np.pi / 2), (2.0, 25.0, 0.0, -6.0, -np.pi / 2), (-30.0, -2.0, -5.0, 0.0, np.pi),
           (2.0, 30.0, 0.0, 5.0, np.pi / 2), (-20.0, 2.0, 8.0, 0.0, 0.0), (-25.0, -2.2, -2.0, 0.0, np.pi)]
    for b, (x, y, vx, vy, h) in enumerate(oth):
        obs[b, 1, 0] = 1
        obs[b, 1, 1:6] = (x, y, vx, vy, h)
    for t in range(3):
        want = host_inputs(agent, obs)
        got = dev(obs)
        assert np.array_equal(got["ego_index"], want["ego_index"])
        assert np.array_equal(got["is_collide"], want["is_collide"])
        for b in range(6):
            assert list(got["conflict"][b, :got["n_conflict"][b]]) == list(want["conflict"][b]), (t, b)
        np.testing.assert_allclose(got["vref"], want["vref"], rtol=0, atol=1e-12)
        assert np.array_equal(got["state"], want["state"])
    assert want["is_collide"].sum() >= 3


def test_double_crossings_on_the_arc_are_all_candidates(pre, ref_table):
    """A straight vehicle path can cut the quarter turn of the ego path (rows 40-59 of the table) twice.  The reference
    tries every intersection point shapely returns (agents/pure_mpc.py:635-654); device code and numpy mirror enumerate
    both crossings, in the ego's direction of travel (GEOS's own order of a MultiPoint is that of a hash map and cannot
    be reproduced), and agree with each other; each candidate lies on both polylines."""
    from host_preamble import path_crossings
    ego = np.ascontiguousarray(ref_table[30:70, :2])            # straight - arc - straight
    rng = np.random.default_rng(5)
    two = 0
    for _ in range(400):
        c = np.array([-4.0, 3.0]) + rng.uniform(-3, 3, 2)       # a chord through the inside of the turn
        ang = rng.uniform(0, np.pi)
        d = np.array([np.cos(ang), np.sin(ang)])
        ag = np.stack([c + (t - 15) * 1.2 * d for t in range(31)])
        ag = np.ascontiguousarray(ag.astype(np.float32).astype(np.float64))     # predicted paths are float32 data
        want = path_crossings(ego, ag)
        out = np.zeros((4, 2))
        n = pre.preamble_path_crossings(ego.ctypes.data_as(ctypes.c_void_p), len(ego), ag.ctypes.data_as(ctypes.c_void_p),
                                        len(ag), out.ctypes.data_as(ctypes.c_void_p), 4)
        assert n == len(want)
        for q in range(n):
            assert np.allclose(out[q], want[q], rtol=0, atol=1e-12)
            # on the agent's straight line and on an ego segment
            r, dd = out[q] - ag[0], (ag[-1] - ag[0]) / np.linalg.norm(ag[-1] - ag[0])
            assert abs(r[0] * dd[1] - r[1] * dd[0]) < 1e-9
            seg = np.linalg.norm(ego[1:] - ego[:-1], axis=1)
            on = [abs(np.linalg.norm(out[q] - ego[i]) + np.linalg.norm(out[q] - ego[i + 1]) - seg[i]) < 1e-9
                  for i in range(len(ego) - 1)]
            assert any(on)
        if n == 2:
            two += 1
            # ordered along the ego path: the first candidate is met first
            first = [int(np.argmin(np.linalg.norm(ego - out[q], axis=1))) for q in range(2)]
            assert first[0] <= first[1]
    assert two >= 20
    # hand-made: the horizontal line y = 9.2 cuts the straight approach (x = 2, at row 10) and nothing else; the diagonal
    # through (2, 6.0) and (-8, -1.5) cuts the arc twice
    ag = np.stack([np.array([3.0, 6.75]) + t * np.array([-0.4, -0.3]) for t in range(31)])
    got = path_crossings(ego, ag)
    assert len(got) == 2 and got[0][1] > got[1][1]               # travelling down and then left: higher point first


def test_collinear_overlaps_stream_merge_equals_the_sorted_list(pre, ref_table):
    """Same-lane traffic: the other vehicle's predicted path lies ON the ego's (collinear overlap, what shapely returns
    as a LineString, agents/pure_mpc.py:619-622).  The device code finds the middle node of the overlap with a two-way
    merge instead of materialising and sorting the node list; the numpy mirror sorts.  Randomised: both directions of
    travel, standing vehicles, overlaps that start / end inside segments, on the approach straight and the exit straight."""
    from host_preamble import path_crossings
    rng = np.random.default_rng(11)
    n_overlap = 0
    for trial in range(600):
        lane = trial % 2
        v_ego = rng.uniform(0.5, 12.0)
        steps = np.cumsum(np.full(30, v_ego * 0.1) + rng.uniform(0, 0.02, 30))
        if lane == 0:       # approach straight x = 2, driving down
            y0 = rng.uniform(20.0, 48.0)
            ego = np.stack([np.full(31, 2.0), y0 - np.concatenate([[0.0], steps])], axis=1)
            ay0, sp, sign = rng.uniform(5.0, 50.0), rng.choice([0.0, rng.uniform(0.2, 12.0)]), rng.choice([-1.0, 1.0])
            ag = np.stack([np.full(31, 2.0), ay0 + sign * sp * 0.1 * np.arange(31)], axis=1)
        else:               # exit straight y = -2.22585..., driving in -x
            yy = float(ref_table[84, 1])
            x0 = rng.uniform(-30.0, -8.0)
            ego = np.stack([x0 - np.concatenate([[0.0], steps]), np.full(31, yy)], axis=1)
            ax0, sp, sign = rng.uniform(-45.0, -5.0), rng.choice([0.0, rng.uniform(0.2, 12.0)]), rng.choice([-1.0, 1.0])
            ag = np.stack([ax0 + sign * sp * 0.1 * np.arange(31), np.full(31, yy)], axis=1)
        ego = np.ascontiguousarray(ego)
        ag = np.ascontiguousarray(ag.astype(np.float32).astype(np.float64))
        if lane == 1:
            ego[:, 1] = ag[0, 1]         # exactly collinear with the float32 line
        want = path_crossings(ego, ag)
        out = np.zeros((4, 2))
        n = pre.preamble_path_crossings(ego.ctypes.data_as(ctypes.c_void_p), len(ego), ag.ctypes.data_as(ctypes.c_void_p),
                                        len(ag), out.ctypes.data_as(ctypes.c_void_p), 4)
        assert n == len(want), trial
        for q in range(n):
            assert np.array_equal(out[q], want[q]), (trial, q, out[q], want[q])
        n_overlap += n
    assert n_overlap >= 300


@pytest.mark.parametrize("M,rows", [(85, 10), (140, 17), (200, 17), (66, 5)])
def test_wave_form_equals_the_one_thread_form_on_long_tables_and_fast_egos(pre, M, rows):
    """Round 6 moved the wave form's serial parts into registers (arc-length sums of up to 128 segments in two registers per
    lane + one scalar, the travelled distance of step k in lane k, the observation read as one word per lane with the presence
    count as a ballot, the detector record's update spread over lanes): the cases that reach those corners - tables longer
    than one and than two words per lane, egos fast enough for the look-ahead to run past 64 and past 128 segments, the
    maximum number of observation rows (136 words), records in every phase of the collision memory - against the one-thread
    statement `preamble_env`, every output and the whole record bit for bit."""
    rng = np.random.default_rng(M * 31 + rows)
    # a straight-arc-straight route like the reference's, M points, ~0.7 m apart (so that 30 m/s x 3 s passes 128 segments)
    ref = preamble_cases.route(M)
    x, y = ref[:, 0], ref[:, 1]
    B = 96
    one, wav = DevicePreamble(pre, ref, N=20, wave=False), DevicePreamble(pre, ref, N=20, wave=True)
    for t in range(14):
        obs = np.zeros((B, rows, 8), np.float32)
        i = rng.integers(0, M, B)
        obs[:, 0, 0] = 1.0
        obs[:, 0, 1] = x[i] + rng.uniform(-0.4, 0.4, B)
        obs[:, 0, 2] = y[i] + rng.uniform(-0.4, 0.4, B)
        sp = np.where(rng.uniform(size=B) < 0.5, rng.uniform(20.0, 31.0, B), rng.uniform(0.0, 12.0, B))
        hd = ref[i, 3] + rng.uniform(-0.1, 0.1, B)
        obs[:, 0, 3], obs[:, 0, 4], obs[:, 0, 5] = sp * np.cos(hd), sp * np.sin(hd), hd
        nv = rng.integers(0, rows, B)                               # present rows are contiguous after the ego's
        for b in range(B):
            for j in range(1, nv[b] + 1):
                k = rng.integers(0, M)
                side = rng.uniform(-25.0, 25.0)
                a = ref[k, 3] + np.pi / 2 if rng.uniform() < 0.7 else ref[k, 3]        # crossing traffic, or same lane
                obs[b, j, 0] = 1.0
                obs[b, j, 1] = x[k] + side * np.cos(a)
                obs[b, j, 2] = y[k] + side * np.sin(a)
                v = rng.uniform(0.0, 12.0)
                if rng.uniform() < 0.2:                             # a crawling vehicle: its path's vertices are "the same point" to
                    v = rng.choice([0.002, 0.004, 0.0])             # np.allclose in runs (which node of a run is kept depends on the last kept)
                obs[b, j, 3], obs[b, j, 4], obs[b, j, 5] = -v * np.cos(a) * np.sign(side), -v * np.sin(a) * np.sign(side), a + (np.pi if side > 0 else 0.0)
        rs = rng.uniform(-1.0, 35.0, B) if t % 5 == 4 else None
        a_, b_ = one(obs, rs), wav(obs, rs)
        for k in ("state", "ego_index", "vref", "is_collide", "others", "nveh"):
            assert np.array_equal(a_[k], b_[k]), (t, k)
        assert np.array_equal(one.env[:B], wav.env[:B]), t          # the whole detector record, word for word
