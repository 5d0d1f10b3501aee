"""TEST INFRASTRUCTURE - the episode trace recorder of csrc/mpc_episode_trace.hpp compiled for the host
(tests/cpu_episode_trace_harness.cpp) behind a numpy wrapper with the layout of evaluate.EpisodeTrace, a plain-Python
restatement of the model (lists per environment, no rings, no slots), and the streams both are run on."""
import ctypes
import os
import subprocess

import numpy as np

import conftest

_lib = None
DEPS = [os.path.join(conftest.ROOT, "mpc-rl_for_avs_amd", "csrc", f) for f in ("mpc_episode_trace.hpp", "mpc_core.hpp")]
STEP_INPUTS = ("terminal_obs", "obs", "seen", "action", "reward", "done", "truncated", "crashed", "arrived", "status", "iters")
PLANES = ("state_i32", "ring_scene", "ring_seen", "ring_act", "ring_reward", "ring_i32", "slot", "kept_scene", "kept_seen",
          "kept_act", "kept_reward", "kept_i32", "index", "counts")
_DTYPES = dict(terminal_obs=np.float32, obs=np.float32, seen=np.float32, action=np.float64, reward=np.float32, done=np.uint8,
               truncated=np.uint8, crashed=np.uint8, arrived=np.uint8, status=np.int32, iters=np.int32)
COLLISION, TRUNCATED, SUCCESS, UNSOLVED, ALL = 1, 2, 4, 8, 16
STEPS = 24
# the launches (1-based) on which the episodes of environment b end: plan b % 6.  Launch 12 ends every environment; launches
# 4, 5, 7, 9, 10, 11, 14, 18, 19 and 22 end none; plan 0 has six episodes (it passes a quota of 3 and goes on); the first
# episodes are 1, 3, 8, 2, 12 and 1 steps long and the later ones include 2, 3, 8 and 9: shorter than, equal to and longer
# than every window of 1 (no episode can be shorter), 3 and 8, within a quota of 1 as within 3
PLANS = ((1, 3, 6, 12, 13, 21), (3, 12, 20), (8, 12, 24), (2, 12, 15, 16, 17), (12, 23), (1, 2, 3, 12, 20))
_UNSOLVED_STATUS, _SOLVED_STATUS = (1, 2, 3, 4, 8), (0, 5, 6, 7)


def load():
    global _lib
    if _lib is None:
        out = os.path.join(conftest.BUILD_DIR, "libcpu_episode_trace.so")
        src = os.path.join(conftest.ROOT, "tests", "cpu_episode_trace_harness.cpp")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + DEPS):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++"] + conftest.HOST_CXXFLAGS + ["-o", out, src], check=True)
        _lib = ctypes.CDLL(out)
        _lib.episode_trace_step.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 25
        _lib.episode_trace_step.restype = ctypes.c_int
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class HostTrace:
    """The recorder's buffers as numpy arrays (the layout of include/mpc_mi355x.h), stepped by the host build."""

    def __init__(self, B, R, Q, W, C, keep, seen=False):
        self.B, self.R, self.Q, self.W, self.C, self.keep, self.seen = B, R, Q, W, C, keep, seen
        self.state_i32 = np.zeros((4, B), np.int32)
        self.ring_scene = np.zeros((B, W + 1, R, 8), np.float32)
        self.ring_seen = np.zeros((B, W, R, 8), np.float32) if seen else None
        self.ring_act, self.ring_reward = np.zeros((B, W, 2), np.float64), np.zeros((B, W), np.float32)
        self.ring_i32, self.slot = np.zeros((B, W, 3), np.int32), np.zeros(B, np.int32)
        self.kept_scene = np.zeros((C, W + 1, R, 8), np.float32)
        self.kept_seen = np.zeros((C, W, R, 8), np.float32) if seen else None
        self.kept_act, self.kept_reward = np.zeros((C, W, 2), np.float64), np.zeros((C, W), np.float32)
        self.kept_i32, self.index, self.counts = np.zeros((C, W, 3), np.int32), np.zeros((C, 6), np.int32), np.zeros(4, np.int64)

    def call(self, s, reset=False, sizes=None, null=()):
        """The harness on the step dict `s` (a missing key is passed as NULL); sizes: overrides of B, R, Q, W, C, keep; null:
        names of this object's planes to pass as NULL.  Returns the harness's return value."""
        size = dict(B=self.B, R=self.R, Q=self.Q, W=self.W, C=self.C, keep=self.keep)
        size.update(sizes or {})
        ins = [None if s.get(k) is None else np.ascontiguousarray(s[k], _DTYPES[k]) for k in STEP_INPUTS]
        return load().episode_trace_step(*size.values(), 1 if reset else 0, *[_p(a) for a in ins],
                                         *[None if n in null else _p(getattr(self, n)) for n in PLANES])

    def update(self, s):
        reset = bool(s.get("reset"))
        if reset:                                            # evaluate.EpisodeTrace zeroes the store on a reset
            for n in ("kept_scene", "kept_seen", "kept_act", "kept_reward", "kept_i32", "index"):
                if getattr(self, n) is not None:
                    getattr(self, n)[:] = 0
        assert self.call(s, reset) == 0

    def planes(self):
        return {n: getattr(self, n) for n in PLANES}


def run_host(steps, B, R, Q, W, C, keep, seen=False):
    h = HostTrace(B, R, Q, W, C, keep, seen)
    for s in steps:
        h.update(s)
    return h


def solved(st):
    return st == 0 or 5 <= st <= 7


def is_selected(keep, outcome):
    return bool(keep & ALL) or (outcome & keep & 15) != 0


def replay(steps, B, Q, W, C, keep, seen=False):
    """The model as plain Python, each environment on its own: its scenes and frames as lists, an episode that ends within
    the quota and is selected put aside with the launch it ended on; at the end the selected episodes are sorted by (launch,
    environment), the first C are kept and cut to their last W steps.  `steps`: dicts of the step inputs, one with reset=True
    (and obs) where the evaluation restarts.  Returns dict(index [n, 6], counts [4], episodes: n dicts of scene [L + 1], act
    [L], reward [L], i32 [L, 3] and seen [L] or None, `all`: every episode that ended as (b, j, T, outcome, selected, launch), T and outcome None past the quota, and `idle_steps`:
    the steps environments took after their quota)."""
    chosen, every, launches, idle_steps = [], [], 0, 0
    for b in range(B):
        scenes, frames, crashed, unsolved, j, launch = [], [], False, False, 0, 0
        mine, mine_all, idle = [], [], 0
        for s in steps:
            if s.get("reset"):                               # the class zeroes the store: what was kept before is gone
                mine, mine_all, idle = [], [], 0
                scenes, frames, crashed, unsolved, j, launch = [np.array(s["obs"][b], np.float32)], [], False, False, 0, 0
                continue
            launch += 1
            if j >= Q:
                if s["done"][b]:
                    mine_all.append((b, j, None, None, False, launch))
                idle += 1
                continue
            flags = (1 if s["done"][b] else 0) | (2 if s["truncated"][b] else 0) | (4 if s["crashed"][b] else 0) | \
                (8 if s["arrived"][b] else 0)
            frames.append(dict(act=np.array(s["action"][b], np.float64), reward=np.float32(s["reward"][b]),
                               i32=np.array([s["status"][b], s["iters"][b], flags], np.int32),
                               seen=np.array(s["seen"][b], np.float32) if seen else None))
            scenes.append(np.array(s["terminal_obs"][b], np.float32))
            crashed = crashed or bool(s["crashed"][b])
            unsolved = unsolved or not solved(int(s["status"][b]))
            if s["done"][b]:
                outcome = (COLLISION if crashed else 0) | (TRUNCATED if s["truncated"][b] else 0) | \
                    (SUCCESS if s["arrived"][b] else 0) | (UNSOLVED if unsolved else 0)
                sel = is_selected(keep, outcome)
                mine_all.append((b, j, len(frames), outcome, sel, launch))
                if sel:
                    mine.append((launch, b, j, outcome, scenes, frames))
                scenes, frames, crashed, unsolved, j = [np.array(s["obs"][b], np.float32)], [], False, False, j + 1
        chosen += mine
        every += mine_all
        idle_steps += idle
        launches = launch
    chosen.sort(key=lambda e: (e[0], e[1]))
    index, episodes = [], []
    for launch, b, j, outcome, scenes, frames in chosen[:C]:
        T = len(frames)
        L = min(T, W)
        index.append([b, j, T, T - L, outcome, launch])
        episodes.append(dict(scene=np.stack(scenes[T - L:]), act=np.stack([f["act"] for f in frames[T - L:]]),
                             reward=np.array([f["reward"] for f in frames[T - L:]], np.float32),
                             i32=np.stack([f["i32"] for f in frames[T - L:]]),
                             seen=np.stack([f["seen"] for f in frames[T - L:]]) if seen else None))
    kept = min(len(chosen), C)
    return dict(index=np.array(index, np.int32).reshape(-1, 6), episodes=episodes, all=every, idle_steps=idle_steps,
                counts=np.array([len(chosen), kept, len(chosen) - kept, launches], np.int64))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_is_replay(planes, want, what):
    """index, counts and every kept plane up to each episode's L, bit for bit, against replay()'s result"""
    n = int(want["counts"][1])
    assert same_bits(np.asarray(planes["counts"]), want["counts"]), (what, planes["counts"], want["counts"])
    assert same_bits(np.asarray(planes["index"])[:n], want["index"]), (what, planes["index"][:n], want["index"])
    assert (planes["kept_seen"] is None) == (n == 0 or want["episodes"][0]["seen"] is None) or n == 0, what
    for i, ep in enumerate(want["episodes"]):
        L = ep["act"].shape[0]
        assert same_bits(planes["kept_scene"][i, :L + 1], ep["scene"]), (what, i, "scene")
        assert same_bits(planes["kept_act"][i, :L], ep["act"]), (what, i, "act")
        assert same_bits(planes["kept_reward"][i, :L], ep["reward"]), (what, i, "reward")
        assert same_bits(planes["kept_i32"][i, :L], ep["i32"]), (what, i, "i32")
        if ep["seen"] is not None:
            assert same_bits(planes["kept_seen"][i, :L], ep["seen"]), (what, i, "seen")


def assert_planes_equal(got, want, what):
    """every plane of the recorder, bit for bit (rings, work array and running state included)"""
    for n in PLANES:
        assert (got[n] is None) == (want[n] is None), (what, n)
        if want[n] is not None:
            assert same_bits(np.asarray(got[n]), want[n]), (what, n)


def random_stream(B, R, Q, W, C, keep, seed, seen=False):
    """A reset and STEPS steps of B environments whose episodes end by PLANS.  Within the quota, the first episode of an
    environment with plan p < 4 has every outcome bit but bit p, that of plans 4 and 5 has all four: under every single bit
    of `keep` five of any six neighbouring environments are selected and one is not.  Later episodes draw their outcome.  A
    crash and an unsolved solve fall on a random step of their episode, not only on the last.  Scenes, actions and rewards
    are random bits of their formats; obs repeats terminal_obs where the episode goes on and is fresh where it ended.
    Q, W, C and keep do not enter: the same stream serves every setting of the recorder."""
    rng = np.random.default_rng(seed)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    crashed, truncated, arrived = (np.zeros((STEPS, B), np.uint8) for _ in range(3))
    done = np.zeros((STEPS, B), np.uint8)
    status = rng.choice(_SOLVED_STATUS, size=(STEPS, B)).astype(np.int32)
    for b in range(B):
        p = b % len(PLANS)
        ends = PLANS[p] + (STEPS + 1,)                       # the last, unfinished episode
        start = 1
        for n, end in enumerate(ends):
            last = min(end, STEPS)
            if start > last:
                break
            bits = (15 & ~(1 << p) if p < 4 else 15) if n == 0 else int(rng.integers(0, 16))
            if bits & COLLISION:
                crashed[rng.integers(start, last + 1) - 1, b] = 1
            if bits & UNSOLVED:
                status[rng.integers(start, last + 1) - 1, b] = rng.choice(_UNSOLVED_STATUS)
            if end <= STEPS:
                done[end - 1, b] = 1
                truncated[end - 1, b] = 1 if bits & TRUNCATED else 0
                arrived[end - 1, b] = 1 if bits & SUCCESS else 0
            start = end + 1
    steps = [dict(reset=True, obs=f32(B, R, 8))]
    for t in range(STEPS):
        terminal = f32(B, R, 8)
        obs = np.where(done[t][:, None, None] != 0, f32(B, R, 8), terminal)
        steps.append(dict(terminal_obs=terminal, obs=obs, seen=f32(B, R, 8) if seen else None, action=rng.standard_normal((B, 2)),
                          reward=f32(B), done=done[t], truncated=truncated[t], crashed=crashed[t], arrived=arrived[t],
                          status=status[t], iters=rng.integers(0, 100, B).astype(np.int32)))
    return steps
