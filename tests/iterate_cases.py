"""Cases, oracle ladders, the bar and the checks of the iterate-by-iterate tests (test_iterates_cpu.py, test_iterates_gpu.py).
TEST INFRASTRUCTURE, no GPU import.

An iteration cap k turns the solver into "k iterations of the algorithm".  At small caps the iterates are not yet chaotic,
so a build of the solve kernel is compared with the oracle at the same cap on EVERY instance: status, iteration count and
the whole control sequence, answers that stop at the cap (status 1) included.  The bar for the controls comes from the
oracle alone (oracle_spread, bar): how far its own iterate moves when the ego state moves by up to two units in the last
place, worst over the batch, times FACTOR."""
from collections import namedtuple

import numpy as np

CAPS = (0, 1, 2, 3, 5, 8, 13)
LONG_CAPS = (1, 3, 5, 8)          # the GPU matrix at N >= 63 (the oracle's time grows with the cube of the horizon)
B_CASE = 256
# bar = FACTOR x worst spread + FLOOR.  Kernel and oracle differ in summation order, contracted multiply-adds and hardware
# reciprocals; the builds of the kernel source need at most 31 x the worst spread (profiles/iterate_ladder.txt), an
# algorithmic error moves U by a visible fraction of a step, 1e-3 and more.
FACTOR = 256.0
FLOOR = 1e-12
U_HI = np.array([5.0, np.pi / 3])

# warm: started from given controls; infeasible: instance BAD_ROW's speed is outside its bounds (status 3, nothing to iterate);
# stall_window: mpc_config.stall_window of both sides (0 = off)
Case = namedtuple("Case", "N cc seed B warm infeasible stall_window", defaults=(B_CASE, False, False, 0))
BAD_ROW = 3


def inputs(B, N, cc, seed):
    """Synthetic solver inputs with a reference speed profile of N + 1 stages; with the collision cost on, 8 vehicles (16 at
    N = 64: the 8 synthetic ones and 8 copies shifted sideways, the largest workspace the interface allows)."""
    from mpc_rl_for_avs_amd import synth
    inp = synth.solver_inputs(B, 8, seed=seed, N=N)
    if cc and N == 64:
        far = inp["others"].copy()
        far[:, :, 0] += 7.0
        far[:, :, 1] -= 9.0
        inp["others"] = np.ascontiguousarray(np.concatenate([inp["others"], far], axis=1))
    if not cc:
        inp["others"] = None
    return inp


def case(N, cc, B=B_CASE, warm=False, infeasible=False, stall_window=0):
    return Case(N, cc, 7100 + N, B, warm, infeasible, stall_window)


_INPUTS = {}


def case_inputs(c):
    """(inp, u_init): the case's inputs, and for a warm case initial controls uniform in +-(6, 1.2) - beyond the control
    bounds (5, pi / 3) on a share of the stages, so that the clamp is part of what is compared - else None."""
    if c not in _INPUTS:
        inp = inputs(c.B, c.N, c.cc, c.seed)
        if c.infeasible:
            inp["state"][BAD_ROW, 3] = 31.0
        u = None
        if c.warm:
            u = np.random.default_rng(c.seed + 4242).uniform(-1.0, 1.0, (c.B, c.N, 2)) * [6.0, 1.2]
            assert (np.abs(u) > U_HI).any()
            u.setflags(write=False)
        _INPUTS[c] = (inp, u)
    return _INPUTS[c]


def solve_oracle(oracle, ref_table, c, cap, state=None, rows=None, **kw):
    """The oracle at iteration cap `cap` on the case's inputs (on `rows` of them; with another ego `state`)."""
    inp, u = case_inputs(c)
    sel = slice(None) if rows is None else rows
    pick = lambda a: None if a is None else np.ascontiguousarray(a[sel])
    return oracle.solve_batch(ref_table, pick(inp["state"]) if state is None else state, pick(inp["ego_index"]),
                              pick(inp["weights"]), pick(inp["is_collide"]), vref=pick(inp.get("vref")),
                              others=pick(inp.get("others")) if c.cc else None, collision_cost=c.cc, N=c.N, max_iter=cap,
                              xy_bounds=False, tol=1e-8, u_init=pick(u), stall_window=c.stall_window, **kw)


_LADDER = {}
_SPREAD = {}


def oracle_ladder(oracle, ref_table, c, cap):
    """The oracle's answer of the case at the cap, cached for the session and left unchanged."""
    key = (c, cap)
    if key not in _LADDER:
        r = solve_oracle(oracle, ref_table, c, cap)
        for a in r.values():
            a.setflags(write=False)
        _LADDER[key] = r
    return _LADDER[key]


def last_place_moved(state, rng):
    """Every component of the ego states moved by -2 .. +2 units in the last place (the loop of
    conftest.unexplained_disagreements)."""
    d = rng.integers(-2, 3, state.shape)
    st = state.copy()
    for k in range(2):
        st = np.where(d > k, np.nextafter(st, np.inf), np.where(d < -k, np.nextafter(st, -np.inf), st))
    return st


def oracle_spread(oracle, ref_table, c, cap, draws=8):
    """(worst spread, flipped), from the oracle alone: the batch's largest max|U' - U| between `draws` runs with the ego
    states moved in the last place and the unmoved run, and whether any draw changed a status or an iteration count."""
    key = (c, cap, draws)
    if key not in _SPREAD:
        inp, _ = case_inputs(c)
        base = oracle_ladder(oracle, ref_table, c, cap)
        worst, flipped = 0.0, False
        for d in range(draws):
            rng = np.random.default_rng(1000 * c.seed + 16 * cap + d)
            r = solve_oracle(oracle, ref_table, c, cap, state=last_place_moved(inp["state"], rng))
            worst = max(worst, float(np.abs(r["U"] - base["U"]).max()))
            flipped |= not (np.array_equal(r["status"], base["status"]) and np.array_equal(r["iters"], base["iters"]))
        _SPREAD[key] = (worst, flipped)
    return _SPREAD[key]


def bar(oracle, ref_table, c, cap):
    """The bar for max|dU| of the case at the cap; the oracle's own statuses and iteration counts must not move."""
    worst, flipped = oracle_spread(oracle, ref_table, c, cap)
    assert not flipped, (c, cap)
    return FACTOR * worst + FLOOR


def clear_cases():
    _INPUTS.clear()
    _LADDER.clear()
    _SPREAD.clear()


def bits_equal(a, b):
    """Equal bit for bit (float64 compared as int64: -0.0 is not 0.0, a NaN equals only itself)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64 and b.dtype == np.float64:
        a, b = a.view(np.int64), b.view(np.int64)
    return a.shape == b.shape and bool((a == b).all())


def check_capped(got, want, state, cap, bar):
    """A build's answers at iteration cap `cap` against the oracle's, for EVERY instance: status and iteration count equal;
    an answer that stopped at the cap took exactly `cap` iterations; u0 is U[:, 0] and X[:, 0] the given state, bit for bit;
    X is the model rollout of U to 1e-11 and controls and states are inside the bounds (the statements of
    test_engine_matches_oracle); at cap 0 U equals the oracle's bit for bit, above max|dU| <= bar.  An infeasible start
    (status 3 on both sides) returns its start, every node of it: U the oracle's bit for bit, X the oracle's to 1e-11 (the
    tolerance of the rollout statement: the kernel source's sines and cosines are its own polynomials, the oracle's are
    libm's, so bits differ), outside the state bounds as it is.  No instance is left out of
    anything.  Returns the batch's largest max|dU|."""
    st, it = np.asarray(got["status"]), np.asarray(got["iters"])
    B = len(st)
    bad = np.nonzero(st != want["status"])[0]
    assert bad.size == 0, ("status", cap, bad[:8], st[bad[:8]], want["status"][bad[:8]])
    bad = np.nonzero(it != want["iters"])[0]
    assert bad.size == 0, ("iters", cap, bad[:8], it[bad[:8]], want["iters"][bad[:8]])
    assert (it[st == 1] == cap).all() and (it <= cap).all(), (cap, it[st == 1])
    out = st == 3
    assert bits_equal(got["U"][out], want["U"][out]), ("infeasible start", cap)
    X, U = got["X"], got["U"]
    assert not out.any() or np.abs(X[out] - want["X"][out]).max() < 1e-11, ("infeasible start", cap)
    assert bits_equal(got["u0"], U[:, 0]), cap
    assert bits_equal(X[:, 0], np.ascontiguousarray(state, dtype=np.float64)), cap
    beta = np.arctan(0.5 * np.tan(U[:, :, 1]))
    nxt = X[:, :-1] + 0.1 * np.stack([X[:, :-1, 3] * np.cos(X[:, :-1, 2] + beta), X[:, :-1, 3] * np.sin(X[:, :-1, 2] + beta),
                                      X[:, :-1, 3] / 2.5 * np.sin(beta), U[:, :, 0]], axis=-1)
    assert np.abs(nxt - X[:, 1:]).max() < 1e-11, (cap, np.abs(nxt - X[:, 1:]).max())
    assert np.all(np.abs(U[:, :, 0]) <= 5 + 1e-7) and np.all(np.abs(U[:, :, 1]) <= np.pi / 3 + 1e-7), cap
    assert np.all(X[~out][:, :, 3] >= -1e-7) and np.all(np.abs(X[~out][:, :, 2]) <= np.pi + 1e-7), cap
    dU = np.abs(got["U"] - want["U"]).reshape(B, -1).max(axis=1)
    if cap == 0:
        assert bits_equal(got["U"], want["U"]), (cap, np.nonzero(dU > 0)[0][:8])
        return 0.0
    dU[out] = 0.0
    worst = int(np.argmax(dU))
    assert dU[worst] <= bar, (cap, worst, float(dU[worst]), bar, int((dU > bar).sum()))
    return float(dU[worst])


def line(c, build, cap, dU, worst):
    """The line every test prints: `[iterates] N cc build cap: dU, worst spread, ratio`."""
    ratio = dU / worst if worst > 0 else (0.0 if dU == 0 else np.inf)
    tags = (" warm" if c.warm else "") + (" infeasible-start" if c.infeasible else "") + \
        (f" stall_window={c.stall_window}" if c.stall_window else "") + (f" B={c.B}" if c.B != B_CASE else "")
    return (f"[iterates] N={c.N} cc={int(c.cc)}{tags} {build} cap={cap}: dU {dU:.2e}, worst spread "
            f"{worst:.2e}, ratio {ratio:.3g}")
