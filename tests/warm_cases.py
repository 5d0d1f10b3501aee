"""Cases, bars and the host model of the warm-start tests (test_warm_start_cpu.py, test_warm_start_gpu.py).  No GPU import.

MPC_FLAG_WARM_START replaces the cold start of a solve by given controls.  mpc_solve_batch reads them from U as they are
(u_shift 0, no u_valid); mpc_predict_batch reads the handle's own memory d_warm[b] advanced one stage (u_shift 1, last stage
repeated) where d_warm_valid[b] says that it holds a solution of the current episode, and writes both after the solve.  This
module builds the initial controls the solve-entry tests share (warm_inputs), states the two conditions those inputs must meet
for the tests to see a fault (warm_changes_iterations, sensitivity), derives the equal-iteration bar from the oracle alone
(iters_bar), restates conftest.unexplained_disagreements with each instance's own initial controls, and models the
per-environment memory on the host (WarmMemory, expected_step)."""
import numpy as np

from conftest import converged, rel_u0_err
from test_solve_builds_gpu import _bars, _inputs, _nlp, _oracle  # noqa: F401  (the cold matrix's builders, re-exported)

U_LO = np.array([-5.0, -np.pi / 3])
U_HI = -U_LO

CPU_N = (1, 2, 16, 20, 31, 32, 33, 63, 64)
COMPILED_N = (16, 20)
RUNTIME_N = (1, 2, 31, 32, 33, 63, 64)


def batch_of(N):
    """Batch of the host-side cases: 256, and 96 from N = 63 (the oracle's time grows with the cube of the horizon)."""
    return 256 if N < 63 else 96


def seed_of(N, cc):
    """The seeds of the cold build matrix (test_solve_builds_gpu.py), whose inputs the oracle's own cold answers certify on;
    oracle_certifies() states the same of the warm answers."""
    return 7100 + N + (50 if cc else 0) if N in COMPILED_N else 7300 + N + (100 if cc else 0)


def advance(U):
    """A control sequence advanced one stage, the last stage repeated: what u_shift = 1 reads, min(k + 1, N - 1)."""
    return np.concatenate([U[:, 1:], U[:, -1:]], axis=1)


def warm_oracle(oracle, ref_table, inp, cc, N, u_init, state=None, max_iter=100):
    return oracle.solve_batch(ref_table, inp["state"] if state is None else state, inp["ego_index"], inp["weights"],
                              inp["is_collide"], vref=inp.get("vref"), others=inp.get("others") if cc else None,
                              collision_cost=cc, N=N, max_iter=max_iter, xy_bounds=False, u_init=u_init)


NAN_ROWS = slice(5, None, 24)

_CASES = {}


def warm_inputs(oracle, ref_table, N, cc, seed, B):
    """(inp, u_init, cold): the inputs and the oracle's cold answer as the cold build matrix makes them, and initial controls
    [B, N, 2]: the cold solution advanced one stage; rows 1::3 uniform inside the control bounds; rows 2::12 uniform in
    [-8, 8] (clamped; some leave the state bounds in the rollout and fall back to the cold start); rows 5::24 NaN (fmax / fmin
    semantics on both sides: the clamped lower bound).  Later strides win.  Cached: shared by the tests of a session."""
    key = (N, cc, seed, B)
    if key not in _CASES:
        inp = _inputs(B, N, cc, seed)
        cold = _oracle(oracle, ref_table, inp, cc, N)
        rng = np.random.default_rng(seed + 31337)
        u = advance(cold["U"])
        u[1::3] = rng.uniform(U_LO, U_HI, u[1::3].shape)
        u[2::12] = rng.uniform(-8.0, 8.0, u[2::12].shape)
        u[NAN_ROWS] = np.nan
        u.setflags(write=False)
        _CASES[key] = (inp, u, cold)
    return _CASES[key]


_WARM = {}


def warm_case(oracle, ref_table, N, cc, B):
    """warm_inputs at the case's own seed, and the oracle's warm answer: (inp, u_init, cold, want)."""
    key = (N, cc, B)
    if key not in _WARM:
        inp, u, cold = warm_inputs(oracle, ref_table, N, cc, seed_of(N, cc), B)
        _WARM[key] = (inp, u, cold, warm_oracle(oracle, ref_table, inp, cc, N, u))
    return _WARM[key]


def clear_cases():
    _CASES.clear()
    _WARM.clear()


# ------------------------------------------------------------------------------------- conditions on the inputs, bars
def warm_changes_iterations(cold, want, N):
    """Condition on the inputs: the share of instances on which the oracle's warm iteration count differs from its cold one,
    asserted at >= 0.30 for N = 1 and >= 0.45 elsewhere (a kernel that ignored its initial controls would then miss the
    equal-iteration bar by a wide margin)."""
    share = float((cold["iters"] != want["iters"]).mean())
    assert share >= (0.30 if N == 1 else 0.45), (N, share)
    return share


def oracle_certifies(ref_table, inp, cc, N, want):
    """Condition on the inputs: the ORACLE's own warm answers pass the certificate gate the builds are held to (an
    instance with hundreds of active bounds can end at 1.0x - 1.1x tol in the certificate's IPOPT-units measure whoever
    solves it, cold or warm - seen at N = 32 with another draw; such a draw cannot test a build)."""
    from solve_gates import certify_converged
    long = N >= 63
    certify_converged(_nlp(ref_table, inp, cc, N), want["status"], want["X"], want["U"],
                      kink_wall_tol=1e-4 if long else None, ipopt_factor=10.0 if long else 1.0)


def ulp_moved(state, draw):
    """The ego states moved by one unit in the last place, each component up or down by the draw's own coin."""
    rng = np.random.default_rng(77000 + draw)
    up = rng.integers(0, 2, state.shape).astype(bool)
    return np.where(up, np.nextafter(state, np.inf), np.nextafter(state, -np.inf))


def sensitivity(oracle, ref_table, inp, cc, N, u_init, want, draws=3):
    """The oracle's own sensitivity: the share of instances (of those converged before and after) whose warm iteration
    count changes when the ego state moves by one unit in the last place; the worst of `draws` draws."""
    worst = 0.0
    for d in range(draws):
        r = warm_oracle(oracle, ref_table, inp, cc, N, u_init, state=ulp_moved(inp["state"], d))
        both = converged(r["status"]) & converged(want["status"])
        if both.any():
            worst = max(worst, float((r["iters"] != want["iters"])[both].mean()))
    return worst


# s(N, cc) as sensitivity() measured it on the inputs of seed_of(N, cc), by batch size: 256 everywhere (the GPU matrix; below
# N = 63 the host-build cases too) and 96 from N = 63 (the host-build cases).  A share of the instances converged on both
# sides, hence the denominators.  test_warm_start_cpu.py recomputes every entry and requires that the fresh value does not
# exceed it.
SENSITIVITY = {
    (1, False, 256): 0.0, (1, True, 256): 0.0,
    (2, False, 256): 0.0, (2, True, 256): 0.0,
    (16, False, 256): 0.0, (16, True, 256): 0.0,
    (20, False, 256): 0.0, (20, True, 256): 1 / 255,
    (31, False, 256): 2 / 255, (31, True, 256): 0.0,
    (32, False, 256): 2 / 255, (32, True, 256): 1 / 256,
    (33, False, 256): 1 / 255, (33, True, 256): 0.0,
    (63, False, 96): 1 / 96, (63, True, 96): 1 / 89,
    (64, False, 96): 2 / 96, (64, True, 96): 1 / 93,
    (63, False, 256): 1 / 254, (63, True, 256): 2 / 247,
    (64, False, 256): 4 / 252, (64, True, 256): 6 / 242,
}


def iters_bar(N, cc, B):
    """The share of instances converged on both sides that must take the oracle's iteration count: two roundings of one
    algorithm (kernel and oracle) against the oracle's own response to one rounding, and one instance of slack."""
    return 1.0 - max(0.01, 2.0 * SENSITIVITY[(N, cc, B)] + 1.0 / B)


def unexplained_disagreements_warm(oracle, ref_table, inp, u_init, cc, got, want, tol=1e-4, tries=48, **oracle_kw):
    """conftest.unexplained_disagreements for warm-started solves: the same two conditions (both points KKT points of the
    reference NLP; the oracle's own answer jumps by more than `tol` when the ego state moves by one or two units in the last
    place, in at least one of `tries` draws), the perturbed oracle runs started from the instance's own u_init[b:b+1]."""
    import kkt_batch as kb
    import nlp_batch as nb
    both = converged(got["status"]) & converged(want["status"])
    err = rel_u0_err(got["u0"], want["u0"])
    far = np.nonzero(both & (err > tol))[0]
    bad = []
    N = got["U"].shape[1]
    for b in far:
        one = {k: (None if inp.get(k) is None else np.ascontiguousarray(inp[k][b:b + 1]))
               for k in ("state", "ego_index", "weights", "is_collide", "vref", "others")}
        p = nb.Batch.build(ref_table, one["state"], one["ego_index"], one["weights"], one["is_collide"], vref=one["vref"],
                           others=one["others"] if cc else None, collision_cost=cc, N=N)
        eps = 1e-8 / kb.objective_scale(p)
        ok = True
        for sol in (got, want):
            c = kb.certify(p, sol["X"][b:b + 1], sol["U"][b:b + 1], eps_c=eps)
            ok = ok and c["stationarity"].max() <= 1e-8 and c["feasibility"].max() <= 1e-10
        chaotic = False
        rng = np.random.default_rng(1000 + int(b))
        for _ in range(tries if ok else 0):
            d = rng.integers(-2, 3, one["state"].shape)
            st = one["state"].copy()
            for _k in range(2):
                st = np.where(d > _k, np.nextafter(st, np.inf), np.where(d < -_k, np.nextafter(st, -np.inf), st))
            r = oracle.solve_batch(ref_table, st, one["ego_index"], one["weights"], one["is_collide"], vref=one["vref"],
                                   others=one["others"] if cc else None, collision_cost=cc, xy_bounds=False, N=N,
                                   u_init=np.ascontiguousarray(u_init[b:b + 1]), **oracle_kw)
            if converged(r["status"])[0] and rel_u0_err(r["u0"], want["u0"][b:b + 1])[0] > tol:
                chaotic = True
                break
        if not (ok and chaotic):
            bad.append(int(b))
    return bad


def warm_gates(oracle, ref_table, inp, u_init, cc, N, got, want, fractions=True):
    """The gates of a warm-started build against the warm-started oracle: the fraction bars of the cold matrix
    (_bars: status, and with `fractions` also both, agree, p99 - bars set for batches of 256), the equal-iteration bar of
    this module, no unexplained disagreement, a certificate for every converged answer (the allowances of the cold matrix
    at N >= 63), and the NaN rows' statuses equal.  Returns the measurements."""
    from solve_gates import TOL, agreement, certify_converged
    B = len(got["status"])
    m = agreement(got, want)
    bars = _bars(N, cc)
    assert m["status"] >= bars.get("status", 0.0), m
    if fractions:
        assert m["both"] >= bars["both"], m
        assert m["agree"] >= bars.get("agree", 0.0), m
        assert m["p99"] < bars.get("p99", np.inf), m
    m["iters_bar"] = iters_bar(N, cc, B)
    assert m["iters"] >= m["iters_bar"], m
    assert np.array_equal(got["status"][NAN_ROWS], want["status"][NAN_ROWS]), (got["status"][NAN_ROWS], want["status"][NAN_ROWS])
    assert unexplained_disagreements_warm(oracle, ref_table, inp, u_init, cc, got, want, TOL, max_iter=100) == []
    long = N >= 63
    c = certify_converged(_nlp(ref_table, inp, cc, N), got["status"], got["X"], got["U"],
                          kink_wall_tol=1e-4 if long else None, ipopt_factor=10.0 if long else 1.0)
    m["cert"] = 0.0 if c["cert"] is None else float(np.max(c["cert"]["stationarity"] / c["tol"]))
    m["n_cert"] = int(c["sel"].size)
    return m


# ------------------------------------------------------------------------------------- the per-environment memory
def solved(status):
    """MPC_STATUS_IS_SOLVED."""
    return converged(status)


class WarmMemory:
    """What the handle remembers per environment for MPC_FLAG_WARM_START: valid[b] (0 at first) and U_prev[b], the controls
    of the environment's last solve, solved or not.  Environments appear cold the first time a step reaches them and keep
    what they hold while shorter steps pass them by."""

    def __init__(self, N):
        self.N = N
        self.valid = np.zeros(0, bool)
        self.U_prev = np.zeros((0, N, 2))

    def reach(self, B):
        if B > len(self.valid):
            n = B - len(self.valid)
            self.valid = np.concatenate([self.valid, np.zeros(n, bool)])
            self.U_prev = np.concatenate([self.U_prev, np.zeros((n, self.N, 2))])

    def u_init(self, rows):
        """The initial controls of the rows' next warm solve."""
        return advance(self.U_prev[rows])

    def record(self, U, status):
        """After a step of len(U) environments: every row's controls, solved or not; valid only where solved."""
        B = len(U)
        self.U_prev[:B] = U
        self.valid[:B] = solved(status)

    def forget(self, which=None):
        """A reset (mask, ids or all) or restored detector records: the environments' next solve starts cold."""
        if which is None:
            self.valid[:] = False
        else:
            self.valid[which] = False


def expected_step(mem, inp, weights, cc, solve):
    """The step the memory predicts for the problem data `inp` of B environments (engine.last_inputs): rows grouped by whether
    they hold a valid start and, with the collision cost, by their vehicle count; each group through
    solve(sub, u_init or None) -> dict(u0, U, status, iters), the solve entry with exactly the group's vehicles.  Records
    the step in `mem` and returns dict(u0, U, status, iters, warm) with warm the rows that started warm."""
    B, N = len(inp["state"]), mem.N
    mem.reach(B)
    warm = mem.valid[:B].copy()
    out = dict(u0=np.full((B, 2), np.nan), U=np.full((B, N, 2), np.nan), status=np.full(B, -77, np.int32),
               iters=np.full(B, -77, np.int32))
    for w in (False, True):
        rows = np.nonzero(warm == w)[0]
        r = solve_grouped(inp, weights, cc, rows, mem.u_init(rows) if w else None, N, solve)
        for k in out:
            out[k][rows] = r[k]
    assert (out["status"] != -77).all()
    mem.record(out["U"], out["status"])
    out["warm"] = warm
    return out


def solve_grouped(inp, weights, cc, rows, u_init, N, solve):
    """The environments `rows` of `inp` through solve(sub, u_init or None), grouped by vehicle count with the collision cost
    (a group's `others` are exactly its vehicles, None for none); u_init [len(rows), N, 2] or None for cold starts."""
    n = len(rows)
    out = dict(u0=np.full((n, 2), np.nan), U=np.full((n, N, 2), np.nan), status=np.full(n, -77, np.int32),
               iters=np.full(n, -77, np.int32))
    nveh = inp["nveh"][rows] if cc else np.zeros(n, np.int32)
    for nv in np.unique(nveh):
        j = np.nonzero(nveh == nv)[0]
        g = rows[j]
        sub = dict(state=inp["state"][g], ego_index=inp["ego_index"][g], weights=weights[g], is_collide=inp["is_collide"][g],
                   vref=inp["vref"][g], others=np.ascontiguousarray(inp["others"][g, :nv]) if nv > 0 else None)
        r = solve(sub, None if u_init is None else np.ascontiguousarray(u_init[j]))
        for k in out:
            out[k][j] = r[k]
    return out


def bits_equal(a, b):
    """Equal bit for bit (float64 compared as int64: -0.0 is not 0.0, a NaN equals only itself)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64 and b.dtype == np.float64:
        a, b = a.view(np.int64), b.view(np.int64)
    return a.shape == b.shape and bool((a == b).all())


def rows_differing(a, b):
    """Per row: do the float64 rows of a and b differ in any bit."""
    a, b = np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)
    return (a != b).reshape(len(a), -1).any(axis=1)
