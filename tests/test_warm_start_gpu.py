"""The warm-start path of every build of the solve kernel, and the per-environment memory behind MPC_FLAG_WARM_START.

What this module covers of the warm path (mpc_solve_wave_kernel's plumbing around Solver::solve, and the handle's memory):
  (a) every build - collision cost on / off x compiled horizon 16 / 20 (latency and throughput build) / runtime horizons
      1, 2, 31, 32, 33, 63, 64 - started from given controls through mpc_solve_batch (u_shift 0, no u_valid): the `lane < N`
      load, warm_clamp of out-of-range and NaN controls, the fall-back to the cold start when the warm rollout leaves the
      state bounds; against the warm-started oracle with an equal-iteration bar derived from the oracle's own sensitivity
      (warm_cases.iters_bar), no unexplained disagreement, and a KKT certificate for everything converged;
  (b) latency against throughput build, and host against device pointers, bit for bit on the same warm inputs;
  (c) mpc_predict_batch's memory bit for bit against the solve entry and a host model (warm_cases.WarmMemory): u_shift 1
      with the last stage repeated, u_valid read before and written after the solve (only a solved instance seeds the next
      start, every instance's controls are stored), u_init aliasing U_out under the launch order of mpc_order_kernel, and
      what forgets or keeps the memory: mpc_reset_env_mask with and without MPC_FLAG_WARM_START, mpc_reset_env_state (ids and
      all), mpc_set_env_state, shorter steps, growth of the per-environment buffers past their first capacity.
The closed-loop claim - warm-started collection needs fewer iterations on average - stays in
test_predict_gpu.py::test_warm_start_flag."""
import numpy as np
import pytest

import warm_cases as wc
from test_solve_builds_gpu import _obs_rows

pytestmark = pytest.mark.gpu

B_SOLVE = 256
_ENGINES = {}


def _engine(N, max_iter=100):
    from mpc_rl_for_avs_amd import engine
    if (N, max_iter) not in _ENGINES:
        _ENGINES[(N, max_iter)] = engine.MPCEngine(horizon=N, max_iter=max_iter)
    return _ENGINES[(N, max_iter)]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
    wc.clear_cases()


def _solve_warm(e, inp, cc, u_init, throughput):
    """mpc_solve_batch with MPC_FLAG_WARM_START | MPC_FLAG_DEVICE_PTRS (the binding's device path has no initial controls):
    U holds u_init going in and the solution coming out."""
    import torch
    from mpc_rl_for_avs_amd import engine as E
    dev = torch.device("cuda", 0)
    B, N = inp["state"].shape[0], e.horizon
    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    f64, i32 = torch.float64, torch.int32
    others = t(inp.get("others") if cc else None, f64)
    a = dict(state=t(inp["state"], f64), ego=t(inp["ego_index"], i32), vref=t(inp.get("vref"), f64),
             w=t(inp["weights"], f64), coll=t(inp["is_collide"], torch.uint8))
    out = dict(u0=torch.empty((B, 2), dtype=f64, device=dev), U=t(u_init, f64),
               X=torch.empty((B, N + 1, 4), dtype=f64, device=dev), status=torch.full((B,), -77, dtype=i32, device=dev),
               iters=torch.full((B,), -77, dtype=i32, device=dev))
    assert tuple(out["U"].shape) == (B, N, 2)
    flags = E.FLAG_WARM_START | E.FLAG_DEVICE_PTRS | (E.FLAG_COLLISION_COST if cc else 0) | (E.FLAG_THROUGHPUT if throughput else 0)
    rc = e._lib.mpc_solve_batch(e._h, B, E._ptr(a["state"]), E._ptr(a["ego"]), E._ptr(a["vref"]), E._ptr(a["w"]),
                                E._ptr(a["coll"]), E._ptr(others), 0 if others is None else int(others.shape[1]), flags,
                                E._ptr(out["u0"]), E._ptr(out["U"]), E._ptr(out["X"]), E._ptr(out["status"]),
                                E._ptr(out["iters"]), E._stream(dev))
    e._check(rc, "mpc_solve_batch")
    torch.cuda.synchronize(dev)
    r = {k: v.cpu().numpy() for k, v in out.items()}
    assert (r["status"] != -77).all() and (r["iters"] != -77).all()
    return r


def _warm_build(oracle, ref_table, cc, N, throughput):
    inp, u_init, cold, want = wc.warm_case(oracle, ref_table, N, cc, B_SOLVE)
    share = wc.warm_changes_iterations(cold, want, N)
    got = _solve_warm(_engine(N), inp, cc, u_init, throughput)
    m = wc.warm_gates(oracle, ref_table, inp, u_init, cc, N, got, want)
    m["warm_vs_cold_iters"] = round(share, 3)
    return m


# ---------------------------------------------------------------------------------------------------- (a) build matrix, warm
@pytest.mark.parametrize("build", ["latency", "throughput"])
@pytest.mark.parametrize("N", wc.COMPILED_N)
@pytest.mark.parametrize("cc", [False, True])
def test_compiled_horizon_builds_warm_match_oracle(oracle, ref_table, cc, N, build):
    m = _warm_build(oracle, ref_table, cc, N, build == "throughput")
    print(f"[warm builds] cc={cc} N={N} {build}: {m}")


@pytest.mark.parametrize("N", wc.RUNTIME_N)
@pytest.mark.parametrize("cc", [False, True])
def test_runtime_horizon_build_warm_matches_oracle(oracle, ref_table, cc, N):
    """Across the `lane < N` load at N = 1, 2, 63 and 64 (the interface maximum: 16 vehicles with the collision cost)."""
    m = _warm_build(oracle, ref_table, cc, N, False)
    print(f"[warm builds] cc={cc} N={N} runtime: {m}")


# ---------------------------------------------------------------------------------------------------- (b) build against build
@pytest.mark.parametrize("N", wc.COMPILED_N)
@pytest.mark.parametrize("cc", [False, True])
def test_warm_latency_and_throughput_builds_are_bit_identical(oracle, ref_table, cc, N):
    inp, u_init, _, _ = wc.warm_case(oracle, ref_table, N, cc, B_SOLVE)
    e = _engine(N)
    lat = _solve_warm(e, inp, cc, u_init, False)
    thr = _solve_warm(e, inp, cc, u_init, True)
    for k in ("status", "iters", "u0", "U", "X"):
        assert wc.bits_equal(lat[k], thr[k]), (k, int(wc.rows_differing(lat["U"], thr["U"]).sum()))


def test_warm_host_pointers_equal_device_pointers(oracle, ref_table):
    """engine.solve_batch(u_init=) stages U in and out through the handle's buffers; the same bits as the device path."""
    N, cc = 20, True
    inp, u_init, _, _ = wc.warm_case(oracle, ref_table, N, cc, B_SOLVE)
    e = _engine(N)
    dev = _solve_warm(e, inp, cc, u_init, False)
    host = e.solve_batch(inp["state"], inp["ego_index"], inp["weights"], inp["is_collide"], vref=inp["vref"],
                         others=inp["others"], collision_cost=cc, u_init=u_init)
    assert np.isnan(u_init[wc.NAN_ROWS]).all()                 # the caller's array is not the one written to
    for k in ("status", "iters", "u0", "U", "X"):
        assert wc.bits_equal(host[k], dev[k]), k


# ---------------------------------------------------------------------------------------------------- (c) the memory
def _entry(e2, cc):
    def solve(sub, u_init):
        return e2.solve_batch(sub["state"], sub["ego_index"], sub["weights"], sub["is_collide"], vref=sub["vref"],
                              others=sub["others"], collision_cost=cc, u_init=u_init)
    return solve


def _same_records(a, b, rows=None):
    rows = slice(None) if rows is None else rows
    return all(np.array_equal(a[k][rows], b[k][rows], equal_nan=True) for k in a)


class _Loop:
    """An engine stepped with warm_start=True next to the model of its memory; every step compared bit for bit with what
    the model expects from a second engine's solve entry."""

    def __init__(self, N, cc, B, max_iter, seed):
        from mpc_rl_for_avs_amd import engine
        self.N, self.cc, self.B = N, cc, B
        self.e = engine.MPCEngine(horizon=N, max_iter=max_iter)
        self.solve = _entry(_engine(N, max_iter), cc)
        self.mem = wc.WarmMemory(N)
        self.rng = np.random.default_rng(seed)
        self.seed = seed
        self.t = 0
        self.seen = set()
        self.valid_share = []

    def step(self, B=None):
        """One step of the first B environments: the same egos every step, a fresh draw of which vehicles are present, RL
        weights on odd steps.  Returns (inp, prev, exp): the problem data, the memory's controls before the step, the
        expected answers with the rows that started warm."""
        B = self.B if B is None else B
        obs = _obs_rows(self.B, 10, self.seed, self.rng)[:B]
        w = self.rng.uniform(0.0, 1.0, (B, 3)) if self.t % 2 == 1 else np.ones((B, 3))
        got = self.e.predict_batch(obs, w, warm_start=True, collision_cost=self.cc)
        inp = self.e.last_inputs(B, 10)
        inp["weights"] = w
        self.seen |= set(np.unique(inp["nveh"]).tolist())
        self.mem.reach(B)
        prev = self.mem.U_prev[:B].copy()
        exp = wc.expected_step(self.mem, inp, w, self.cc, self.solve)
        differ = {k: int(wc.rows_differing(got[a].astype(np.float64), exp[k].astype(np.float64)).sum())
                  for a, k in (("act", "u0"), ("status", "status"), ("iters", "iters"))}
        assert wc.bits_equal(got["act"], exp["u0"]) and np.array_equal(got["status"], exp["status"]) and \
            np.array_equal(got["iters"], exp["iters"]), (self.t, B, differ, int(exp["warm"].sum()))
        self.valid_share.append(float(self.mem.valid[:B].mean()))
        self.t += 1
        return inp, prev, exp

    def third(self, B=None):
        return self.rng.uniform(size=self.B if B is None else B) < 1.0 / 3.0

    def reset_mask(self, mask, warm_only):
        import torch
        before = self.e.env_state(self.B)
        self.e.reset_env_mask_torch(torch.as_tensor(mask.astype(np.uint8), device="cuda:0"), warm_only=warm_only)
        torch.cuda.synchronize()
        after = self.e.env_state(self.B)
        if warm_only:
            assert _same_records(before, after)                    # the detector records are untouched
        else:
            assert _same_records(before, after, ~mask)
            assert (after["collision_memory"][mask] == 0).all() and (after["is_collide"][mask] == 0).all()
        self.mem.forget(np.nonzero(mask)[0])

    def reset_ids(self, ids):
        before = self.e.env_state(self.B)
        self.e.reset_env_state(ids)
        after = self.e.env_state(self.B)
        if ids is None:
            assert (after["collision_memory"] == 0).all()
            self.mem.forget()
        else:
            keep = np.ones(self.B, bool)
            keep[ids] = False
            assert _same_records(before, after, keep) and (after["collision_memory"][ids] == 0).all()
            self.mem.forget(ids)

    def restore(self):
        before = self.e.env_state(self.B)
        self.e.load_env_state(self.e.save_env_state(self.B))
        assert _same_records(before, self.e.env_state(self.B))      # the detector is kept
        self.mem.forget(np.arange(self.B))

    def power(self, inp, prev, exp):
        """The comparison can see the faults it is there for: on the rows that started warm, the expected first control
        differs in bits from the cold answer, from the answer started at the unshifted memory and from the one with the
        last stage zeroed, each on at least half of the rows (the solve entry on the expected side only)."""
        g = np.nonzero(exp["warm"])[0]
        assert g.size >= 32, g.size
        zeroed = wc.advance(prev[g])
        zeroed[:, -1] = 0.0
        shares = {}
        for name, u in (("cold", None), ("unshifted", prev[g]), ("last stage zeroed", zeroed)):
            r = wc.solve_grouped(inp, inp["weights"], self.cc, g, u, self.N, self.solve)
            shares[name] = float(wc.rows_differing(r["u0"], exp["u0"][g]).mean())
        assert min(shares.values()) >= 0.5, shares
        return shares

    def close(self):
        self.e.close()


MEMORY_CASES = [(N, cc, 100) for N in (2, 16, 20, 33, 64) for cc in (False, True)] + [(16, False, 10)]


@pytest.mark.parametrize("N,cc,max_iter", MEMORY_CASES)
def test_memory_bit_for_bit_through_resets(N, cc, max_iter):
    """Six steps of 192 environments (one of them of the first 120 only) with, in between: the warm-only mask reset, the
    full mask reset, the reset by ids, the shorter step, restored detector records.  With max_iter 10 a large share of
    solves ends unsolved: both values of `valid` occur on >= 10 % of the rows."""
    B, Bs = 192, 120
    L = _Loop(N, cc, B, max_iter, 9500 + N + (50 if cc else 0))
    try:
        L.step()
        L.reset_mask(L.third(), warm_only=True)
        inp, prev, exp = L.step()
        assert 0 < exp["warm"].sum() < B
        shares = L.power(inp, prev, exp)
        L.reset_mask(L.third(), warm_only=False)
        L.step()
        L.reset_ids(np.nonzero(L.third())[0].astype(np.int32))
        L.step(Bs)
        kept = L.mem.valid[Bs:].copy()
        _, _, exp = L.step()                                       # environments beyond the shorter step kept their memory
        assert np.array_equal(exp["warm"][Bs:], kept) and kept.any()
        L.restore()
        _, _, exp = L.step()
        assert not exp["warm"].any()
        share = float(np.mean(L.valid_share))
        print(f"[warm memory] N={N} cc={cc} max_iter={max_iter}: bits differing from the warm answer {shares}, "
              f"valid after each step {np.round(L.valid_share, 3).tolist()}")
        if max_iter == 10:
            assert 0.1 <= share <= 0.9, L.valid_share
        assert 0 in L.seen and len(L.seen) >= 3, L.seen             # vehicle counts: none, and at least two others
    finally:
        L.close()


@pytest.mark.parametrize("N,cc", [(N, cc) for N in (2, 16, 20, 33, 64) for cc in (False, True)])
def test_memory_survives_growth_and_full_reset(N, cc):
    """A fresh engine stepped at 200 environments, then at 300: the per-environment buffers grow past their first capacity
    (256), the old environments keep their controls and `valid`, the new ones start cold.  Then mpc_reset_env_state for all:
    everything starts cold."""
    L = _Loop(N, cc, 300, 100, 9700 + N + (50 if cc else 0))
    try:
        L.step(200)
        L.step(200)
        assert L.mem.valid[:200].mean() > 0.5
        _, _, exp = L.step()
        assert exp["warm"][:200].mean() > 0.5 and not exp["warm"][200:].any()
        _, _, exp = L.step()
        assert exp["warm"][200:].mean() > 0.5
        L.reset_ids(None)
        _, _, exp = L.step()
        assert not exp["warm"].any()
    finally:
        L.close()


@pytest.mark.parametrize("B", [1100, 4100])
def test_memory_under_the_launch_order(B):
    """u_init aliases U_out (the handle's d_warm) while mpc_order_kernel permutes which workgroup owns which instance: a
    batch just above one wave per SIMD (4 x CUs = 1024: launch order, latency build) and one just above the switch to the
    throughput build (4096), N = 20 with the collision cost, three steps, bit comparison only (the expected side runs
    whichever build its group sizes select: the builds are bit-identical by the test above)."""
    L = _Loop(20, True, B, 100, 9900 + B)
    try:
        L.step()
        _, _, exp = L.step()
        assert exp["warm"].mean() > 0.5
        L.reset_mask(L.third(), warm_only=True)
        _, _, exp = L.step()
        assert 0.2 < exp["warm"].mean() < 0.9
    finally:
        L.close()
