"""TEST INFRASTRUCTURE - shapes, inputs and references that drive the two kernels which write the training data
(mpc_rollout_record, mpc_rollout_finish; csrc/mpc_rollout_glue.hpp and their __global__ wrappers in csrc/mpc_engine.hip) through
their edges: tests/test_rollout_glue_cases_cpu.py runs the host build of the per-thread code over these lists, and
tests/test_rollout_glue_gpu.py the device entry points.  Both results are defined exactly - the record is copies, the finish is
float32 operation by operation in the order of RolloutBuffer.bootstrap_truncated + compute_returns_and_advantage - so every
comparison here is of bit patterns (NaNs: equal positions) and no tolerance appears."""
import functools

import numpy as np
import torch

from mpc_rl_for_avs_amd import rollout

O = 80                       # observation columns (VEHICLES_COUNT x 8)
START_STEP = 7               # the policy-step counter's value before the first record launch
PAST_END = 2                 # record launches issued past the end of the buffer in every record case
GAMMA_LAMBDA = ((0.99, 0.95), (0.9, 1.0), (1.0, 1.0), (0.0, 0.5))


def cols_of(A, keep):
    return O + A + 4 + ((O + 1) if keep else 0)


# ---- record: (B, A, keep_terminal, T) -------------------------------------------------------------------------------------
# B = 1: the ticket's B - 1 == 0 case (the only workgroup is also the last); 3: a few workgroups; 257: just past a multiple of
# the 256 compute units; 8193: more than twice the 256 x 16 two-wave workgroups that can be resident, so the workgroup that
# takes the last ticket starts after others have retired.  Every B at A = 1 with both keep_terminal, every A (8 = kMaxAction) at
# B = 3 and 257.
def _record_cases():
    cases = []
    for B in (1, 3, 257):
        for keep in (0, 1):
            for T in (1, 4):
                cases.append((B, 1, keep, T))
    cases += [(8193, 1, 0, 3), (8193, 1, 1, 3)]
    for B in (3, 257):
        for A in (3, 8):
            for keep in (0, 1):
                cases.append((B, A, keep, 4 if (A == 3) == bool(keep) else 1))
    return cases


RECORD_CASES = _record_cases()
GRAPH_CASE = (257, 3, 1, 5)
COUPLED_CASE = (5, 3, 1, 7)


def record_id(case):
    return "B%d-A%d-keep%d-T%d" % case


# ---- finish: (T, B, A, mode) ----------------------------------------------------------------------------------------------
# T walks the seams of the 256-thread stride and of the LDS split delta = lds[0:T], coef = lds[T:2T]: thread 0 alone, 2, one short
# of / exactly / one past one pass of the stride, a third pass with one thread, and the entry point's maximum (64 KB of LDS).
# mode: "plain" keep_terminal = 0; "bootstrap" keep_terminal = 1 with terminal values; "keep-null" keep_terminal = 1 with
# terminal_values = NULL (no bootstrap, rewards untouched).
FINISH_T = (1, 2, 255, 256, 257, 513, 8192)
FINISH_MODES = ("plain", "bootstrap", "keep-null")


def _finish_cases():
    cases = []
    for (B, A) in ((3, 8), (5, 3)):
        cases += [(T, B, A, m) for T in FINISH_T for m in FINISH_MODES]
    cases += [(T, 1, 1, m) for T in (1, 257, 8192) for m in FINISH_MODES]
    cases += [(T, 160, 1, m) for T in (1, 257) for m in FINISH_MODES]          # T = 8192 stays at B <= 5
    return cases


FINISH_CASES = _finish_cases()
NONFINITE_CASES = ((300, 6, 2, "plain"), (300, 6, 2, "bootstrap"))


def finish_id(case):
    return "T%d-B%d-A%d-%s" % case


# ---- memory the test owns around every array a kernel writes --------------------------------------------------------------
SENTINEL = 0xA5


def guarded(shape, dtype, device, margin=None):
    """A zeroed tensor of `shape` in the middle of a larger allocation whose margins hold the byte SENTINEL, and a function that
    asserts the margins still do.  A margin is `margin` elements (default: one slice of the leading index, B x cols for the buffer
    [T][B][cols] - where a write to row T or row -1 lands - and never less than 256), rounded up to a multiple of 16 bytes so that
    the view starts 16-byte aligned."""
    shape = tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape)) * item
    m = max(int(np.prod(shape[1:])) if margin is None else int(margin), 256) * item
    m = (m + 15) // 16 * 16
    raw = torch.full((m + n + m,), SENTINEL, dtype=torch.uint8, device=device)
    view = raw[m:m + n].view(dtype).view(shape)
    view.zero_()
    assert view.data_ptr() % 16 == 0

    def intact(name=""):
        assert bool((raw[:m] == SENTINEL).all()), f"{name}: something wrote in front of the array"
        assert bool((raw[m + n:] == SENTINEL).all()), f"{name}: something wrote behind the array"

    return view, intact


def bits(t):
    """The array as integers on the host: what a copy must preserve (-0.0, NaN payloads, infinities)."""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- record: inputs ---------------------------------------------------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(int(sum((int(k) + 1) * p for k, p in zip(key, (1000003, 10007, 101, 7, 1)))) % (2 ** 31))
    return g


def _payload_nan(t, index, payload=0x7FC12345):
    """a quiet NaN that is not the default one: a copy carries its payload"""
    flat = t.view(-1)
    if t.dtype == torch.float32:
        flat.view(torch.int32)[index] = payload
    else:
        flat.view(torch.int64)[index] = 0x7FF8000000012345


def record_initial(case, device="cpu"):
    """last_obs [B, 80] and last_starts [B] before the first step of a record case"""
    B, A, keep, T = case
    g = _gen(B, A, keep, T, -1)
    return torch.randn(B, O, generator=g).to(device), (torch.rand(B, generator=g) < 0.3).float().to(device)


def record_inputs(case, step, device="cpu", plant=True):
    """What one mpc_rollout_record launch reads at `step` of `case`, from a generator of that pair alone.  MPC status drawn from
    0 ... 8 (solved 0, 5, 6, 7 and unsolved codes both occur); crashed and arrived are subsets of done.  plant: every step carries
    a -0.0, a NaN with a payload and an infinity of each sign somewhere in its float inputs - float32 and float64 - which the
    record, a copy, must carry bit for bit (off for the coupled test, whose advantages are compared as numbers)."""
    B, A, keep, T = case
    g = _gen(B, A, keep, T, step)
    rn = lambda *s, dt=torch.float32: torch.randn(*s, generator=g, dtype=dt)
    coin = lambda p: torch.rand(B, generator=g) < p
    d = dict(actions=rn(B, A), values=rn(B), log_probs=rn(B), mpc_act=rn(B, 2, dt=torch.float64),
             mpc_status=torch.randint(0, 9, (B,), generator=g, dtype=torch.int32), new_obs=rn(B, O), reward=rn(B),
             terminal_obs=rn(B, O))
    done = coin(0.3)
    d.update(done=done, truncated=coin(0.2), crashed=done & coin(0.5), arrived=done & coin(0.5))
    if plant:
        at = lambda n: int(torch.randint(0, n, (1,), generator=g))
        d["actions" if step % 2 == 0 else "reward"].view(-1)[at(B)] = -0.0
        d["terminal_obs"].view(-1)[at(B * O)] = -0.0
        _payload_nan(d["new_obs"], at(B * O))
        _payload_nan(d["mpc_act"], 2 * at(B) + 1)
        d["mpc_act"].view(-1)[2 * at(B)] = -0.0
        d["values" if step % 2 == 0 else "log_probs"][at(B)] = float("inf")
        d["log_probs" if step % 2 == 0 else "values"][at(B)] = float("-inf")
        d["terminal_obs"].view(-1)[at(B * O)] = float("inf")
    for k in ("done", "truncated", "crashed", "arrived"):
        d[k] = d[k].to(torch.uint8)
    return {k: v.contiguous().to(device) for k, v in d.items()}


def solved(status):
    return (status == 0) | ((status >= 5) & (status <= 7))          # MPC_STATUS_IS_SOLVED (include/mpc_mi355x.h)


def record_reference(case, steps, pos0=0, plant=True):
    """`steps` collector steps on the CPU in torch: RolloutBuffer.add where the position is inside the buffer (the torch path
    raises elsewhere; the kernel refuses and counts), the carry-over of observation and episode start, the five counters
    (finished, crashed, arrived, unsolved, refused), position and policy-step counter."""
    B, A, keep, T = case
    buf = rollout.RolloutBuffer(T, B, A, "cpu", keep_terminal=bool(keep))
    last_obs, starts = record_initial(case)
    counts = np.zeros(5, np.int64)
    pos, inp = pos0, None
    for s in range(steps):
        inp = record_inputs(case, s, plant=plant)
        if 0 <= pos < T:
            buf.pos = pos
            kw = dict(terminal_obs=inp["terminal_obs"], truncated=inp["truncated"].bool()) if keep else {}
            buf.add(last_obs, inp["actions"], inp["reward"], starts, inp["values"], inp["log_probs"], inp["mpc_act"], **kw)
        else:
            counts[4] += 1
        last_obs, starts = inp["new_obs"].clone(), inp["done"].float()
        counts[:4] += [int(inp["done"].sum()), int(inp["crashed"].sum()), int(inp["arrived"].sum()),
                       int((~solved(inp["mpc_status"])).sum())]
        pos += 1
    return dict(buffer=buf, row=buf._row, mpc_actions=buf.mpc_actions, last_obs=last_obs, last_starts=starts,
                dones_out=inp["done"], counts=counts, pos=pos, step_counter=START_STEP + steps)


RECORD_STATE = ("row", "mpc_actions", "last_obs", "last_starts", "dones_out", "counts")


def record_state(case, device, pos0=0):
    """Everything a record launch writes, in guarded memory on `device`: dict of tensors, and dict name -> margin check."""
    B, A, keep, T = case
    cols = cols_of(A, keep)
    spec = dict(row=((T, B, cols), torch.float32), mpc_actions=((T, B, 2), torch.float64), last_obs=((B, O), torch.float32),
                last_starts=((B,), torch.float32), dones_out=((B,), torch.uint8), counts=((5,), torch.int64),
                pos=((1,), torch.int64), ticket=((1,), torch.int32), step_counter=((1,), torch.int64))
    # margins: a full row of the buffer, B x cols elements, around the two arrays indexed by the position; a full copy around the
    # arrays indexed by the environment
    margin = dict(row=B * cols, mpc_actions=B * cols, last_obs=B * O, last_starts=B, dones_out=B)
    st, intact = {}, {}
    for name, (shape, dt) in spec.items():
        st[name], intact[name] = guarded(shape, dt, device, margin.get(name))
    lo, ls = record_initial(case, device)
    st["last_obs"].copy_(lo)
    st["last_starts"].copy_(ls)
    st["pos"].fill_(pos0)
    st["step_counter"].fill_(START_STEP)
    return st, intact


def check_record(st, intact, want, step_counter=True):
    """the state after the launches against record_reference's, everything as bit patterns, and every margin"""
    for name in ("row", "mpc_actions", "last_obs", "last_starts"):
        assert same_bits(st[name], want[name]), name
    assert torch.equal(st["dones_out"].cpu(), want["dones_out"])
    assert np.array_equal(st["counts"].cpu().numpy(), want["counts"]), (st["counts"].cpu().numpy(), want["counts"])
    assert int(st["pos"]) == want["pos"] and int(st["ticket"]) == 0
    assert int(st["step_counter"]) == (want["step_counter"] if step_counter else START_STEP)
    for name, f in intact.items():
        f(name)


# ---- finish: inputs and reference -------------------------------------------------------------------------------------
def finish_inputs(case, nonfinite=False):
    """CPU tensors of one finish case: the buffer [T, B, cols] random normal with episode starts Bernoulli 0.1 and (keep_terminal)
    truncation flags Bernoulli 0.05, last values, mixed dones, terminal values.  nonfinite: environment 0 gets one infinite
    reward mid-rollout, environment 1 one NaN value, environment 2 rewards of 3e38 that overflow in the recurrence."""
    T, B, A, mode = case
    keep = mode != "plain"
    g = _gen(T, B, A, FINISH_MODES.index(mode), int(nonfinite))
    c = O + A
    row = torch.randn(T, B, cols_of(A, keep), generator=g)
    row[..., c + 1] = (torch.rand(T, B, generator=g) < 0.1).float()
    if keep:
        row[..., c + 4 + O] = (torch.rand(T, B, generator=g) < 0.05).float()
        if mode == "bootstrap":
            row[T // 2, B - 1, c + 4 + O] = 1.0                 # at least one truncated step, whatever the draw
    if nonfinite:
        row[T // 2, 0, c] = float("inf")
        row[T // 3, 1, c + 2] = float("nan")
        row[:, 2, c] = 3e38
        row[:, 2, c + 1] = 0.0                                  # one long episode: the sum runs over the float32 range
    last_values = torch.randn(B, generator=g)
    dones = (torch.rand(B, generator=g) < 0.4)
    if B > 1:
        dones[0], dones[1] = True, False
    if nonfinite:
        dones[2] = False
    tv = torch.randn(T, B, generator=g) if mode == "bootstrap" else None
    return dict(row=row, last_values=last_values, dones=dones.to(torch.uint8), terminal_values=tv, keep=int(keep))


@functools.lru_cache(maxsize=None)
def finish_reference(case, gamma, lam, nonfinite=False):
    """bootstrap_truncated + compute_returns_and_advantage of a CPU RolloutBuffer on finish_inputs(case): rewards, advantages and
    returns after them, and whether any other column of the buffer changed (computed once per case and pair of factors and kept,
    hence without the buffer; callers do not write to it)"""
    T, B, A, mode = case
    inp = finish_inputs(case, nonfinite)
    ref = rollout.RolloutBuffer(T, B, A, "cpu", gamma=gamma, gae_lambda=lam, keep_terminal=bool(inp["keep"]))
    ref._row.copy_(inp["row"])
    if inp["terminal_values"] is not None:
        ref.bootstrap_truncated(lambda o: inp["terminal_values"].reshape(-1))
    ref.compute_returns_and_advantage(inp["last_values"], inp["dones"].bool())
    c = O + A
    others = [k for k in range(ref._row.shape[2]) if k != c]
    assert same_bits(ref._row[..., others], inp["row"][..., others])      # the torch form touches the reward column alone
    return dict(rewards=ref.rewards.clone(), advantages=ref.advantages, returns=ref.returns)


def finish_state(case, device, nonfinite=False):
    """the inputs of a finish launch on `device`, what it writes in guarded memory"""
    T, B, A, mode = case
    inp = finish_inputs(case, nonfinite)
    st, intact = {}, {}
    st["row"], intact["row"] = guarded(inp["row"].shape, torch.float32, device)
    st["advantages"], intact["advantages"] = guarded((T, B), torch.float32, device)
    st["returns"], intact["returns"] = guarded((T, B), torch.float32, device)
    st["row0"] = inp["row"].to(device)
    for k in ("last_values", "dones", "terminal_values"):
        st[k] = None if inp[k] is None else inp[k].to(device)
    st["keep"] = inp["keep"]
    return st, intact


def nan_equal(a, b):
    return np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy(), equal_nan=True)


def check_finish(case, gamma, st, intact, want):
    """row / advantages / returns against the reference; only the reward column may differ from the input, and only with the
    bootstrap on - where the reference itself must have changed a reward, so that the case cannot pass vacuously (with
    gamma = 0 the bootstrap adds 0 * V: there it must have changed none)"""
    T, B, A, mode = case
    c = O + A
    got_row, row0 = st["row"].cpu(), st["row0"].cpu()
    assert torch.equal(got_row[..., c], want["rewards"])
    others = [k for k in range(got_row.shape[2]) if k != c]
    assert same_bits(got_row[..., others], row0[..., others])           # terminal observations included
    if mode == "bootstrap" and gamma != 0.0:
        assert not torch.equal(want["rewards"], row0[..., c])
    else:
        assert same_bits(got_row[..., c], row0[..., c])
    assert torch.equal(st["advantages"].cpu(), want["advantages"]) and torch.equal(st["returns"].cpu(), want["returns"])
    for name, f in intact.items():
        f(name)


def check_nonfinite(st, intact, want):
    """finish_inputs(nonfinite=True): equal to the reference with NaNs at equal positions; environments 0 ... 2 are not finite in
    the reference (asserted, so that the case is known to bite), 3 ... are finite and bit-identical"""
    adv, ret = want["advantages"], want["returns"]
    for b in range(3):
        assert not torch.isfinite(adv[:, b]).all() and not torch.isfinite(ret[:, b]).all(), b
    assert torch.isfinite(adv[:, 3:]).all() and torch.isfinite(ret[:, 3:]).all() and adv.shape[1] > 3
    c = st["row"].shape[2] - 4 - ((O + 1) if st["keep"] else 0)
    got = dict(rewards=st["row"][..., c], advantages=st["advantages"], returns=st["returns"])
    for name in got:
        assert nan_equal(got[name], want[name]), name
        assert same_bits(got[name][:, 3:], want[name][:, 3:]), name
    others = [k for k in range(st["row"].shape[2]) if k != c]
    assert same_bits(st["row"][..., others], st["row0"][..., others])     # the NaN value of environment 1 included, bit for bit
    for name, f in intact.items():
        f(name)


# ---- record, then finish: the two kernels must agree about the row layout ------------------------------------------------
def _coupled_values():
    B, A, keep, T = COUPLED_CASE
    g = _gen(B, A, keep, T, 99)
    return torch.randn(B, generator=g), torch.randn(T, B, generator=g)          # last values, terminal values


def coupled_reference():
    """add x T, then bootstrap + GAE, on the CPU: (the record reference, the finished buffer)"""
    B, A, keep, T = COUPLED_CASE
    rec = record_reference(COUPLED_CASE, T, plant=False)
    buf = rec["buffer"]
    rec["row"] = buf._row.clone()
    buf.gamma, buf.gae_lambda = GAMMA_LAMBDA[0]
    last_values, tv = _coupled_values()
    buf.bootstrap_truncated(lambda o: tv.reshape(-1))
    buf.compute_returns_and_advantage(last_values, rec["dones_out"].bool())
    assert buf.truncated.any()                                               # something to bootstrap
    return rec, dict(row=buf._row, advantages=buf.advantages, returns=buf.returns)


def coupled_finish_state(st, device):
    """what the finish launch after COUPLED_CASE's records takes: the recorded buffer and dones in place, the rest new"""
    B, A, keep, T = COUPLED_CASE
    last_values, tv = _coupled_values()
    fin = dict(row=st["row"], dones=st["dones_out"], last_values=last_values.to(device), terminal_values=tv.to(device), keep=1,
               intact={})
    for name in ("advantages", "returns"):
        fin[name], fin["intact"][name] = guarded((T, B), torch.float32, device)
    return fin
