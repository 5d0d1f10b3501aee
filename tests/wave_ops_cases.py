"""TEST INFRASTRUCTURE - input sets and plain numpy statements for the primitives of the wave interface (tests/wave_ops_probe.hpp),
and the loaders of its two builds: the host model (tests/cpu_wave_ops_harness.cpp over HostCtx) and the device probe
(tests/dev_wave_ops.hip over WaveOpsT<RELAX>).  tests/test_wave_ops_cpu.py holds the host model to the numpy statements,
tests/test_wave_ops_gpu.py the device to both.

Kinds of sets (each [S, rows, 64] float64, S = 32 unless the construction gives another count):
  int    integer values, |v| < 2^20 (mfma: < 2^10): every association of the additions is exact, so the result is a fact of plain
         arithmetic and numpy_op() states it without reference to any order;
  lane   lane ids and single bits, for what moves values between lanes;
  tie    equal maxima / minima / ratios in several lanes and rows, a lone non-zero for the suffix sum;
  round  normal doubles of both signs with exponents spread over 2^-30 ... 2^30: here the order of the additions shows in the
         bits (test_rounding_sets_show_the_order asserts that it does), device and host model are compared with each other only -
         except for the operations that move or select values without rounding, which numpy_op() states for every kind.
Values are finite, denominators positive; NaNs and signed zeros are outside what the solver feeds these primitives."""
import ctypes
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np

import conftest

L = 64
S = 32
RELAX_BUILDS = (0, 3, 7, 11)     # WaveCtx<., 0>, the preamble's 3, kRelaxLat, kLtvRelaxLat (csrc/mpc_engine.hip)
OPS = ("mfma", "lane_get", "row_bcast", "row_bcast2", "ident", "bit_select", "bcast_ballot", "reduce", "suffix_sum", "sum2",
       "max_ratio", "lds_rounds")                # the order of the enum in tests/wave_ops_probe.hpp
N_IN = dict(zip(OPS, (3, 2, 1, 1, 3, 3, 2, 1, 1, 1, 2, 1)))
N_OUT = dict(zip(OPS, (1, 8, 16, 8, 6, 2, 6, 3, 1, 2, 2, 1)))
# results that are copies or selections of the inputs, or single correctly rounded additions in a fixed pairing: numpy_op() is
# exact for every kind of set
EXACT_FOR_ALL = ("lane_get", "row_bcast", "row_bcast2", "ident", "bit_select", "bcast_ballot", "lds_rounds")
EXACT_KINDS = ("int", "lane", "tie")
LANES = np.arange(L)
GET_LANES = (0, 5, 16, 31, 32, 47, 63)
BCAST_LANES = (0, 21, 63)
LDS_ROUNDS = 8


def row_partner(l, step):
    """partner of lane l in exchange step 0 ... 3 of the row reductions: xor 1, xor 2, mirror within 8, mirror within 16"""
    return (l ^ 1, l ^ 2, (l & ~7) | (7 - (l & 7)), (l & ~15) | (15 - (l & 15)))[step]


# ---- inputs -------------------------------------------------------------------------------------------------------------
def _rng(op, kind):
    return np.random.default_rng(1000 * OPS.index(op) + ("int", "lane", "tie", "round").index(kind))


def _ints(rng, shape, bound):
    return rng.integers(-bound + 1, bound, shape).astype(np.float64)


def _normals(rng, shape):
    return (1.0 + rng.random(shape)) * np.exp2(rng.integers(-30, 31, shape)) * rng.choice([-1.0, 1.0], shape)


def _lane_rows():
    return np.stack([LANES.astype(np.float64), np.exp2(LANES % 52), (L - LANES).astype(np.float64), np.exp2(-(LANES % 52))])


def _given(rng, n):
    """a row whose every word is one lane index (the probe reads word 0), covering the row seams"""
    idx = np.concatenate([[0, 15, 16, 33, 48, 63], rng.integers(0, L, max(n - 6, 0))])[:n]
    return np.repeat(idx[:, None], L, axis=1).astype(np.float64)


def _ratio_ties(rng):
    """equal ratios 3k / 2k with different positive denominators, above every other lane's ratio (< 1/2): in the two partner
    lanes of each of the four exchange steps (both orders), in equal and different positions of two rows, and in three lanes"""
    groups = []
    for step in range(4):
        for l in (0, 5, 22, 43, 63):
            groups += [(l, row_partner(l, step))] * 2
    groups += [(3, 19), (3, 35), (3, 51), (19, 51), (7, 40), (12, 61), (15, 16), (47, 48), (0, 63)]
    groups += [(1, 2, 17), (9, 30, 55), (4, 5, 6), (20, 36, 52)]
    sets = []
    for i, g in enumerate(groups):
        n, d = rng.integers(1, 1000, L), rng.integers(2000, 4000, L)
        ks = rng.choice(np.arange(1, 400), len(g), replace=False)
        if i % 2:
            ks = ks[::-1]
        for lane, k in zip(g, ks):
            n[lane], d[lane] = 3 * k, 2 * k
        sets.append(np.stack([n, d]))
    return np.array(sets, np.float64)


@functools.lru_cache(maxsize=None)
def _inputs(op, kind):
    rng = _rng(op, kind)
    n_in = N_IN[op]
    if kind == "round":
        x = _normals(rng, (S, n_in, L))
        if op in ("reduce", "sum2"):
            # one sum per set: a few large terms often decide it in any order, so sets are drawn until S of them tell the
            # documented association from index order
            x = _normals(rng, (8 * S, n_in, L))
            lo, hi = documented_sums(x[:, 0])
            tells = ((lo + hi) != left_to_right("reduce", x)[:, 0]) & (np.stack([lo, hi], 1) != left_to_right("sum2", x)).all(axis=1)
            x = x[tells][:S]
            assert x.shape[0] == S
    elif kind == "int":
        x = _ints(rng, (S, n_in, L), 2 ** 10 if op == "mfma" else 2 ** 20)
    elif kind == "lane":
        rows = _lane_rows()
        x = np.stack([np.stack([rows[(i + r) % len(rows)] for r in range(n_in)]) for i in range(len(rows))])
    else:
        x = None
    if op == "mfma" and kind == "lane":
        # one operand the identity in every block, the other the lane id: the product is the other operand's block layout itself
        eye = ((LANES >> 4) == (LANES & 3)).astype(np.float64)
        ids, zero = LANES.astype(np.float64) + 1.0, np.zeros(L)
        x = np.array([[ids, eye, zero], [eye, ids, zero], [ids, eye, 100.0 * ids]])
    if op in ("lane_get", "bcast_ballot") and x is not None:
        x[:, 1] = _given(rng, x.shape[0])
    if op == "ident" and x is not None:
        x[:, 1] = x[:, 1, :1]                                          # the wave-uniform operand of uni / fresh
        x[:, 2] = rng.integers(-2 ** 31, 2 ** 31, (x.shape[0], L))
    if op == "bit_select" and x is not None:
        x[:, 0] = -(rng.random((x.shape[0], L)) < 0.5).astype(np.float64)     # 0 or -1 = ~0
    if op == "bcast_ballot":
        if kind == "lane":
            single = [np.where(LANES == k, 7.0, 0.0) for k in (0, 31, 32, 63)]
            rows = [LANES.astype(np.float64), np.exp2(LANES % 31), (LANES % 3 == 0).astype(np.float64), np.zeros(L), np.ones(L)]
            x = np.stack([np.stack([r, np.zeros(L)]) for r in rows + single])
            x[:, 1] = _given(rng, x.shape[0])
        elif x is not None:
            x[:, 0] = rng.integers(-2 ** 31, 2 ** 31, (x.shape[0], L)) * (rng.random((x.shape[0], L)) < 0.6)
    if op == "max_ratio":
        if kind == "tie":
            x = _ratio_ties(rng)
        elif kind == "lane":
            x = None
        else:
            x[:, 1] = np.abs(x[:, 1]) + (kind == "int")                # positive denominators
    if kind == "tie":
        if op == "reduce":
            # the extreme values of a set sit in several lanes at once: of one row, of every row, of the whole wave
            x = _ints(rng, (S, 1, L), 2 ** 20)
            for s in range(S):
                lanes = (rng.choice(L, 2 + s % 7, replace=False) if s % 3 else 16 * np.arange(4) + s % 16) if s < S - 1 else LANES
                x[s, 0, lanes] = 2.0 ** 20 if s % 2 else -2.0 ** 20
        elif op == "suffix_sum":
            x = np.zeros((S, 1, L))
            for s in range(S):
                x[s, 0, (2 * s + (s > 15)) % L] = float(rng.integers(1, 2 ** 20))
    return x


def kinds(op):
    return tuple(k for k in ("int", "lane", "tie", "round") if _inputs(op, k) is not None)


def inputs(op, kind):
    """[S', N_IN[op], 64] float64 (a copy; the cached arrays stay as drawn)"""
    return _inputs(op, kind).copy()


def has_numpy_statement(op, kind):
    return kind in EXACT_KINDS or op in EXACT_FOR_ALL


# ---- what every operation is, in plain numpy ----------------------------------------------------------------------------------
def _as_int32(x):
    return x.astype(np.int64).astype(np.int32)


def numpy_op(op, x):
    """[S', N_OUT[op], 64]: the result of `op` on the sets x, exact wherever has_numpy_statement() says so"""
    n = x.shape[0]
    out = np.zeros((n, N_OUT[op], L))
    row0 = LANES & ~15
    if op == "mfma":
        # lane 16 k + 4 blk + i holds A_blk[i][k] and B_blk[k][i]; lane 16 i + 4 blk + j holds C_blk[i][j] (host_wave_ctx.hpp)
        A = x[:, 0].reshape(n, 4, 4, 4).transpose(0, 2, 3, 1)          # [set, blk, row, k]
        B = x[:, 1].reshape(n, 4, 4, 4).transpose(0, 2, 1, 3)          # [set, blk, k, col]
        C = x[:, 2].reshape(n, 4, 4, 4).transpose(0, 2, 1, 3)          # [set, blk, row, col]
        out[:, 0] = (C + A @ B).transpose(0, 2, 1, 3).reshape(n, L)
    elif op == "lane_get":
        for i, lane in enumerate(GET_LANES):
            out[:, i] = x[:, 0, lane:lane + 1]
        out[:, 7] = x[np.arange(n), 0, x[:, 1, 0].astype(int)][:, None]
    elif op == "row_bcast":
        for j in range(16):
            out[:, j] = x[:, 0, row0 + j]
    elif op == "row_bcast2":
        for j in range(8):
            out[:, j] = x[:, 0, row0 + j + (LANES & 8)]
    elif op == "ident":
        out[:, 0] = out[:, 1] = x[:, 1, :1]
        out[:, 2] = x[:, 0]
        out[:, 3] = out[:, 4] = out[:, 5] = _as_int32(x[:, 2])
    elif op == "bit_select":
        out[:, 0] = out[:, 1] = np.where(x[:, 0] != 0, x[:, 1], x[:, 2])
    elif op == "bcast_ballot":
        q = _as_int32(x[:, 0])
        for i, lane in enumerate(BCAST_LANES):
            out[:, i] = q[:, lane:lane + 1]
        out[:, 3] = q[np.arange(n), x[:, 1, 0].astype(int)][:, None]
        out[:, 4] = ((q[:, :32] != 0) * np.exp2(LANES[:32])).sum(axis=1)[:, None]
        out[:, 5] = ((q[:, 32:] != 0) * np.exp2(LANES[:32])).sum(axis=1)[:, None]
    elif op == "reduce":
        out[:, 0] = x[:, 0].sum(axis=1)[:, None]
        out[:, 1] = x[:, 0].max(axis=1)[:, None]
        out[:, 2] = x[:, 0].min(axis=1)[:, None]
    elif op == "suffix_sum":
        out[:, 0] = np.cumsum(x[:, 0, ::-1], axis=1)[:, ::-1]
    elif op == "sum2":
        out[:, 0] = x[:, 0, :32].sum(axis=1)[:, None]
        out[:, 1] = x[:, 0, 32:].sum(axis=1)[:, None]
    elif op == "max_ratio":
        # the largest n / d as an exact fraction; among equal ratios the pair with the larger denominator
        for s in range(n):
            best = max(range(L), key=lambda l: (Fraction(int(x[s, 0, l]), int(x[s, 1, l])), x[s, 1, l]))
            out[s, 0], out[s, 1] = x[s, 0, best], x[s, 1, best]
    elif op == "lds_rounds":
        v = x[:, 0].copy()
        for r in range(LDS_ROUNDS):
            v = v + v[:, (LANES ^ 17) if r & 1 else (L - 1 - LANES)]
        out[:, 0] = v
    else:
        raise KeyError(op)
    return out


def documented_sums(v):
    """the association mpc_wave_dev.hpp documents for a sum over the wave, v [n, 64]: four symmetric partner exchanges inside
    each 16-lane row, then rows 0 + 1 and rows 2 + 3 (wave_sum2's two results; wave_sum adds them).  Used to draw the rounding
    sets only - the comparisons are with the host model itself."""
    for step in range(4):
        v = v + v[:, [row_partner(l, step) for l in range(L)]]
    return v[:, 0] + v[:, 16], v[:, 32] + v[:, 48]


def left_to_right(op, x):
    """the additive results in plain index order, one rounding per addition: what an order-blind implementation would give"""
    v = x[:, 0]
    if op == "reduce":
        return np.cumsum(v, axis=1)[:, -1:]
    if op == "suffix_sum":
        return np.cumsum(v[:, ::-1], axis=1)[:, ::-1]
    if op == "sum2":
        return np.stack([np.cumsum(v[:, :32], axis=1)[:, -1], np.cumsum(v[:, 32:], axis=1)[:, -1]], axis=1)
    if op == "mfma":                                                    # products rounded, then added in k order
        hi, blk, lo = LANES >> 4, (LANES >> 2) & 3, LANES & 3
        acc = x[:, 2].copy()
        for k in range(4):
            acc = acc + x[:, 0, 16 * k + 4 * blk + hi] * x[:, 1, 16 * k + 4 * blk + lo]
        return acc
    raise KeyError(op)


def mfma_reversed_k(x):
    """the matrix product with one fused multiply-add per k like the documented one, but k = 3 ... 0: each step the exactly
    rounded a b + acc (as fractions).  An implementation that only got the order of k wrong would give this."""
    hi, blk, lo = LANES >> 4, (LANES >> 2) & 3, LANES & 3
    out = np.zeros((x.shape[0], L))
    for s in range(x.shape[0]):
        for l in range(L):
            acc = Fraction(x[s, 2, l])
            for k in (3, 2, 1, 0):
                acc = Fraction(float(Fraction(x[s, 0, 16 * k + 4 * blk[l] + hi[l]]) * Fraction(x[s, 1, 16 * k + 4 * blk[l] + lo[l]]) + acc))
            out[s, l] = float(acc)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the two builds ---------------------------------------------------------------------------------------------------------
_CSRC = os.path.join(conftest.ROOT, "mpc-rl_for_avs_amd", "csrc")
_TESTS = os.path.join(conftest.ROOT, "tests")
_HOST_DEPS = [os.path.join(_TESTS, f) for f in ("cpu_wave_ops_harness.cpp", "wave_ops_probe.hpp", "host_wave_ctx.hpp")] + \
    [os.path.join(_CSRC, f) for f in ("mpc_core.hpp", "mpc_wave.hpp")]
_DEV_DEPS = [os.path.join(_TESTS, f) for f in ("dev_wave_ops.hip", "wave_ops_probe.hpp")] + \
    [os.path.join(_CSRC, f) for f in ("mpc_core.hpp", "mpc_wave.hpp", "mpc_wave_dev.hpp")]
DEVICE_LIB = os.path.join(_TESTS, "_build", "libdev_wave_ops.so")     # never a sanitizer build: the code runs on the device
DEVICE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC"]          # _build.build()'s, the product's


def _stale(out, deps):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps)


@functools.lru_cache(maxsize=None)
def host_lib():
    out = os.path.join(conftest.BUILD_DIR, "libcpu_wave_ops.so")
    if _stale(out, _HOST_DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["g++"] + conftest.HOST_CXXFLAGS + ["-o", out, _HOST_DEPS[0]], check=True)
    lib = ctypes.CDLL(out)
    lib.cpu_wave_op.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    lib.cpu_math.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2
    return lib


def compile_device_lib(out):
    """the probe compiled for gfx950 into `out` with the product's compiler and flags; RuntimeError without hipcc or on an error"""
    from mpc_rl_for_avs_amd import _build
    res = subprocess.run([_build._hipcc()] + DEVICE_FLAGS + ["-o", out, _DEV_DEPS[0]], capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + res.stdout + res.stderr)
    return out


def build_device_lib():
    """tests/_build/libdev_wave_ops.so: compiled when missing or older than its sources; where there is no hipcc, the library
    that build() shipped; an error if there is neither.  Returns its path."""
    from mpc_rl_for_avs_amd import _build
    if _stale(DEVICE_LIB, _DEV_DEPS):
        try:
            _build._hipcc()
        except RuntimeError:
            if not os.path.exists(DEVICE_LIB):
                raise
            return DEVICE_LIB
        os.makedirs(os.path.dirname(DEVICE_LIB), exist_ok=True)
        os.replace(compile_device_lib(DEVICE_LIB + ".tmp"), DEVICE_LIB)
    return DEVICE_LIB


@functools.lru_cache(maxsize=None)
def device_lib():
    lib = ctypes.CDLL(build_device_lib())
    lib.dev_wave_op.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
    lib.dev_math.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3
    return lib


def host_op(op, x, relax=0):
    x = np.ascontiguousarray(x, np.float64)
    assert x.shape[1:] == (N_IN[op], L)
    out = np.full((x.shape[0], N_OUT[op], L), np.nan)
    rc = host_lib().cpu_wave_op(relax, OPS.index(op), x.shape[0], x.ctypes.data, out.ctypes.data)
    assert rc == 0, (op, relax, rc)
    return out


def device_op(op, x, relax, device):
    """the probe on `device` (a torch device): the result lies between guard margins of 256 doubles, checked after the launch"""
    import torch
    from rollout_glue_cases import guarded
    x = np.ascontiguousarray(x, np.float64)
    assert x.shape[1:] == (N_IN[op], L)
    d_in = torch.from_numpy(x).to(device)
    d_out, intact = guarded((x.shape[0], N_OUT[op], L), torch.float64, device, margin=256)
    d_out.fill_(float("nan"))
    torch.cuda.synchronize(device)
    rc = device_lib().dev_wave_op(relax, OPS.index(op), x.shape[0], d_in.data_ptr(), d_out.data_ptr(),
                                  torch.cuda.current_stream(device).cuda_stream)
    assert rc == 0, (op, relax, rc)
    torch.cuda.synchronize(device)
    intact(f"{op} RELAX {relax}")
    return d_out.cpu().numpy()
