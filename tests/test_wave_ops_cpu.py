"""The host model of the wave primitives (tests/host_wave_ctx.hpp, through tests/cpu_wave_ops_harness.cpp) against their plain
numpy statements (tests/wave_ops_cases.py), the premise of the rounding sets, and the cross-compilation of the device probe.
tests/test_wave_ops_gpu.py holds the device to the same statements and to this model bit for bit."""
import os

import numpy as np
import pytest

import wave_ops_cases as wc

CASES = [(op, kind) for op in wc.OPS for kind in wc.kinds(op)]


@pytest.mark.parametrize("op,kind", [c for c in CASES if wc.has_numpy_statement(*c)], ids=lambda v: str(v))
def test_host_model_equals_numpy(op, kind):
    x = wc.inputs(op, kind)
    want = wc.numpy_op(op, x)
    for relax in (0, 11):                                    # the host model's two code paths
        got = wc.host_op(op, x, relax)
        bad = np.nonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=(1, 2)))[0]
        assert wc.same_bits(got, want), f"{op} / {kind} / relax {relax}: sets {bad[:8]} differ"


def test_every_operation_has_integer_sets():
    for op in wc.OPS:
        assert "int" in wc.kinds(op), op
        x = wc.inputs(op, "int")
        assert x.shape[0] >= 32 and np.array_equal(x, np.rint(x)) and np.abs(x).max() < 2.0 ** 32


def test_ratio_tie_sets_tie():
    """every tie set has at least two lanes with the same largest ratio and different denominators: the rule decides"""
    x = wc.inputs("max_ratio", "tie")
    assert x.shape[0] >= 32
    for s in range(x.shape[0]):
        r = x[s, 0] / x[s, 1]                                 # 1.5 exactly in the tied lanes, below 0.5 elsewhere
        top = np.nonzero(r == r.max())[0]
        assert top.size >= 2 and np.unique(x[s, 1, top]).size == top.size and (x[s, 1] > 0).all()
    pairs = {tuple(sorted(np.nonzero(x[s, 0] / x[s, 1] == 1.5)[0])) for s in range(x.shape[0])}
    for step in range(4):                                     # partner lanes of every exchange step, and lanes of different rows
        assert any(len(p) == 2 and wc.row_partner(p[0], step) == p[1] for p in pairs), step
    assert any(len(p) == 2 and p[0] // 16 != p[1] // 16 for p in pairs)


@pytest.mark.parametrize("op", ["reduce", "suffix_sum", "sum2", "mfma"])
def test_rounding_sets_show_the_order(op):
    """On at least 90 % of the rounding sets the documented association gives other bits than plain index order: only then does
    the bit comparison of device and host model say anything about the order of the additions.  (The sets of wave_sum and
    wave_sum2 are drawn until they do - the draw asserts that enough did; here the host model itself confirms it.)"""
    x = wc.inputs(op, "round")
    got = wc.host_op(op, x)
    got = got[:, 0, :1] if op == "reduce" else (got[:, :, 0] if op == "sum2" else got[:, 0])
    plain = wc.left_to_right(op, x)
    differs = (got.view(np.uint64) != np.ascontiguousarray(plain).view(np.uint64)).reshape(x.shape[0], -1).any(axis=1)
    print(f"[wave ops] {op}: {differs.sum()} of {differs.size} rounding sets differ from index order")
    assert differs.mean() >= 0.9
    if op == "mfma":          # ... and than the same fused steps with k running the other way
        other = (got.view(np.uint64) != wc.mfma_reversed_k(x).view(np.uint64)).any(axis=1)
        print(f"[wave ops] mfma: {other.sum()} of {other.size} rounding sets differ from k = 3 ... 0")
        assert other.mean() >= 0.9


def test_probe_cross_compiles_for_gfx950(tmp_path):
    """the device probe compiles with the product's compiler and flags (no GPU needed; no hipcc is a failure): a compile error
    shows here.  Compiled into a scratch file: the library the GPU tests load is left alone."""
    path = wc.compile_device_lib(str(tmp_path / "libdev_wave_ops.so"))
    assert os.path.getsize(path) > 0
    with open(path, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"dev_wave_op" in blob and b"dev_math" in blob
