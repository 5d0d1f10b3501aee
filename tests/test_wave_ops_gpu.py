"""The device side of the wave interface (csrc/mpc_wave_dev.hpp: WaveOpsT<RELAX> - the FP64 matrix core, the DPP lane permutations
and their bank masks, the reductions' association, the tie rule of the ratio, LDS phases without a hardware barrier) run one
primitive at a time by tests/dev_wave_ops.hip, in every RELAX build the engine instantiates, against
  - the host model of tests/host_wave_ctx.hpp, which every CPU test of the solvers rests on: bit for bit on every set, and
  - the plain numpy statements of tests/wave_ops_cases.py on the integer, lane-id and tie sets (and on every set for the
    primitives that only move or select values).
Every result lies between guard margins that must come back untouched."""
import numpy as np
import pytest

import wave_ops_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


@pytest.mark.parametrize("relax", wc.RELAX_BUILDS)
@pytest.mark.parametrize("op", wc.OPS)
def test_device_equals_host_model_and_numpy(dev, op, relax):
    for kind in wc.kinds(op):
        x = wc.inputs(op, kind)
        got = wc.device_op(op, x, relax, dev)
        host = wc.host_op(op, x, relax)
        differ = np.nonzero((got.view(np.uint64) != host.view(np.uint64)).any(axis=(1, 2)))[0]
        assert wc.same_bits(got, host), f"{op} / {kind} / RELAX {relax}: device and host model differ on sets {differ[:8]} " \
                                        f"({differ.size} of {x.shape[0]})"
        if wc.has_numpy_statement(op, kind):
            assert wc.same_bits(got, wc.numpy_op(op, x)), f"{op} / {kind} / RELAX {relax}: device differs from the numpy statement"


def test_unknown_build_or_operation_is_refused(dev):
    import torch
    lib = wc.device_lib()
    buf = torch.zeros(16 * 64, dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    assert lib.dev_wave_op(5, 0, 1, buf.data_ptr(), buf.data_ptr(), s) == -1
    assert lib.dev_wave_op(0, len(wc.OPS), 1, buf.data_ptr(), buf.data_ptr(), s) == -1
    assert lib.dev_wave_op(0, 0, 0, buf.data_ptr(), buf.data_ptr(), s) == -1
