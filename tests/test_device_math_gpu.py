"""The lean FP64 math of csrc/mpc_core.hpp as the device runs it - the raw v_rcp_f64 / v_rsq_f64 seeds, frcp, frsqrt, sincos_half,
sincos_delta_theta, atan_b, log_pos, dyn_eval, with the coefficient tables read from LDS as in the solver - one point per thread
(tests/dev_wave_ops.hip: dev_math) against mpmath at the bars of tests/device_math_cases.py.  frcp, frsqrt, atan_b and log_pos
have device-only branches that no CPU test compiles.  Each test prints its worst errors (pytest -s)."""
import pytest

import device_math_cases as mc
import wave_ops_cases as wc

pytestmark = pytest.mark.gpu


def device_math(fn, x):
    import torch
    from rollout_glue_cases import guarded
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(x).to(dev)
    d_out, intact = guarded((mc.N_OUT[fn], x.shape[1]), torch.float64, dev, margin=256)
    d_out.fill_(float("nan"))
    torch.cuda.synchronize(dev)
    rc = wc.device_lib().dev_math(mc.FUNCTIONS.index(fn), x.shape[1], d_in.data_ptr(), d_out.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, (fn, rc)
    torch.cuda.synchronize(dev)
    intact(fn)
    return d_out.cpu().numpy()


@pytest.mark.parametrize("fn", mc.FUNCTIONS)
def test_device_math_against_mpmath(fn):
    mc.check(fn, device_math(fn, mc.points(fn)), "device")
