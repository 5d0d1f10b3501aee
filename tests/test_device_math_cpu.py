"""The lean FP64 math of csrc/mpc_core.hpp that is one branch for host and device - sincos_half, sincos_delta_theta, dyn_eval -
in the host build the CPU harnesses run, against mpmath at the bars of tests/device_math_cases.py.  The device build of every
function: tests/test_device_math_gpu.py.  Each test prints its worst errors (pytest -s)."""
import numpy as np
import pytest

import device_math_cases as mc
import wave_ops_cases as wc


def host_math(fn, x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.full((mc.N_OUT[fn], x.shape[1]), np.nan)
    rc = wc.host_lib().cpu_math(mc.FUNCTIONS.index(fn), x.shape[1], x.ctypes.data, out.ctypes.data)
    assert rc == 0, (fn, rc)
    return out


@pytest.mark.parametrize("fn", mc.HOST_FUNCTIONS)
def test_host_math_against_mpmath(fn):
    mc.check(fn, host_math(fn, mc.points(fn)), "host")


def test_device_only_functions_are_refused_on_the_host():
    """frcp, frsqrt, atan_b and log_pos run libm on the host: their lean branches exist on the device only"""
    x = np.ones((1, 4))
    out = np.zeros((1, 4))
    for fn in set(mc.FUNCTIONS) - set(mc.HOST_FUNCTIONS):
        assert wc.host_lib().cpu_math(mc.FUNCTIONS.index(fn), 4, x.ctypes.data, out.ctypes.data) == -2, fn


def test_the_error_measures_measure():
    """errors() on values a known distance from the reference: the nearest double, and its neighbour above"""
    hi, lo = mc.reference("frcp")
    e = mc.errors("frcp", hi)
    assert e["ulp"].max() <= 0.5 and e["rel"].max() <= 2.0 ** -53
    e = mc.errors("frcp", np.nextafter(hi, np.inf))
    assert 0.5 <= e["ulp"].min() and e["ulp"].max() <= 1.5 and e["rel"].min() >= 2.0 ** -54
    with pytest.raises(AssertionError):
        mc.check("frcp", np.nextafter(hi, np.inf), "self-test")
