"""TEST INFRASTRUCTURE - points, mpmath references (250 bits) and error bars for the lean FP64 math of csrc/mpc_core.hpp.
tests/test_device_math_gpu.py runs the device build of every function (tests/dev_wave_ops.hip: dev_math),
tests/test_device_math_cpu.py the host build of the three that have no device-only branch.

The bars are derived, not read off the code under test (u = 2^-53):
  raw rcp / rsq       relative error <= 2^-24: the premise the header states for the hardware seeds
  frcp                <= 0.5 + 2^-18 ulp: e = 1 - x y is exact to 2^-78, the cubic remainder e^3 is 2^-72 relative, one final rounding
  frsqrt              <= 1 + 2^-17 ulp: the rounded product -x y puts up to 2^-54 relative into the result before the final rounding
  sincos_half, sin / cos(delta)    absolute <= 7e-16: the kernel polynomials are below 1 ulp of a value <= 1 (d = 1.1e-16); one
                      doubling gives 2 sqrt 2 d + 2 u (sine) resp. 4 d + 2 u (cosine)
  sin / cos(theta)    absolute <= 3e-15: a second doubling of 7e-16
  atan_b              absolute <= 1e-15: the Newton update's residual (ds + t dc) / (c + t s) <= sqrt 2 x 5e-16 plus the rounding of
                      d <= 1.4; the relative error at small |t| is reported only (nothing claims one)
  log_pos             <= 1 ulp: fdlibm's bound for e_log, which the header repeats
  dyn_eval            from the bars above.  a = 1 + 3 cd^2 lies in [1.75, 4] and its relative error is at most
                      6 cd 7e-16 / a + 2 u <= 1.73 x 7e-16 + 2.2e-16 = 1.43e-15 (6 c / (1 + 3 c^2) peaks at c = 1 / sqrt 3), so
                      q = a^-1/2 <= 0.756 carries 7.2e-16 + 1.2e-16 (frsqrt) = 8.4e-16 relative, 6.4e-16 absolute;
                      sb = sd q:    7e-16 x 0.756 + 0.87 x 6.4e-16 + u <= 1.2e-15
                      cb = 2 cd q:  2 (7e-16 x 0.756 + 6.4e-16) + u   <= 2.5e-15
                      S, C = st cb +- ct sb and its mirror: 3e-15 (|cb| + |sb|) + 2.5e-15 + 1.2e-15 + 2 u, |cb| + |sb| <= sqrt 2:
                                                                      <= 8.2e-15"""
import functools

import mpmath
import numpy as np

mp = mpmath.mp
PREC = 250
FUNCTIONS = ("rcp", "rsq", "frcp", "frsqrt", "sincos_half", "sincos_delta_theta", "atan_b", "log_pos", "dyn_eval")   # probe::FN_*
HOST_FUNCTIONS = ("sincos_half", "sincos_delta_theta", "dyn_eval")      # one branch for host and device
N_IN = dict(zip(FUNCTIONS, (1, 1, 1, 1, 1, 2, 1, 1, 2)))
N_OUT = dict(zip(FUNCTIONS, (1, 1, 1, 1, 2, 4, 1, 1, 4)))
OUTPUTS = dict(sincos_half=("sin", "cos"), sincos_delta_theta=("sin delta", "cos delta", "sin theta", "cos theta"),
               dyn_eval=("S", "C", "sin beta", "cos beta"))
# (measure, bar) per output
BARS = dict(rcp=[("rel", 2.0 ** -24)], rsq=[("rel", 2.0 ** -24)], frcp=[("ulp", 0.5 + 2.0 ** -18)], frsqrt=[("ulp", 1.0 + 2.0 ** -17)],
            sincos_half=[("abs", 7e-16)] * 2, sincos_delta_theta=[("abs", 7e-16)] * 2 + [("abs", 3e-15)] * 2,
            atan_b=[("abs", 1e-15)], log_pos=[("ulp", 1.0)], dyn_eval=[("abs", 8.2e-15)] * 2 + [("abs", 1.2e-15), ("abs", 2.5e-15)])
PI = float(np.pi)
N_RANDOM = 6144
K9 = 7.07106781186547524401e-01          # log_coef(9): the mantissa switch of log_pos


def _scaled_points(rng):
    """2^k (1 + m), k uniform in [-1000, 1000]; 2^k, 2^k (1 +- 2^-52) and 2^k (2 - 2^-52) for 64 values of k, odd and even"""
    x = np.ldexp(1.0 + rng.random(N_RANDOM), rng.integers(-1000, 1001, N_RANDOM))
    ks = np.concatenate([[-1000, -999, -2, -1, 0, 1, 2, 999, 1000], rng.integers(-1000, 1001, 55)])
    edge = [np.ldexp(m, ks) for m in (1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, 2.0 - 2.0 ** -52)]
    return np.concatenate([x] + edge)


def _angles(rng):
    """(delta, theta) inside the NLP's relaxed bounds, the four corners, and a band of theta next to +-pi"""
    dm, tm = PI / 3.0 * (1.0 + 1e-8), PI * (1.0 + 1e-8)
    delta = np.concatenate([rng.uniform(-dm, dm, N_RANDOM), [dm, dm, -dm, -dm, 0.0], rng.uniform(-dm, dm, 2048)])
    theta = np.concatenate([rng.uniform(-tm, tm, N_RANDOM), [tm, -tm, tm, -tm, 0.0],
                            rng.uniform(3.0, tm, 2048) * rng.choice([-1.0, 1.0], 2048)])
    return delta, theta


@functools.lru_cache(maxsize=None)
def _points(fn):
    rng = np.random.default_rng(77 + FUNCTIONS.index(fn))
    if fn in ("rcp", "rsq", "frcp", "frsqrt"):
        x = _scaled_points(rng)[None]
    elif fn == "sincos_half":
        x = np.concatenate([rng.uniform(-PI / 2, PI / 2, N_RANDOM), [PI / 2, -PI / 2, 0.0]])[None]
    elif fn == "sincos_delta_theta":
        x = np.stack(_angles(rng))
    elif fn == "dyn_eval":
        x = np.stack(_angles(rng)[::-1])                               # dyn_eval(theta, delta)
    elif fn == "atan_b":
        # the solver's argument is 2 s / sqrt(1 - s^2) with |s| < 0.9: |t| < 4.13
        small = np.exp2(-np.arange(0.0, 61.0))
        one = np.array([1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52])
        x = np.concatenate([rng.uniform(-4.2, 4.2, N_RANDOM), [0.0, 4.2, -4.2], one, -one, small, -small])[None]
    elif fn == "log_pos":
        k = np.arange(1.0, 53.0)
        j = np.arange(-5.0, 6.0)
        switch = np.concatenate([np.exp2(j) * m for m in (K9, K9 * (1.0 + 1e-12), K9 * (1.0 - 1e-12), np.nextafter(K9, 0.0),
                                                           np.nextafter(K9, 1.0))])
        x = np.concatenate([_scaled_points(rng), 1.0 + np.exp2(-k), 1.0 - np.exp2(-k), switch, np.exp2(np.arange(-1000.0, 1001.0, 8.0))])[None]
    else:
        raise KeyError(fn)
    x = np.ascontiguousarray(x, np.float64)
    assert x.shape[0] == N_IN[fn] and x.shape[1] <= 16384 and np.isfinite(x).all()
    return x


def points(fn):
    """[N_IN[fn], n] float64 (a copy)"""
    return _points(fn).copy()


def _exact(fn, x):
    """the N_OUT[fn] exact values at one point, as mpmath numbers"""
    a = [mp.mpf(float(v)) for v in x]
    if fn in ("rcp", "frcp"):
        return [1 / a[0]]
    if fn in ("rsq", "frsqrt"):
        return [1 / mp.sqrt(a[0])]
    if fn == "sincos_half":
        return [mp.sin(a[0]), mp.cos(a[0])]
    if fn == "sincos_delta_theta":
        return [mp.sin(a[0]), mp.cos(a[0]), mp.sin(a[1]), mp.cos(a[1])]
    if fn == "atan_b":
        return [mp.atan(a[0])]
    if fn == "log_pos":
        return [mp.log(a[0])]
    if fn == "dyn_eval":                                               # beta = atan(tan(delta) / 2), the kinematic bicycle model
        beta = mp.atan(mp.tan(a[1]) / 2)
        return [mp.sin(a[0] + beta), mp.cos(a[0] + beta), mp.sin(beta), mp.cos(beta)]
    raise KeyError(fn)


@functools.lru_cache(maxsize=None)
def reference(fn):
    """(hi, lo), each [N_OUT[fn], n]: the exact values as unevaluated sums of two doubles (hi the nearest double).  Computed once
    per process; callers do not write to it."""
    x = _points(fn)
    hi, lo = np.zeros((N_OUT[fn], x.shape[1])), np.zeros((N_OUT[fn], x.shape[1]))
    with mp.workprec(PREC):
        for i in range(x.shape[1]):
            for k, v in enumerate(_exact(fn, x[:, i])):
                hi[k, i] = float(v)
                lo[k, i] = float(v - mp.mpf(hi[k, i]))
    return hi, lo


def errors(fn, got):
    """dict: abs, rel, ulp, each [N_OUT[fn], n], of `got` against reference(fn).  An ulp is that of the exact value's binade;
    where the exact value is 0 (log 1) the relative measures are 0 for an exact 0 and infinite otherwise."""
    hi, lo = reference(fn)
    got = np.asarray(got, np.float64)
    assert got.shape == hi.shape and np.isfinite(got).all(), fn
    err = np.abs((got - hi) - lo)
    m, e = np.frexp(np.abs(hi))
    below = (m == 0.5) & (np.sign(lo) == -np.sign(hi))                  # |exact| just under a power of two: the binade below
    ulp = np.ldexp(1.0, e - 53 - below)
    zero = hi == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(zero, np.where(err == 0.0, 0.0, np.inf), err / np.abs(hi))
        ulps = np.where(zero, np.where(err == 0.0, 0.0, np.inf), err / ulp)
    return dict(abs=err, rel=rel, ulp=ulps)


def check(fn, got, where):
    """prints the worst error of every output of `fn` with the point it occurs at, then holds it to its bar"""
    x, e = _points(fn), errors(fn, got)
    worst = []
    for k, (measure, bar) in enumerate(BARS[fn]):
        i = int(np.argmax(e[measure][k]))
        name = fn if N_OUT[fn] == 1 else f"{fn} {OUTPUTS[fn][k]}"
        at = ", ".join(float(v).hex() for v in x[:, i])
        print(f"[math {where}] {name}: worst {measure} error {e[measure][k, i]:.4g} (bar {bar:.4g}) at {at}, {x.shape[1]} points")
        worst.append((name, measure, e[measure][k, i], bar))
    if fn == "atan_b":
        small = np.abs(x[0]) < 0.5
        print(f"[math {where}] atan_b: worst ulp error for |t| < 0.5 {e['ulp'][0, small].max():.4g} (reported, no claim)")
    for name, measure, value, bar in worst:
        assert value <= bar, f"{name}: {measure} error {value:.6g} above the bar {bar:.6g}"
