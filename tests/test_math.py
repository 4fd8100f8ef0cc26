"""include/mcs_math.h (the deterministic elementary functions shared by the oracle's
det mode and the HIP kernels) against glibc libm: accuracy in ulps and exact identities --
and, at the directed edges that tests/test_gpu_math_forms.py compares the device forms with
the oracle at, against mpmath: that pins the reference those bit comparisons lean on."""
import ctypes as ct
from fractions import Fraction

import numpy as np
import pytest

from conftest import mcs, orc

dp = ct.POINTER(ct.c_double)


def ev(lib, fn, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a if b is None else np.ascontiguousarray(b, dtype=np.float64)
    out = np.zeros_like(a)
    assert lib.orc_eval_fn(mcs.capi.FN[fn], len(a), a.ctypes.data_as(dp), b.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    return out


def ulps(x, y):
    return np.abs(x.view(np.int64) - y.view(np.int64))


def test_accuracy_vs_libm():
    det, libm = orc.load("det", mcs.capi), orc.load("libm", mcs.capi)
    assert det.orc_math_mode() == b"det" and libm.orc_math_mode() == b"libm"
    rng = np.random.default_rng(7)
    n = 400_000
    cases = {
        # (sin, cos: the whole domain the header states for the Cody-Waite reduction, |x| < 1e5)
        "sin": (rng.uniform(-1e5, 1e5, n), None, 2), "cos": (rng.uniform(-1e5, 1e5, n), None, 2),
        "asin": (rng.uniform(-1, 1, n), None, 2), "acos": (rng.uniform(-1, 1, n), None, 2),
        "atan2": (rng.normal(size=n), rng.normal(size=n), 3), "log10": (10 ** rng.uniform(-40, 40, n), None, 2),
        "hypot1": (10 ** rng.uniform(-8, 12, n), None, 1), "sqrt": (10 ** rng.uniform(-60, 60, n), None, 0),
        "div": (rng.normal(size=n), rng.normal(size=n), 0),
    }
    for fn, (a, b, tol) in cases.items():
        d, l = ev(det, fn, a, b), ev(libm, fn, a, b)
        assert ulps(d, l).max() <= tol, (fn, int(ulps(d, l).max()))


def test_exact_values():
    det = orc.load("det", mcs.capi)
    z = np.array([0.0])
    assert ev(det, "sin", z)[0] == 0.0 and ev(det, "cos", z)[0] == 1.0
    assert ev(det, "asin", np.array([1.0]))[0] == np.pi / 2 and ev(det, "asin", np.array([-1.0]))[0] == -np.pi / 2
    assert ev(det, "acos", np.array([1.0]))[0] == 0.0
    assert ev(det, "log10", np.array([1.0]))[0] == 0.0
    assert ev(det, "atan2", np.array([0.0]), np.array([1.0]))[0] == 0.0
    # prevfloat(1.0), the clamp of src/scattering.jl:3, is a legal asin argument
    assert np.isfinite(ev(det, "asin", np.array([np.nextafter(1.0, 0.0)]))[0])


def test_mod2pi_range_and_identity():
    det = orc.load("det", mcs.capi)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1e5, 1e5, 200_000)                            # the header's stated domain
    r = ev(det, "mod2pi", x)
    assert np.all(r >= 0) and np.all(r < 2 * np.pi)
    inside = rng.uniform(0, 6.28, 1000)
    assert np.array_equal(ev(det, "mod2pi", inside), inside)       # Base.mod2pi returns x itself in [0, 2pi)
    k = np.rint((x - r) / (2 * np.pi))
    # (k * 2 pi in extended precision: at |x| ~ 1e5 a float64 product is itself off by 1e-11)
    twopi = 4 * np.longdouble(PIO2_HI) + 4 * np.longdouble(PIO2_LO)
    assert np.finfo(np.longdouble).nmant >= 63
    assert np.max(np.abs(x.astype(np.longdouble) - k.astype(np.longdouble) * twopi - r.astype(np.longdouble))) < 1e-13


# ---- the directed edges against mpmath ---------------------------------------------------------------------------------
PIO2_HI, PIO2_LO = 1.5707963267948966, 6.123233995736766e-17        # pi/2 as a double-double (MCS_PIO2_DD_0/1)
TWOPI = 6.283185307179586
TAN_PIO8 = float.fromhex("0x1.a827999fcef32p-2")                     # the switch of atan2
SQRT_HALF = float.fromhex("0x1.6a09e667f3bcdp-1")                    # the mantissa switch of log10


# (neighbours and nearest_multiples are also in tests/test_gpu_math_forms.py, which builds the same edge sets: change both together)
def neighbours(x, k=1):
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo = np.nextafter(lo, -np.inf); hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def nearest_multiples(ks, step_hi, step_lo):
    s = Fraction(step_hi) + Fraction(step_lo)
    return np.array([float(int(k) * s) for k in ks], dtype=np.float64)


def ulp_errors(mp, got, exact):
    """|got - exact| in ulps of the exact value (an exact 0 allows only 0)"""
    out = []
    for g, e in zip(got, exact):
        if e == 0:
            out.append(0.0 if g == 0 else np.inf)
            continue
        ulp = mp.ldexp(1, int(mp.floor(mp.log(abs(e), 2))) - 52)
        out.append(float(abs(mp.mpf(float(g)) - e) / ulp))
    return np.array(out)


def test_directed_edges_against_mpmath():
    """The oracle's det functions at the edge sets of the GPU form tests (plus acos, atan2, log10) against mpmath at 250 bits:
    less than 2 ulp of the exact value, the header's bound; mod2pi within 4 ulp(2 pi) absolutely -- next to a multiple of
    2 pi no relative bound can hold."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.prec = 250
    det = orc.load("det", mcs.capi)
    rng = np.random.default_rng(17)
    f = mp.mpf

    ks = np.concatenate([np.arange(-40, 41), rng.integers(-63661, 63662, 300)])
    U = np.array([0.0, 2.0 ** -53, 1 - 2.0 ** -53])
    trig = np.concatenate([neighbours(nearest_multiples(ks, PIO2_HI, PIO2_LO)), [0.0, np.pi, -np.pi, TWOPI, -TWOPI], U * TWOPI - np.pi,
                           [1e-300, 2.0 ** -27, 2.0 ** -26]])
    to1 = 1 - np.ldexp(1.0, -np.arange(1, 53))
    arc = np.concatenate([neighbours([0.5, -0.5], 3), [np.nextafter(1.0, 0.0), -np.nextafter(1.0, 0.0), 1.0, -1.0, 0.0, 1e-300], to1, -to1])
    e10 = np.arange(-1000, 1001)
    logs = np.concatenate([np.ldexp(m, e10) for m in neighbours([SQRT_HALF], 2)] + [[10.0 ** k for k in range(23)]])
    worst = {}
    for fn, x, ref in (("sin", trig, mp.sin), ("cos", trig, mp.cos), ("asin", arc, mp.asin), ("acos", arc, mp.acos),
                       ("log10", logs, mp.log10)):
        err = ulp_errors(mp, ev(det, fn, x), [ref(f(float(v))) for v in x])
        worst[fn] = float(err.max())
        assert err.max() < 2, (fn, float(x[err.argmax()]).hex(), float(err.max()))

    # atan2: the tan(pi/8) switch, |y| = |x|, both signs of both arguments
    mag = np.concatenate([neighbours([TAN_PIO8], 3), [1.0], neighbours([1.0], 2), [1e-300, 1e-10, 0.1, 0.3, 0.5, 0.9]])
    ys, xs = [], []
    for scale in (1.0, 3.7e-14, 2.5e9):
        for sy in (1.0, -1.0):
            for sx in (1.0, -1.0):
                ys += [sy * mag * scale, sy * np.full_like(mag, scale)]; xs += [sx * np.full_like(mag, scale), sx * mag * scale]
    y, x = np.concatenate(ys), np.concatenate(xs)
    err = ulp_errors(mp, ev(det, "atan2", y, x), [mp.atan2(f(float(a)), f(float(b))) for a, b in zip(y, x)])
    worst["atan2"] = float(err.max())
    assert err.max() < 2, ("atan2", float(y[err.argmax()]).hex(), float(x[err.argmax()]).hex(), float(err.max()))

    # mod2pi: the doubles nearest k * 2 pi and two neighbours each side, values inside, the ends, small negatives
    ks = np.concatenate([np.arange(-30, 31), rng.integers(-15900, 15901, 300)])
    x = np.concatenate([neighbours(nearest_multiples(ks, 4 * PIO2_HI, 4 * PIO2_LO), 2), rng.uniform(0, TWOPI, 200),
                        [TWOPI, np.nextafter(TWOPI, 0.0), 0.0], -np.ldexp(1.0, -np.arange(1, 61))])
    r = ev(det, "mod2pi", x)
    two_pi = 2 * mp.pi
    exact = [f(float(v)) - mp.floor(f(float(v)) / two_pi) * two_pi for v in x]
    # (the distance on the circle: right below a multiple of 2 pi the exact value is 2 pi - tiny, and the nearest double
    # to that may be the double 2 pi itself, which mod2pi folds to 0)
    d = [abs(f(float(g)) - e) for g, e in zip(r, exact)]
    absd = np.array([float(min(v, two_pi - v)) for v in d])
    worst["mod2pi"] = float(absd.max())
    assert absd.max() <= 4 * np.spacing(TWOPI), ("mod2pi", float(x[absd.argmax()]).hex(), float(absd.max()))
    assert np.all((r >= 0) & (r < TWOPI))
    print("largest errors against mpmath [ulp; mod2pi absolute]:", worst)


def test_atan2_signed_zeros():
    """mpmath has no signed zero: the IEEE / Julia values of atan(y, x) at the zeros, bit for bit (atan(-0.0, -1.0) == -pi)."""
    det = orc.load("det", mcs.capi)
    pi, h = np.pi, np.pi / 2
    cases = [(0.0, 1.0, 0.0), (-0.0, 1.0, -0.0), (0.0, -1.0, pi), (-0.0, -1.0, -pi),
             (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (0.0, -0.0, pi), (-0.0, -0.0, -pi),
             (1.0, 0.0, h), (1.0, -0.0, h), (-1.0, 0.0, -h), (-1.0, -0.0, -h),
             (5e-324, 1.0, 5e-324), (-5e-324, 1.0, -5e-324), (2.5, 2.5, pi / 4), (-2.5, 2.5, -pi / 4), (2.5, -2.5, 3 * pi / 4),
             (-2.5, -2.5, -3 * pi / 4)]
    y, x, want = (np.array(c) for c in zip(*cases))
    got = ev(det, "atan2", y, x)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), list(zip(y, x, got, want))
