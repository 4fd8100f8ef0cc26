"""The transport kernel's OWN square roots, divisions and trigonometric forms, one at a time, on a real MI355X.

test_math_and_rng_bit_parity (test_gpu_parity.py) evaluates include/mcs_math.h in csrc/mcs_population.hip, which is built
without MCS_DEVICE_FAST_SQRT and never calls rcp_refined / div_r / fdiv, sincos_t / asin_t or the tail loop's *_k forms.  Here
mcs_eval_fn's codes from "sqrt_fast" on run mcs_k_eval_hot, a kernel INSIDE csrc/mcs_transport.hip that calls the functions the
particle loop calls with the coefficient tables the particle loop fills, and mcs_eval_scatter runs one whole scatter in the
three spellings of the kernel (common pass, lossy kernel / tail ring, tail loop).

Every comparison is bit equality: against correctly rounded IEEE arithmetic (numpy's float64 sqrt and division) and against the
CPU oracle (whose own accuracy tests/test_math.py pins to mpmath).  Inputs are a directed edge set plus 2 x 10^5 random draws
per function; nothing is filtered -- the domain of an assertion is itself asserted of the inputs -- and no n is a multiple of
the block size of 256, so the `i < n` guard always has work."""
import ctypes as ct
from fractions import Fraction

import numpy as np
import pytest

from conftest import mcs, make_problem, oracle_backend, hip_backend, fuzz_problem, bits

pytestmark = pytest.mark.gpu

N_RANDOM = 200_000
PIO2_HI, PIO2_LO = 1.5707963267948966, 6.123233995736766e-17        # pi/2 as a double-double (MCS_PIO2_DD_0/1)
PI, TWOPI = 3.141592653589793, 6.283185307179586
SIN_UL = float(np.nextafter(1.0, 0.0))                              # MCS_SIN_UPPER_LIMIT
SQRT_LO = 2.0 ** -767       # below it the compiler's own sqrt sequence rescales its argument (include/mcs_math.h)
dp = ct.POINTER(ct.c_double)


@pytest.fixture(scope="module")
def be():
    prob = make_problem(64)
    hb, ob = hip_backend(prob), oracle_backend(prob)
    yield hb, ob
    hb.destroy(); ob.destroy()


def oev(ob, fn, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64); b = a if b is None else np.ascontiguousarray(b, dtype=np.float64)
    out = np.zeros_like(a)
    assert ob.lib.orc_eval_fn(mcs.capi.FN[fn], len(a), a.ctypes.data_as(dp), b.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    return out


def u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# (neighbours and nearest_multiples are also in tests/test_math.py, which builds the same edge sets: change both together)
def neighbours(x, k=1):
    """x and its k neighbours on either side, for every x"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo = np.nextafter(lo, -np.inf); hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def cat(*parts):
    a = np.concatenate([np.atleast_1d(np.asarray(p, dtype=np.float64)) for p in parts])
    if len(a) % 256 == 0:
        a = np.concatenate([a, a[:1]])
    return a


def assert_bits(got, ref, what, *args):
    assert got.shape == ref.shape
    bad = np.flatnonzero(u64(got) != u64(ref))
    if len(bad):
        show = [tuple(float(a[i]).hex() for a in args) + (float(got[i]).hex(), float(ref[i]).hex()) for i in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} results differ; (arguments..., device, reference): {show}")


def nearest_multiples(ks, step_hi, step_lo):
    """the doubles nearest k * (step_hi + step_lo), by exact rational arithmetic"""
    s = Fraction(step_hi) + Fraction(step_lo)
    return np.array([float(int(k) * s) for k in ks], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# square roots
def sqrt_edges(lo_exp, hi_exp, top):
    """Directed arguments in {0} u [2^lo_exp, top]: every power of two and its neighbours, perfect squares and theirs, the values
    around 1, and what K1 passes: (1 - |x|) / 2 for x -> 1 (down to 2^-54) and 1 - c^2 for c -> 1 (down to ~1.1e-16, and 0)."""
    rng = np.random.default_rng(11)
    top_p2 = np.array([top, np.nextafter(top, 0.0)])                   # the ends of the domain with their inner neighbour only
    p2 = np.concatenate([neighbours(np.ldexp(1.0, np.arange(lo_exp + 1, hi_exp))), [2.0 ** lo_exp, np.nextafter(2.0 ** lo_exp, 1.0)], top_p2])
    ints = np.concatenate([np.arange(2, 1025), rng.integers(1025, 2 ** 26, 2000)]).astype(np.float64)
    sq = ints * ints                                                    # exact: below 2^52
    scales = (0, -52, -104) if top > 4 else (-52, -60, -104)            # (for the roots of a scatter: squares up to 1)
    sq = np.concatenate([sq * 2.0 ** k for k in scales])
    m = np.arange(0, 300, dtype=np.float64)
    x_to_1 = np.concatenate([1 - np.ldexp(1.0, -np.arange(1, 54)), 1 - m * 2.0 ** -53])
    c_to_1 = np.concatenate([1 - m * 2.0 ** -53, 1 - np.ldexp(1.0, -np.arange(1, 54)), 1 - rng.uniform(0, 1e-7, 2000)])
    k1 = np.concatenate([(1.0 - x_to_1) * 0.5, 1 - c_to_1 * c_to_1])
    return np.concatenate([[0.0, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 0.25, 0.5], p2, neighbours(sq), k1])


def check_sqrt(be, fn, x):
    hb, ob = be
    assert len(x) % 256 != 0
    g = hb.eval_fn(fn, x)
    assert_bits(g, np.sqrt(x), f"{fn} against the correctly rounded square root", x)
    assert_bits(g, oev(ob, "sqrt", x), f"{fn} against the oracle's sqrt", x)


def test_sqrt_fast_is_correctly_rounded(be):
    """mcsm::sqrt_ as the transport TU compiles it (MCS_DEVICE_FAST_SQRT: no exponent rescale), on 0, +inf and [2^-767, 2^1023]."""
    rng = np.random.default_rng(1)
    x = cat([np.inf], sqrt_edges(-767, 1023, 2.0 ** 1023),
            np.ldexp(rng.uniform(1, 2, N_RANDOM), rng.integers(-767, 1023, N_RANDOM)))
    assert np.all((x == 0) | np.isposinf(x) | ((x >= SQRT_LO) & (x <= 2.0 ** 1023)))
    check_sqrt(be, "sqrt_fast", x)


@pytest.mark.parametrize("fn", ["sqrt_nn", "sqrt_nn_k"])
def test_sqrt_nn_is_correctly_rounded(be, fn):
    """mcsm::sqrt_nn_ (the two roots of a scatter, asin_t) and the tail loop's sqrt_nn_k, on +-0 and [2^-767, 4]."""
    rng = np.random.default_rng(2)
    x = cat([-0.0], sqrt_edges(-767, 2, 4.0),
            np.ldexp(rng.uniform(1, 2, N_RANDOM // 2), rng.integers(-767, 2, N_RANDOM // 2)), rng.uniform(0, 1, N_RANDOM // 2))
    assert np.all((x == 0) | ((x >= SQRT_LO) & (x <= 4.0)))
    check_sqrt(be, fn, x)


SQRT_EXACT_LO = 2.0 ** -968


def test_sqrt_fast_below_the_rescale_threshold(be):
    """Below 2^-767 the compiler's own sequence rescales its argument by 2^256 and sqrt_ / sqrt_nn_ do not (the transport path
    takes no such root).  Down to 2^-968 that cannot change a bit, and this case asserts it: every intermediate of the
    unscaled iteration is the scaled one's times an exact power of two as long as none leaves the normal range, and the
    smallest, the remainder d = x - g^2, is a multiple of ulp(g)^2 = 2^(2 e_g - 104) >= 2^-1074 for x >= 2^-968, hence exact.
    Below 2^-968 d is rounded to the subnormal grid and the last bit may differ: nothing is asserted there (include/mcs_math.h
    says so).  Measured on an MI355X, 2000 draws per binary exponent: one-ulp
    differences from the correctly rounded root in the binades 2^-1022 .. 2^-1011 (9 % of the arguments at 2^-1022, 0.05 % at
    2^-1014), none from 2^-1010 up; for subnormal arguments the fast forms are simply wrong."""
    rng = np.random.default_rng(3)
    x = cat(neighbours(np.ldexp(1.0, np.arange(-967, -767))), [SQRT_EXACT_LO, np.nextafter(SQRT_EXACT_LO, 1.0), np.nextafter(SQRT_LO, 0.0)],
            np.ldexp(rng.uniform(1, 2, N_RANDOM), rng.integers(-968, -767, N_RANDOM)))
    assert np.all((x >= SQRT_EXACT_LO) & (x < SQRT_LO)) and len(x) % 256 != 0
    for fn in ("sqrt_fast", "sqrt_nn", "sqrt_nn_k"):
        assert_bits(be[0].eval_fn(fn, x), np.sqrt(x), f"{fn} on [2^-968, 2^-767)", x)


def test_hypot1_in_the_transport_unit(be):
    """mcsm::hypot1 with the fast square root (gam_pf after an in-line loss): t = p / mc from 1e-6 to 1e12 and the edges of 1 + t^2."""
    hb, ob = be
    rng = np.random.default_rng(4)
    t = cat([0.0, 1.0, 1e-6, 1e12, 2.0 ** -26, 2.0 ** -27, 2.0 ** -53], neighbours(np.ldexp(1.0, np.arange(-30, 41))),
            10 ** rng.uniform(-6, 12, N_RANDOM))
    g = hb.eval_fn("hypot1_hot", t)
    assert_bits(g, np.sqrt(1.0 + t * t), "hypot1_hot against sqrt(1 + t*t)", t)
    assert_bits(g, oev(ob, "hypot1", t), "hypot1_hot against the oracle", t)


# ---------------------------------------------------------------------------------------------------------------------------
# divisions
def hard_quotients(rng, n):
    """Operands whose exact quotient lies 1/(2 b) of an ulp beside a rounding tie -- as close as two doubles get: integers
    A, B < 2^53 with A * 2^53 = Q * B + (B +- 1) / 2, i.e. A / B = 2^-53 (Q + 1/2 +- 1/(2B))."""
    a, b = [], []
    while len(a) < n:
        B = int(rng.integers(2 ** 52, 2 ** 53)) | 1
        inv = pow(B, -1, 2 ** 53)
        for R in ((B + 1) // 2, (B - 1) // 2):
            Q = (-R * inv) % 2 ** 53
            if Q < 2 ** 52:
                continue
            A, rem = divmod(Q * B + R, 2 ** 53)
            assert rem == 0 and A < 2 ** 53
            a.append(float(A)); b.append(float(B))
    return np.array(a), np.array(b)


def div_inputs():
    rng = np.random.default_rng(5)
    n = N_RANDOM
    # powers of two
    e = np.arange(-330, 331, 6)
    pa, pb = [v.ravel() for v in np.meshgrid(e, e)]
    keep = np.abs(pa - pb) <= 330
    A, B = [np.ldexp(1.0, pa[keep])], [np.ldexp(1.0, pb[keep])]
    # exactly representable quotients: q and b of 26 bits each, a = q * b exact
    q = rng.integers(1, 2 ** 26, 4000).astype(np.float64) * np.ldexp(1.0, rng.integers(-60, 60, 4000))
    b = rng.integers(1, 2 ** 26, 4000).astype(np.float64) * np.ldexp(1.0, rng.integers(-60, 60, 4000)) * rng.choice([-1.0, 1.0], 4000)
    A.append(q * b); B.append(b)
    # one ulp either side of q * b for random q and b
    q = np.ldexp(rng.uniform(1, 2, 20000), rng.integers(-40, 40, 20000)); b = np.ldexp(rng.uniform(1, 2, 20000), rng.integers(-40, 40, 20000))
    qb = q * b
    A += [qb, np.nextafter(qb, np.inf), np.nextafter(qb, -np.inf)]; B += [b, b, b]
    # quotients right beside a rounding tie, at several magnitudes
    ha, hb_ = hard_quotients(rng, 4000)
    for sa, sb in ((0, 0), (-185, -132), (-60, 40), (200, -100)):
        A.append(np.ldexp(ha, sa)); B.append(np.ldexp(hb_, sb))
    # 0 / b, both signs of b
    zb = 10 ** rng.uniform(-100, 100, 500) * rng.choice([-1.0, 1.0], 500)
    A.append(np.zeros(500)); B.append(zb)
    # CGS momenta over masses
    A.append(10 ** rng.uniform(-41, -39, 5000)); B.append(10 ** rng.uniform(-25, -23, 5000))
    # the call sites' magnitudes (see test_fdiv_is_correctly_rounded)
    for (alo, ahi), (blo, bhi) in [((9, 21), (9, 24)), ((-20, -6), (-20, -6)), ((-24, 0), (-8.1, 0)), ((-7, 13), (-18, -8)),
                                   ((-11, 16), (-28, -18)), ((0, 0), (-28, -18)), ((-20, -6), (0, 6)), ((-20, -6), (-17, -13)),
                                   ((0.79, 0.8), (1, 4)), ((-9, 13), (1, 4))]:
        A.append(10 ** rng.uniform(alo, ahi, 2000) * rng.choice([-1.0, 1.0], 2000)); B.append(10 ** rng.uniform(blo, bhi, 2000))
    # random draws over the asserted domain
    la = rng.uniform(-99.9, 99.9, n)                                   # log10 |a|, then log10 |a / b| such that b is in the domain too
    lq = rng.uniform(np.maximum(-99.9, la - 99.9), np.minimum(99.9, la + 99.9))
    a = 10 ** la * rng.choice([-1.0, 1.0], n)
    b = 10 ** (la - lq) * rng.choice([-1.0, 1.0], n)
    A.append(a); B.append(b)
    a, b = np.concatenate(A), np.concatenate(B)
    if len(a) % 256 == 0:
        a, b = a[:-1], b[:-1]
    return a, b


def in_div_domain(a, b):
    q = np.abs(a / b)
    return np.all((np.abs(b) >= 1e-100) & (np.abs(b) <= 1e100) &
                  ((a == 0) | ((np.abs(a) >= 1e-100) & (np.abs(a) <= 1e100) & (q >= 1e-100) & (q <= 1e100))))


def test_fdiv_is_correctly_rounded(be):
    """fdiv(a, b) = div_r(a, b, rcp_refined(b)) against IEEE division, for |a|, |b|, |a / b| in [1e-100, 1e100] and 0 / b.

    The divisions of the transport path and their operands (CGS; m = aa m_p from 9.1e-28 g to ~1e-22 g, p = ptot_pf from
    ~1e-3 m_e c = 2.7e-20 to ~1e6 m_p c = 5e-8 g cm/s, B from 1e-6 G to ~50 G so gyro_denom = 1/(qB) from 4e7 to 2e15):
      refresh_scatter_k  fdiv(6 vp_tg, xn_per lam)       12 pi r_g over xn_per eta r_g: r_g = p c / (qB) 1e9..1e21 cm, quotient 1e-3..4
      scattering_rest    div_r(pb_pf | p_perp, ptot_pf)  |a| <= b = p (2.7e-20..5e-8); p_perp / p is 0 or >= 1e-8
      scattering_rest    fdiv(ssd, sin_new)              sin(phi_scat) sin_d: 0 or 1e-24..1, over sin_new: 1e-8..1 (0: NaN, discarded)
      refresh_dtest_k    fdiv(r_g p, m gam u2)           1e9..1e21 x p = 1e-11..1e13 over m gam u2 = 1e-18..1e-8
      move               div_r(pb_pf t_step, gam m)      p x (1e-4..1e11 s) over gam m = 9e-28..1e-18; rg_val = rcp_refined(gam m)
      in-line loss       fdiv(ptot, 1 + dlnp)            p over 1.01..1e6
                         fdiv(ptot, mc)                  p over mc = 2.7e-17..5e-14
                         fdiv(ptot, ptot_old)            p over p, quotient in (0, 1)
                         div_r(2 pi | gyro_period, xn_per)   6.28 or 1e-9..1e13 s over xn_per = 10..1e4, one reciprocal for both
    All of them lie tens of decades inside the asserted domain."""
    hb, _ = be
    a, b = div_inputs()
    assert len(a) % 256 != 0 and len(a) > N_RANDOM and in_div_domain(a, b)
    assert_bits(hb.eval_fn("fdiv", a, b), a / b, "fdiv against IEEE division", a, b)


def test_div_r_with_a_shared_reciprocal(be):
    """div_r(a, b, r) and div_r(2a, b, r) with ONE r = rcp_refined(b): the first is a / b, the second exactly twice that."""
    hb, _ = be
    a, b = div_inputs()
    fits = (np.abs(2 * a) <= 1e100) & (np.abs(2 * a / b) <= 1e100)
    a = np.where(fits, a, a / 4)                                        # (2a stays inside the domain; nothing is dropped)
    assert in_div_domain(a, b) and in_div_domain(2 * a, b)
    q1, q2 = hb.eval_fn("div_r", a, b), hb.eval_fn("div_r2", a, b)
    assert_bits(q1, a / b, "div_r against IEEE division", a, b)
    assert_bits(q2, 2 * q1, "div_r(2a, b, r) against twice div_r(a, b, r)", a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# sincos_t, asin_t / asin_tk, mod2pi_k
def test_sincos_t_against_the_oracle(be):
    """sincos_t (coefficients from HotCoef, negations as sign-bit flips) against the oracle's sin and cos, sign of zero included."""
    hb, ob = be
    rng = np.random.default_rng(6)
    ks = np.concatenate([np.arange(-40, 41), rng.integers(-63661, 63662, 3000)])
    U = np.array([0.0, 2.0 ** -53, 1 - 2.0 ** -53])
    x = cat(neighbours(nearest_multiples(ks, PIO2_HI, PIO2_LO)), [0.0, -0.0, PI, -PI, TWOPI, -TWOPI], U * TWOPI - PI,
            [1e-300, 2.0 ** -27, 2.0 ** -26, -1e-300, -2.0 ** -27, -2.0 ** -26], rng.uniform(-1e5, 1e5, N_RANDOM))
    assert np.all(np.abs(x) < 1e5) and len(x) % 256 != 0
    assert_bits(hb.eval_fn("sin_t", x), oev(ob, "sin", x), "sin of sincos_t against the oracle", x)
    assert_bits(hb.eval_fn("cos_t", x), oev(ob, "cos", x), "cos of sincos_t against the oracle", x)


@pytest.mark.parametrize("fn", ["asin_t", "asin_tk"])
def test_asin_forms_against_the_oracle(be, fn):
    hb, ob = be
    rng = np.random.default_rng(7)
    to1 = 1 - np.ldexp(1.0, -np.arange(1, 53))
    x = cat(neighbours([0.5, -0.5], 3), [SIN_UL, -SIN_UL, 1.0, -1.0, 0.0, -0.0, 1e-300, -1e-300], to1, -to1, rng.uniform(-1, 1, N_RANDOM))
    assert np.all(np.abs(x) <= 1) and len(x) % 256 != 0
    assert_bits(hb.eval_fn(fn, x), oev(ob, "asin", x), f"{fn} against the oracle's asin", x)


def test_mod2pi_k_against_the_oracle(be):
    hb, ob = be
    rng = np.random.default_rng(8)
    ks = np.concatenate([np.arange(-30, 31), rng.integers(-15900, 15901, 3000)])
    inside = rng.uniform(0, TWOPI, 5000)
    inside = inside[inside < TWOPI]
    x = cat(neighbours(nearest_multiples(ks, 4 * PIO2_HI, 4 * PIO2_LO), 2), inside, [TWOPI, np.nextafter(TWOPI, 0.0), 0.0],
            -np.ldexp(1.0, -np.arange(1, 61)), rng.uniform(-1e5, 1e5, N_RANDOM))
    assert np.all(np.abs(x) < 1e5) and len(x) % 256 != 0
    g = hb.eval_fn("mod2pi_k", x)
    assert_bits(g, oev(ob, "mod2pi", x), "mod2pi_k against the oracle's mod2pi", x)
    assert np.all((g >= 0) & (g < TWOPI))
    already = (x >= 0) & (x < TWOPI)
    assert already.sum() >= len(inside) and np.array_equal(u64(g[already]), u64(x[already]))      # Base.mod2pi returns x itself


def test_unknown_fn_is_an_error(be):
    hb, _ = be
    a = np.ones(5); out = np.full(5, 7.0)
    for fn in (len(mcs.capi.FN), 9999, -1):
        assert hb.lib.mcs_eval_fn(hb.h, fn, len(a), a.ctypes.data_as(dp), a.ctypes.data_as(dp), out.ctypes.data_as(dp)) != 0
        assert b"unknown fn" in hb.lib.mcs_last_error()
    assert np.all(out == 7.0)
    assert hb.lib.mcs_eval_scatter(hb.h, 3, 0, a.ctypes.data_as(dp), out.ctypes.data_as(dp)) != 0
    assert b"unknown form" in hb.lib.mcs_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# one scatter as a unit
N_STATES = 100_000
KEY, IDX, AA, GD, PTOT, GAM, XN, PB, PPERP, PHI = range(10)
OUT_NAMES = ["pb_pf", "p_perp", "phi", "gyro_period", "cos_max"]


def scatter_states(prob, aa, p_lo, p_hi, seed):
    """N_STATES states of species aa: random ones with ptot_pf log-uniform in [p_lo, p_hi], and the directed ones in front."""
    rng = np.random.default_rng(seed)
    P = prob.params
    n = N_STATES + 3
    mc = aa * mcs.constants.MP * mcs.constants.C
    s = np.zeros((n, 10))
    s[:, KEY] = rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64)
    s[:, IDX] = 2.0 * rng.integers(0, 2 ** 31, n)
    s[:, AA] = aa
    s[:, GD] = 1.0 / (mcs.constants.QCGS * 10 ** rng.uniform(-6, 2, n))
    s[:, PTOT] = 10 ** rng.uniform(np.log10(p_lo), np.log10(p_hi), n)
    s[:, GAM] = np.sqrt(1.0 + (s[:, PTOT] / mc) ** 2)
    s[:, XN] = np.where(rng.random(n) < 0.5, P.xn_per_fine, P.xn_per_coarse)
    s[:, PB] = s[:, PTOT] * rng.uniform(-1, 1, n)
    s[:, PPERP] = np.sqrt(np.maximum(s[:, PTOT] ** 2 - s[:, PB] ** 2, 0.0))
    s[:, PHI] = rng.uniform(0, TWOPI, n)
    # directed states (every one accepted by the oracle; none had to be taken out):
    d = 0
    for sign in (1.0, -1.0):
        for xn in (P.xn_per_fine, P.xn_per_coarse, 1e18, 1e20):   # 12 pi / xn_per < 2^-53 from 3.4e17 on: cos_max rounds to 1, sin_d == 0
            for idx in (0.0, 2.0 ** 32 - 2):
                # pitch at the pole: with cos_max == 1 also sin_new == 0 -- the NaN quotient must be discarded, phi stays finite
                s[d, PB] = sign * s[d, PTOT]; s[d, PPERP] = 0.0; s[d, XN] = xn; s[d, IDX] = idx; d += 1
                # p_perp one ulp above 0
                s[d, PB] = sign * s[d, PTOT]; s[d, PPERP] = 5e-324; s[d, XN] = xn; s[d, IDX] = idx; d += 1
                # an ordinary pitch with the degenerate cone, phi at 0 and just below 2 pi
                s[d, XN] = xn; s[d, IDX] = idx; s[d, PHI] = 0.0 if sign > 0 else np.nextafter(TWOPI, 0.0); d += 1
    for phi in (0.0, float(np.nextafter(TWOPI, 0.0))):
        for idx in (0.0, 2.0 ** 32 - 2):
            s[d, PHI] = phi; s[d, IDX] = idx; d += 1
    assert d < 64 and n % 256 != 0
    return s


def check_scatter(prob, states):
    hb, ob = hip_backend(prob), oracle_backend(prob)
    try:
        ref = ob.eval_scatter(states)
        assert np.all(np.isfinite(ref)), "the oracle's own result is not finite"
        got = [hb.eval_scatter(form, states) for form in (0, 1, 2)]
    finally:
        hb.destroy(); ob.destroy()
    for form, g in enumerate(got):
        for c, name in enumerate(OUT_NAMES):
            assert_bits(g[:, c], ref[:, c], f"form {form}: {name} against the oracle", *(states[:, k] for k in range(1, 10)))
    for form in (1, 2):
        assert np.array_equal(bits(got[form]), bits(got[0])), f"form {form} differs from form 0"
    return ref


def test_scatter_forms_protons():
    """refresh_scatter + scattering(), the lossy kernel's spelling and the tail loop's, on 10^5 proton states: bit-equal to the
    oracle in pb_pf, p_perp, phi, gyro_period and cos_max, and to each other."""
    prob = make_problem(64)
    mc = mcs.constants.MP * mcs.constants.C
    states = scatter_states(prob, 1.0, 1e-3 * mc, 1e6 * mc, 21)
    ref = check_scatter(prob, states)
    degenerate = states[:, XN] >= 1e18
    assert degenerate.sum() == 24 and np.all(ref[degenerate, 4] == 1.0)    # the cone really closed: cos_max == 1
    pole = (states[:, PPERP] == 0) & (states[:, XN] >= 1e18)
    assert pole.sum() == 8 and np.all(ref[pole, 1] == 0.0)                 # sin_new == 0: the discarded quotient


def test_scatter_forms_electrons_around_pe_crit():
    """The same for electrons with momenta on both sides of pe_crit (the branch of refresh_scatter that freezes the mean free path)."""
    prob, aa = fuzz_problem("electrons", 64)
    pe = prob.params.pe_crit
    assert aa < 1 and pe > 0
    states = scatter_states(prob, aa, 1e-2 * pe, 1e3 * pe, 22)
    below = states[:, PTOT] < pe
    assert 0.3 < below.mean() < 0.5
    check_scatter(prob, states)
