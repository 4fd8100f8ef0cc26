"""Helpers of the term-by-term tests of the three photon folds (test_photon_folds_host.py, test_gpu_photon_folds.py): K5
mcs_k_photon_synch, K6 mcs_k_photon_ic, K7 mcs_k_photon_pion and their CPU twins.

The reference: ONE term of each fold, written from the Julia text the headers cite (src/synch_emission.jl:112-171 with
src/photon_synch.jl:45-52; src/inverse_compton.jl:232-308; src/pion_kafexhiu.jl:171-241 with src/KATV2014.jl), with the quirks
P1-P3 and I1-I3 of include/mcs_pion.h and include/mcs_ic.h, in mpmath at 50 digits on the same double inputs.  It shares no code
with include/mcs_synch.h, mcs_ic.h or mcs_pion.h; the two Chebyshev fits of the first synchrotron function are evaluated in
mpmath from include/mcs_synch_coeffs.inc, read as data.

The bound: every reference value carries a running bound of |fp64 evaluation - exact value| (class `V`).  The model of the fp64
side is: every + - * / sqrt is correctly rounded (2^-53 relative; the libraries are built without contraction, and a fused
operation would only round once less), every libm call returns within L_f ulps of the exact function of its (already inexact)
argument, and the argument's error goes through the function itself: |f(a +- e) - f(a)|, evaluated in mpmath (all five
functions are monotone in each argument).  The bound therefore covers the cancellations by itself: 1 - X at the kinematic limit
of the pion fold, the Jones bracket at q -> 1, exp(-x) at x -> 30.  The products of two errors are kept, so the bound is a
true one for the model, not a first-order estimate of it.

L_f, inputs that are not fitted to anything measured here:
  GLIBC  -- the glibc manual, "Known Maximum Errors in Math Functions", x86_64, double: cbrt 4, exp 1, log 1, pow 1, hypot 1.
  DEVICE -- the ROCm documentation's table of double-precision device functions is part of the online documentation and not of
            a ROCm installation's files, and was not at hand: 2 ulp for each of the five, an ASSUMPTION, recorded in DESIGN.md.

A discrete decision (a cut or a branch of the Julia text) is UNDECIDABLE at a point when the reference's interval straddles
it; such points are left out of the value and mask comparisons and counted (at most 0.1 % of a test's lit points).
"""
import math
import os
import re

import mpmath
import numpy as np

from conftest import ROOT, mcs

mp = mpmath.mp.clone()
mp.dps = 50
MPF = mp.mpf
U = 2.0 ** -53

GLIBC = dict(cbrt=4, exp=1, log=1, pow=1, hypot=1)
DEVICE = dict(cbrt=2, exp=2, log=2, pow=2, hypot=2)
UNDECIDABLE_CAP = 1.0e-3

C, ME, MPROT, QCGS = mcs.constants.C, mcs.constants.ME, mcs.constants.MP, mcs.constants.QCGS
HBAR, MEV, GEV = 1.054571817e-27, 1.602176634e-6, 1.602176634e-3
PI = 3.141592653589793                  # the double the Julia `pi` becomes in a Float64 expression
E_REL_PT = 0.005                        # parameters.jl:32
TTH, MRES, GRES, MPI0, MPC2 = 0.2797, 1.1883, 0.2264, 0.134976, 0.93827208816        # constants.jl:16-22; P2


# ---- a value with its running error bound ----------------------------------------------------------------------------------------
class Model:
    """The libm of the side under test (one of GLIBC, DEVICE)."""
    L = GLIBC


def use_libm(L):
    Model.L = L


class libm:
    """with libm(DEVICE): ... -- the bounds inside are the device's"""
    def __init__(self, L):
        self.L = L

    def __enter__(self):
        self.old, Model.L = Model.L, self.L

    def __exit__(self, *a):
        Model.L = self.old


def _v(x):
    return x if isinstance(x, V) else V(MPF(x), 0.0)


class V:
    """r: the exact value (mpmath) of an expression of double inputs; e: a bound of |its fp64 evaluation - r| (a Python float)."""
    __slots__ = ("r", "e")

    def __init__(self, r, e=0.0):
        self.r, self.e = r, float(e)

    @staticmethod
    def _rounded(r, e):
        return V(r, e + U * (float(abs(r)) + e))

    def __add__(self, o):
        o = _v(o)
        return V._rounded(self.r + o.r, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = _v(o)
        return V._rounded(self.r - o.r, self.e + o.e)

    def __rsub__(self, o):
        return _v(o) - self

    def __neg__(self):
        return V(-self.r, self.e)

    def __mul__(self, o):
        o = _v(o)
        a, b = float(abs(self.r)), float(abs(o.r))
        return V._rounded(self.r * o.r, a * o.e + b * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _v(o)
        r = self.r / o.r
        low = float(abs(o.r)) - o.e
        if low <= 0:
            raise ZeroDivisionError("divisor's interval holds zero")
        return V._rounded(r, (self.e + float(abs(r)) * o.e) / low)

    def __rtruediv__(self, o):
        return _v(o) / self


def sqrt(a):
    a = _v(a)
    r = mp.sqrt(a.r)
    lo = a.r - a.e
    return V._rounded(r, float(r - (mp.sqrt(lo) if lo > 0 else 0)) if a.e else 0.0)


def _libm(name, f, a):
    """A monotone function of one argument: the argument's error through f itself, then L_f ulps (1 ulp <= 2^-52 |f|)."""
    r = f(a.r)
    ep = float(max(abs(f(a.r + a.e) - r), abs(f(a.r - a.e) - r))) if a.e else 0.0
    return V(r, ep + Model.L[name] * 2 * U * (float(abs(r)) + ep))


def exp(a):
    return _libm("exp", mp.exp, _v(a))


def log(a):
    a = _v(a)
    if a.r - a.e <= 0:
        raise ValueError("log: the argument's interval reaches zero")
    return _libm("log", mp.log, a)


def cbrt(a):
    return _libm("cbrt", mp.cbrt, _v(a))


def hypot1(a):
    """hypot(a, 1.0)"""
    return _libm("hypot", lambda t: mp.sqrt(t * t + 1), _v(a))


def power(a, b):
    """pow(a, b), a >= 0: monotone in either argument, so the corners of the box bound the propagated error."""
    a, b = _v(a), _v(b)
    f = lambda x, y: mp.power(x, y) if x > 0 else (MPF(0) if y > 0 else MPF("inf"))
    r = f(a.r, b.r)
    ep = 0.0
    if a.e or b.e:
        xs = (max(a.r - a.e, MPF(0)), a.r + a.e)
        ys = (b.r - b.e, b.r + b.e)
        ep = float(max(abs(f(x, y) - r) for x in xs for y in ys))
    return V(r, ep + Model.L["pow"] * 2 * U * (float(abs(r)) + ep))


class Decisions:
    """The discrete decisions of one point: each is taken on the exact values and is undecidable when the interval of the
    difference holds zero (exact inputs on either side decide exactly, equality included)."""
    def __init__(self):
        self.undecidable = False

    def _cmp(self, a, b):
        a, b = _v(a), _v(b)
        d, tol = a.r - b.r, a.e + b.e
        if tol > 0 and abs(d) <= tol:
            self.undecidable = True
        return d

    def lt(self, a, b):
        return self._cmp(a, b) < 0

    def le(self, a, b):
        return self._cmp(a, b) <= 0

    def gt(self, a, b):
        return self._cmp(a, b) > 0

    def ge(self, a, b):
        return self._cmp(a, b) >= 0


class Point:
    """The reference at one output: value r with bound e, whether the output is above the floor, the branch it took."""
    __slots__ = ("r", "e", "lit", "undecidable", "branch")

    def __init__(self, val, lit, undecidable, branch):
        self.r, self.e, self.lit, self.undecidable, self.branch = val.r, val.e, lit, undecidable, branch


FLOOR = V(MPF(1.0e-99))


# ---- K5: one term of synch_emission! ----------------------------------------------------------------------------------------------
def _read_coeffs():
    text = open(os.path.join(ROOT, "include", "mcs_synch_coeffs.inc")).read()
    num = r"[-+]?[0-9.]+(?:[eE][-+]?[0-9]+)?"
    defs = {k: float(v) for k, v in re.findall(r"#define\s+MCS_SYNCH_(\w+)\s+(" + num + r")\s", text)}
    tabs = {k: [float(x) for x in re.findall(num, body)] for k, body in re.findall(r"MCS_SYNCH_(\w+)\[\d+\]\s*=\s*\{([^}]*)\}", text)}
    assert len(tabs["SMALL"]) == defs["SMALL_N"] and len(tabs["LARGE"]) == defs["LARGE_N"]
    return defs, tabs


CHEB_DEFS, CHEB = _read_coeffs()
SYNCH_X0 = CHEB_DEFS["X0"]


def _clenshaw(c, t):
    b1, b2 = _v(0.0), _v(0.0)
    for j in range(len(c) - 1, 0, -1):
        b1, b2 = 2 * t * b1 - b2 + c[j], b1
    return t * b1 - b2 + 0.5 * c[0]


def synch_F(D, x):
    """The fit of F(x) = x int_x^inf K_5/3 the fold evaluates -> (value, "F_small" | "F_large")."""
    if D.le(x, SYNCH_X0):
        v = cbrt(x)
        return v * _clenshaw(CHEB["SMALL"], 2 * (v * v) / CHEB_DEFS["WMAX"] - 1), "F_small"
    s, a, b = 1 / x, CHEB_DEFS["SMIN"], _v(1) / SYNCH_X0
    return sqrt(PI * x / 2) * exp(-x) * _clenshaw(CHEB["LARGE"], (2 * s - (a + b)) / (b - a)), "F_large"


def synch_F_exact(x, bessel=False):
    """mpmath's own x int_x^inf K_5/3(t) dt.  K_nu(t) = int_0^inf exp(-t cosh u) cosh(nu u) du, so the integral over t is
    int_0^inf exp(-x cosh u) cosh(5 u / 3) / cosh u du, an integral of elementary functions (cut where the exponent passes
    -150 + ...); bessel=True: the integral of mpmath's besselk itself (slow; the host test holds the two against each other)."""
    x = MPF(x)
    if bessel:
        return x * mp.quad(lambda t: mp.besselk(MPF(5) / 3, t), [x, x + 1, x + 10, x + 80])
    top = mp.acosh(1 + 150 / x)
    cuts = [top * k / 8 for k in range(9)]
    return x * mp.quad(lambda u: mp.exp(-x * mp.cosh(u)) * mp.cosh(5 * u / 3) / mp.cosh(u), cuts)


def synch_bin(d, p_lo, p_hi, B, mc):
    """What one electron bin contributes at every photon energy -> term(E_erg) -> Point."""
    D0 = Decisions()
    skip = None
    if B < 1.0e-20:
        skip = "B<1e-20"
    else:
        p_fac = sqrt(3.0) / (2 * PI) * (_v(QCGS) * QCGS * QCGS * B / (_v(ME) * C * C))                  # synch_emission.jl:60
        xN = _v(1.0e-99) if d <= 1.0e-99 else _v(d) * (_v(p_hi) - p_lo)                                # photon_synch.jl:45-52
        p = sqrt(_v(p_lo) * p_hi)
        if D0.le(xN, 1.0e-60):
            skip = "xN<=1e-60"
        elif D0.lt(p * C, 3 * _v(MEV)):                                                                # :130
            skip = "pc<3MeV"
        else:
            ge = hypot1(p / mc)
            w_c = 3 * ge * ge * QCGS * B / (2 * _v(mc))
            if D0.lt(w_c, 1.0e-55):
                skip = "w_c<1e-55"

    def term(E):
        D = Decisions()
        D.undecidable = D0.undecidable
        if skip:
            return Point(FLOOR, False, D.undecidable, "skip:" + skip)
        w_g = _v(E) / HBAR
        x = w_g / w_c
        if D.ge(x, 30.0):
            return Point(FLOOR, False, D.undecidable, "skip:x>=30")
        if D.lt(x, 1.0e-15):
            return Point(FLOOR, False, D.undecidable, "skip:x<1e-15")
        F, branch = synch_F(D, x)
        add = xN * w_g * p_fac * F
        if not D.gt(add, 1.0e-55):
            return Point(FLOOR, False, D.undecidable, "skip:add<=1e-55")
        return Point(FLOOR + add, True, D.undecidable, branch)
    return term


# ---- K6: one term of IC_emission_FCJ ---------------------------------------------------------------------------------------------
def ic_cone_count(col, p_lo, p_hi, j_max):
    """The electrons of one momentum bin inside the cone: photon_IC's conversion (inverse_compton.jl:54-61) and the sum over the
    angle rows 0..j_max (:235-238) -- a numpy sum in row order (np.cumsum adds sequentially), taken as an exact double -> the
    count, or None for a bin the fold skips (no row above 1e-99)."""
    dp = p_hi - p_lo
    c = np.where(col[:j_max + 1] <= 1.0e-99, 1.0e-99, col[:j_max + 1] * dp)
    return None if c.max() <= 1.0e-99 else float(np.cumsum(c)[-1])


def ic_bin(col, p_lo, p_hi, mc_e, j_max, beam_area):
    """One electron bin (column `col` of the zone's d2N/dp dcos over the angle rows) -> term(E_erg, alpha_in[], n_in[]) -> Point:
    the incoming photon bins in order (one bin: ONE term of the fold), then the flux conversion of :285-308."""
    D0 = Decisions()
    xn = ic_cone_count(col, p_lo, p_hi, j_max)
    t = sqrt(_v(p_lo) * p_hi) / mc_e
    slow = D0.lt(t, E_REL_PT)                                                                           # :240-241
    g = _v(1.0) if slow else sqrt(t * t + 1.0)
    mec2 = _v(ME) * C * C
    r0 = _v(QCGS) * QCGS / mec2                                                                         # :217
    tag = "gamma=1" if slow else "gamma>1"

    def term(E, alpha_in, n_in):
        D = Decisions()
        D.undecidable = D0.undecidable
        if xn is None or not xn > 0:
            return Point(FLOOR, False, D.undecidable, "skip:empty")
        ao = _v(E) / mec2                                    # the energy the call reports, in units of m_e c^2
        if D.ge(ao, g):                                                                                 # :262
            return Point(FLOOR, False, D.undecidable, "skip:alpha_out>=g," + tag)
        acc, n_add, qmax = FLOOR, 0, MPF(0)
        for a1, n1 in zip(alpha_in, n_in):
            a1 = _v(float(a1))
            norm_fac = _v(float(n1)) * 2 * PI * (r0 * r0) * C / (a1 * (g * g))                          # :252
            q = ao / (4 * a1 * (g * g) * (1 - ao / g))                                                  # :265
            tt = a1 * g * q
            br = 2 * q * log(q) + (1 + 2 * q) * (1 - q) + 8 * (tt * tt) * (1 - q) / (1 + 4 * a1 * g * q)      # :268-271
            cur = norm_fac * xn * br
            if D.gt(cur, 1.0e-60):                                                                      # :275-277
                acc, n_add, qmax = acc + cur, n_add + 1, max(qmax, q.r)
        if not n_add:
            return Point(FLOOR, False, D.undecidable, "skip:cur<=1e-60," + tag)
        e = ao * mec2
        v = acc / beam_area / mec2 * (e * e)                                                            # :285-308
        if D.le(v, 1.0e-55):
            return Point(FLOOR, False, D.undecidable, "skip:flux<=1e-55," + tag)
        return Point(v, True, D.undecidable, ("q>0.9," if qmax > 0.9 else "q<=0.9,") + tag)
    return term


# ---- K7: one term of pion_kafexhiu -----------------------------------------------------------------------------------------------
def pion_sigma_inel(Tp):
    ratio = Tp / TTH
    lr = log(ratio)
    t = 1 - power(ratio, -1.9)
    return (30.7 - 0.96 * lr + 0.18 * lr * lr) * (t * t * t)


def pion_sigma_pi(D, Tp, i_data, s, Td=None):
    """KATV2014.jl:22-111 -> (sigma [mb], branch).  Td: the value the branches are decided on (pion_bin), T_p itself if None."""
    Td = Tp if Td is None else Td
    if D.lt(Td, 2):
        g4 = MRES * sqrt(_v(MRES) * MRES + _v(GRES) * GRES)
        K = sqrt(8.0) * MRES * GRES * g4 / (PI * sqrt(_v(MRES) * MRES + g4))
        rs = sqrt(s)
        d = (rs - MPC2) * (rs - MPC2) - _v(MRES) * MRES
        fBW = MPC2 * K / (d * d + _v(MRES) * MRES * GRES * GRES)
        a, b = s - _v(MPI0) * MPI0 - 4 * _v(MPC2) * MPC2, 4 * _v(MPI0) * MPC2
        eta = sqrt(a * a - b * b) / (2 * MPI0 * rs)
        s1 = 7.66e-3 * power(eta, 1.95) * (1 + eta + power(eta, 5.0)) * power(fBW, 1.86)
        if D.lt(Td, 2 * _v(TTH)):
            return s1 + 0.0, "sig<2Tth"
        return s1 + 5.7 / (1 + exp(-9.3 * (Tp - 1.4))), "sig<2"
    if D.lt(Td, 5):
        Q = (Tp - TTH) / MPC2
        return (-6.0e-3 + 0.237 * Q - 0.023 * Q * Q) * pion_sigma_inel(Tp), "sig<5"
    a1, a2, a3, a4, a5, br = 0.728, 0.596, 0.491, 0.2503, 0.117, "sig>=5"
    if i_data == 2 and D.gt(Td, 50.0):
        a1, a2, a3, a4, a5, br = 0.652, 0.0016, 0.488, 0.1928, 0.483, "sig>50,d2"
    elif i_data == 3 and D.gt(Td, 100.0):
        a1, a2, a3, a4, a5, br = 5.436, 0.254, 0.072, 0.075, 0.166, "sig>100,d3"
    elif i_data == 4 and D.gt(Td, 100.0):
        a1, a2, a3, a4, a5, br = 0.908, 0.0009, 6.089, 0.176, 0.448, "sig>100,d4"
    xi = (Tp - 3) / MPC2
    n_pi0 = a1 * power(xi, a4) * (1 + exp(-(a2 * power(xi, a5)))) * (1 - exp(-(a3 * power(xi, 0.25))))
    return n_pi0 * pion_sigma_inel(Tp), br


def pion_amax(D, Tp, i_data, s, sigma, Td=None):
    """KATV2014.jl:229-296 -> (E_gamma^max, A_max, branch)"""
    Td = Tp if Td is None else Td
    rs = sqrt(s)
    E_pi = (s - 4 * _v(MPC2) * MPC2 + _v(MPI0) * MPI0) / (2 * rs)
    g_cm = (Tp + 2 * _v(MPC2)) / rs
    b_cm = sqrt(1 - 1 / (g_cm * g_cm))
    P_pi = sqrt(E_pi * E_pi - _v(MPI0) * MPI0)
    Emax_pi = g_cm * (E_pi + P_pi * b_cm)
    g_lab = Emax_pi / MPI0
    b_lab = sqrt(1 - 1 / (g_lab * g_lab))
    Eg_max = _v(MPI0) / 2 * g_lab * (1 + b_lab)
    if D.lt(Td, 1):
        return Eg_max, 5.9 * sigma / Emax_pi, "A<1"
    b1, b2, b3, br = 9.13, 0.35, 0.0097, "A,else"
    if i_data == 1 and D.lt(Td, 5):
        b1, b2, b3, br = 9.53, 0.52, 0.054, "A<5,d1"
    elif i_data == 2 and D.gt(Td, 50):
        b1, b2, b3, br = 9.06, 0.3795, 0.01105, "A>50,d2"
    elif i_data == 3 and D.gt(Td, 100):
        b1, b2, b3, br = 10.77, 0.412, 0.01264, "A>100,d3"
    elif i_data == 4 and D.gt(Td, 100):
        b1, b2, b3, br = 13.16, 0.4419, 0.01439, "A>100,d4"
    th = Tp / MPC2
    lt = log(th)
    return Eg_max, b1 * power(th, -b2) * sigma / MPC2 * exp(b3 * lt * lt), br


def pion_F(D, Tp, Eg, i_data, Eg_max, Td=None):
    """KATV2014.jl:136-212 with P1 -> (F, branch); F is exactly 0 outside 0 <= X <= 1."""
    Td = Tp if Td is None else Td
    Y = Eg + _v(MPI0) * MPI0 / Eg
    Ymax = Eg_max + _v(MPI0) * MPI0 / Eg_max
    X = (Y - MPI0) / (Ymax - MPI0)
    if D.lt(X, 0) or D.gt(X, 1):
        return None, "X>1"
    if D.lt(Td, 1):
        kappa = 3.29 - 0.2 * power(Tp / MPC2, -1.5)
        return power(1 - X, kappa), "F<1"
    if D.lt(Td, 20):
        q = (Tp - 1) / MPC2
        mu = 1.25 * power(q, 1.25) * exp(-1.25 * q)
        if D.lt(Td, 4):
            lam, al, be, ga, br = 3.0, 1.0, mu + 2.45, mu + 1.45, "F<4"
        else:
            lam, al, be, ga, br = 3.0, 1.0, 1.5 * mu + 4.95, mu + 1.5, "F<20"
    elif i_data == 1 and D.gt(Td, 100):
        lam, al, be, ga, br = 3.0, 0.5, 4.9, 1.0, "F>100,d1"
    elif i_data == 2 and D.gt(Td, 50):
        lam, al, be, ga, br = 3.5, 0.5, 4.0, 1.0, "F>50,d2"
    elif i_data == 3 and D.gt(Td, 100):
        lam, al, be, ga, br = 3.55, 0.5, 3.6, 1.0, "F>100,d3"
    elif i_data == 4 and D.gt(Td, 100):
        lam, al, be, ga, br = 3.55, 0.5, 4.5, 1.0, "F>100,d4"
    else:
        lam, al, be, ga, br = 3.0, 0.5, 4.2, 1.0, "F,else"
    Cc = lam * MPI0 / Ymax
    return power(1 - power(X, al), be) / power(1 + X / Cc, ga), br


def pion_Tp_f64(p_lo, p_hi, mc, aa):
    """T_p per nucleon [GeV] of a bin AS THE FP64 SIDE HOLDS IT: pion_kafexhiu.jl:171-186 is five + - * / sqrt on the inputs and no
    libm call, every one correctly rounded on the host and on the device (no contraction), so Python floats give the same bits.
    The branches of the parametrisation (T_p against 0.2797, 0.5594, 1, 2, 4, 5, 20, 50, 100) are decided on this value: they
    are never undecidable, and a bin whose T_p IS a branch point pins < against <=."""
    gam = math.sqrt(1 + (p_lo * p_hi) / (mc * mc))
    Tp = (gam - 1) * (aa * MPC2)
    return Tp / aa


def pion_bin(d, p_lo, p_hi, mc, aa, i_data, n_t, scaling):
    """One momentum bin of a nucleus species (pion_kafexhiu.jl:171-193, photon_pion_decay.jl:86-92) -> term(E_erg) -> Point."""
    D0 = Decisions()
    floor = FLOOR * scaling
    skip = branch0 = None
    if d <= 1.0e-99:
        skip = "empty"
    else:
        cnt = _v(d) * (_v(p_hi) - p_lo)
        if D0.le(cnt, 1.0e-99):
            skip = "count<=1e-99"
        else:
            p2 = _v(p_lo) * p_hi
            gam = sqrt(1 + p2 / (_v(mc) * mc))
            Tp = (gam - 1) * (_v(aa) * MPC2) / aa                                                       # P2
            vel = sqrt(p2) / (gam * aa * MPROT)
            Td = _v(pion_Tp_f64(p_lo, p_hi, mc, aa))
            assert abs(Td.r - Tp.r) <= Tp.e
            if D0.lt(Td, TTH):
                skip = "Tp<Tth"
            else:
                s = 2 * _v(MPC2) * (Tp + 2 * _v(MPC2))
                sig, bs = pion_sigma_pi(D0, Tp, i_data, s, Td)
                Eg_max, Amax, ba = pion_amax(D0, Tp, i_data, s, sig, Td)
                pref = _v(n_t) * cnt * vel
                branch0 = bs + "|" + ba
                if not pref.r > 0:
                    skip = "pref<=0"

    def term(E):
        D = Decisions()
        D.undecidable = D0.undecidable
        if skip:
            return Point(floor, False, D.undecidable, "skip:" + skip)
        Eg = _v(E) / GEV
        F, bf = pion_F(D, Tp, Eg, i_data, Eg_max, Td)
        if F is None:
            return Point(floor, False, D.undecidable, "skip:" + bf)
        sig_tot = Amax * F * Eg
        rate = pref * (sig_tot * 1.0e-27)
        acc = FLOOR + rate * E
        if D.lt(acc, 1.0e-99):
            return Point(FLOOR, False, D.undecidable, "skip:acc<1e-99")
        out = acc * scaling
        lit = D.gt(out, floor)
        return Point(out, lit, D.undecidable, branch0 + "|" + bf)
    return term


# ---- comparing an output array with the reference --------------------------------------------------------------------------------
class Tally:
    """Worst |error| / bound per branch, the undecidable share of the lit points, and what failed."""
    def __init__(self, what):
        self.what, self.worst, self.count, self.n, self.n_lit, self.n_und, self.bad = what, {}, {}, 0, 0, 0, []

    def add(self, out, pt, floor, where):
        self.n += 1
        self.n_lit += bool(pt.lit or out > floor)
        if pt.undecidable:
            self.n_und += 1
            return
        err = abs(MPF(float(out)) - pt.r)
        if pt.e == 0.0:
            ratio = 0.0 if err == 0 else math.inf
        else:
            ratio = float(err / pt.e)
        self.worst[pt.branch] = max(self.worst.get(pt.branch, 0.0), ratio)
        self.count[pt.branch] = self.count.get(pt.branch, 0) + 1
        if ratio > 1.0 or bool(out > floor) != bool(pt.lit):
            self.bad.append((where, pt.branch, float(out), float(pt.r), pt.e, ratio))

    def report(self):
        print(f"{self.what}: {self.n} points, {self.n_lit} lit, {self.n_und} undecidable; worst |error| / bound per branch:")
        for k in sorted(self.worst):
            print(f"    {k:40s} {self.worst[k]:.3f}   ({self.count[k]} points)")

    def check(self, min_lit=1, branches=()):
        """branches: prefixes of branch names that must have been met at decidable points (each side of every cut aimed at)"""
        self.report()
        for b in branches:
            assert any(k.startswith(b) or ("|" + b) in k for k in self.count), (self.what, "no decidable point took", b)
        assert not self.bad, (self.what, len(self.bad), self.bad[:5])
        assert self.n_lit >= min_lit, (self.what, self.n_lit)
        assert self.n_und <= UNDECIDABLE_CAP * self.n_lit, (self.what, self.n_und, self.n_lit)


def lit_bin_of(row):
    """The one lit bin of an impulse row (None: an empty zone)."""
    k = np.flatnonzero(row > 1.0e-99)
    assert len(k) <= 1
    return int(k[0]) if len(k) else None


def check_synch(tally, d, pe, btot, mc, E, out, tag="", js=None):
    """Every output of an impulse call of K5 against its term; empty zones hold the floor exactly."""
    for z in range(d.shape[0]):
        i = lit_bin_of(d[z])
        if i is None:
            assert np.all(out[z] == 1.0e-99), (tag, z)
            continue
        term = synch_bin(float(d[z, i]), float(pe[i]), float(pe[i + 1]), float(btot[z + 1]), mc)
        for j in (range(len(E)) if js is None else js):
            tally.add(out[z, j], term(float(E[j])), 1.0e-99, (tag, z, i, j))


def check_pion(tally, d, pe, mc, aa, target, scaling, i_data, E, out, tag="", js=None):
    for z in range(d.shape[0]):
        i = lit_bin_of(d[z])
        if i is None:
            assert np.all(out[z] == 1.0e-99 * scaling), (tag, z)
            continue
        term = pion_bin(float(d[z, i]), float(pe[i]), float(pe[i + 1]), mc, aa, i_data, float(target[z]), scaling)
        for j in (range(len(E)) if js is None else js):
            tally.add(out[z, j], term(float(E[j])), 1.0e-99 * scaling, (tag, z, i, j))


def check_ic(tally, d2n, pe, mc_e, j_max, alpha_in, n_in, beam_area, E, out, tag="", js=None):
    """d2n: the [n_grid][NT][NM] array the fold read, with at most one lit momentum bin per zone inside the cone."""
    for z in range(d2n.shape[0]):
        lit = np.flatnonzero((d2n[z, :j_max + 1, :-1] > 1.0e-99).any(axis=0))
        assert len(lit) <= 1
        if not len(lit):
            assert np.all(out[z] == 1.0e-99), (tag, z)
            continue
        i = int(lit[0])
        term = ic_bin(d2n[z, :, i], float(pe[i]), float(pe[i + 1]), mc_e, j_max, beam_area)
        for j in (range(len(E)) if js is None else js):
            tally.add(out[z, j], term(float(E[j]), alpha_in, n_in), 1.0e-99, (tag, z, i, j))


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def impulse_spectra(n_grid, n_bins, weight, dark_every=9):
    """One lit momentum bin per zone, a different bin in every zone, swept until every bin 0..n_bins-1 was lit once; every
    `dark_every`-th zone stays empty, and the sweep's first call lights the first grid zone, its last call the last one.
    weight(bin) -> dN/dp of the lit bin.  -> list of [n_grid][n_bins + 1] arrays (the last column is never read)."""
    calls, b = [], 0
    while b < n_bins:
        d = np.full((n_grid, n_bins + 1), 1.0e-99)
        for z in range(n_grid):
            if b >= n_bins or (z % dark_every == dark_every - 1 and z != n_grid - 1):
                continue
            d[z, b] = weight(b)
            b += 1
        calls.append(d)
    last = calls[-1]
    if last[n_grid - 1].max() <= 1.0e-99:                       # light the last zone as well, with a bin of the last call
        z = int(np.flatnonzero((last > 1.0e-99).any(axis=1))[-1])
        last[[z, n_grid - 1]] = last[[n_grid - 1, z]]
    assert calls[0][0].max() > 1.0e-99 and calls[-1][n_grid - 1].max() > 1.0e-99
    return calls


def edges_for(p_targets, n_edges, width=1.0e-3):
    """A crafted edge grid: bin 2k has the geometric-mean momentum p_targets[k] (to an ulp or two), the odd bins between them are
    fillers that stay dark (the folds read a bin's own two edges only, so the grid need not be monotone) -> (edges, lit bins)."""
    assert 2 * len(p_targets) + 1 <= n_edges
    pe = np.zeros(n_edges)
    bins = []
    for k, p in enumerate(p_targets):
        lo = float(p) * (1 - width)
        hi = float(MPF(float(p)) ** 2 / MPF(lo))
        pe[2 * k], pe[2 * k + 1] = lo, hi
        bins.append(2 * k)
    rest = 2 * len(p_targets)
    top = max(float(max(p_targets)) * 2, 1.0)
    pe[rest:] = top * (1 + np.arange(n_edges - rest))
    return pe, bins


def ladder(p0, offsets=(2.0 ** -44, 1.0e-9, 1.0e-3)):
    """momenta on either side of p0: an ulp-scale neighbourhood (256 ulps) and two coarser relative offsets"""
    return [p0 * (1 + s * o) for o in offsets for s in (-1, 1)]


def solve(f, target, lo, hi, iters=200):
    """p in [lo, hi] with f(p) = target for a monotone f of exact values (bisection in double, geometric)"""
    flo = f(lo) - target
    for _ in range(iters):
        mid = math.sqrt(lo * hi)
        if mid <= lo or mid >= hi:
            break
        fm = f(mid) - target
        if (fm < 0) == (flo < 0):
            lo, flo = mid, fm
        else:
            hi = mid
    return lo


def dense_spectrum(rng, n_grid, n_edges, lit_share=0.6, floors=(1.0e-60, 1.0e-99)):
    """A random subset of lit bins per zone, weights over 40 decades, some at the 1e-99 and 1e-60 input floors, every fifth zone dark."""
    d = np.full((n_grid, n_edges), 1.0e-99)
    for z in range(n_grid):
        if z % 5 == 4:
            continue
        lit = rng.random(n_edges - 1) < lit_share
        w = 10.0 ** rng.uniform(0, 40, n_edges - 1)
        d[z, :-1] = np.where(lit, w, 1.0e-99)
        for f in floors:
            d[z, rng.integers(0, n_edges - 1, 2)] = f
    return d


def ordered_sum(terms, floor=1.0e-99):
    """floor followed by the terms added in order, as the folds do: np.cumsum adds sequentially (np.sum adds pairwise)"""
    return np.cumsum(np.concatenate([[floor], np.asarray(terms, dtype=np.float64)]))[-1]


# every branch a threshold test must have met at decidable points: each side of every cut it aims at
K5_BRANCHES = ("F_small", "F_large", "skip:pc<3MeV", "skip:x>=30", "skip:x<1e-15", "skip:xN<=1e-60", "skip:add<=1e-55")
K6_BRANCHES = ("q<=0.9,gamma=1", "q<=0.9,gamma>1", "q>0.9,gamma>1", "skip:alpha_out>=g,gamma=1", "skip:alpha_out>=g,gamma>1", "skip:cur<=1e-60,gamma>1")
K7_BRANCHES = ("sig<2Tth", "sig<2|", "sig<5", "sig>=5", "sig>50,d2", "sig>100,d3", "sig>100,d4", "A<1", "A<5,d1", "A,else", "A>50,d2", "A>100,d3",
               "A>100,d4", "F<1", "F<4", "F<20", "F,else", "F>100,d1", "F>50,d2", "F>100,d3", "F>100,d4", "skip:Tp<Tth", "skip:X>1")


# ---- the scenarios: the same calls and the same points for the CPU twin and for the device -----------------------------------------
ELECTRON = mcs.inputs.Species(ME / MPROT, -1.0, 1e6, 1.0)
B_FLAT = 3.0e-3
SYNCH_GRID = (14, 1.0e-16, 0.5)            # (n_photon, emin [MeV], bins per decade): x from below 1e-15 to above 30 over the momentum grid
PION_GRID = (20, 1.0, 2)                   # 1 MeV .. 3e6 GeV
PION_GRID_THR = (8, 10.0, 1)               # 10 MeV .. 1e5 GeV
IC_GRID = (10, 1.0e-9, 0.5)


def synch_problem(flat=True, **binning):
    """Electrons in a flat field of 3 mG; flat=False: zone 40 below the 1e-20 cut, zones 41-43 one ulp below, at and one ulp above
    it, zones 44-49 around the field at which w_c of a slow electron of mass SYNCH_HEAVY_MC passes 1e-55."""
    from conftest import make_problem
    prob = make_problem(16, species=[ELECTRON], b_field_turbulence=1.0, B_mag_upstream=B_FLAT, **binning)
    bt = np.full_like(np.asarray(prob.btot, dtype=np.float64), B_FLAT)
    if not flat:
        bt[1 + 40] = 1.0e-21
        bt[1 + 41:1 + 44] = (np.nextafter(1.0e-20, 0.0), 1.0e-20, np.nextafter(1.0e-20, 1.0))
        bt[1 + 44:1 + 50] = ladder(SYNCH_B_WC)
    prob.btot = bt
    return prob


SYNCH_B_WC = 1.5e-20
SYNCH_HEAVY_MC = 3 * QCGS * SYNCH_B_WC / (2 * 1.0e-55)          # w_c = 3 gamma^2 q B / (2 mc) = 1e-55 at gamma = 1


def _count_weight(b):
    return 10.0 ** (10 + (7 * b) % 40)


def _crafted(ng, NM, pairs):
    """pairs (p, particle count of the bin) dealt to calls of one lit bin per zone on crafted edge grids -> [(edges, dndp)]"""
    per_call = min(ng, (NM - 1) // 2)
    calls = []
    for r in range(0, len(pairs), per_call):
        chunk = pairs[r:r + per_call]
        pe, bins = edges_for([p for p, _ in chunk], NM)
        d = np.full((ng, NM), 1.0e-99)
        for z, (b, (_, cnt)) in enumerate(zip(bins, chunk)):
            d[z, b] = cnt / (pe[b + 1] - pe[b])
        calls.append((pe, d))
    return calls


def synch_threshold_pairs(mc, E):
    """Crafted (momentum, count) pairs of K5 in the flat field: p c = 3 MeV; x = 30, x = X0 and x = 1e-15 at energies of the
    grid; xN = 1e-60 and add = 1e-55 by the count."""
    B = B_FLAT
    p_of_x = lambda x, e: mc * math.sqrt(2 * mc * e / (3 * x * HBAR * QCGS * B) - 1)
    pairs = [(p, 1.0e30) for p in ladder(3 * MEV / C)]
    for x, js in ((30.0, (3, 6)), (SYNCH_X0, (3, 6)), (1.0e-15, (0, 2))):
        for j in js:
            pairs += [(p, 1.0e30) for p in ladder(p_of_x(x, float(E[j])))]
    p_gen = 1.0e-12
    pairs += [(p_gen, c) for c in ladder(1.0e-60)]
    for j in (2, 5):                                            # add = 1e-55 at energy j: from the term of a count of 1e30
        pe, _ = edges_for([p_gen], 4)
        unit = synch_bin(1.0e30 / (pe[1] - pe[0]), pe[0], pe[1], B, mc)(float(E[j]))
        assert unit.lit
        pairs += [(p_gen, c) for c in ladder(float(1.0e-25 / (unit.r - MPF(1.0e-99))))]
    return pairs


def synch_term_by_term(be, prob, what, part):
    """K5, every output against its term.  part "impulses": the sweep over the problem's own momentum grid; "thresholds": the
    crafted edge grids."""
    tabs = mcs.consumers.consumer_tables(prob, 1)
    pe, mc, ng = tabs.mom_edge_cgs, tabs.mc, prob.params.n_grid
    n_photon, emin, bpd = SYNCH_GRID
    T = Tally(what + " " + part)
    if part == "impulses":
        for c, d in enumerate(impulse_spectra(ng, len(pe) - 1, lambda b: _count_weight(b) / (pe[b + 1] - pe[b]))):
            E, out = be.photon_synch(d, pe, mc, n_photon, emin, bpd)
            check_synch(T, d, pe, prob.btot, mc, E, out, c)
        return T
    E = be.photon_synch(np.full((ng, len(pe)), 1.0e-99), pe, mc, n_photon, emin, bpd)[0]
    for c, (pc, d) in enumerate(_crafted(ng, len(pe), synch_threshold_pairs(mc, E))):
        E, out = be.photon_synch(d, pc, mc, n_photon, emin, bpd)
        check_synch(T, d, pc, prob.btot, mc, E, out, c)
    return T


def synch_field_cuts(be, prob_odd, what):
    """K5 on the problem of synch_problem(flat=False): B around 1e-20 and w_c around 1e-55 (a slow 'electron' of mass SYNCH_HEAVY_MC,
    photon energies low enough for x < 30); the zone below the cut holds the floor row, and no other lit zone does."""
    ng = prob_odd.params.n_grid
    NM = prob_odd.params.num_psd_mom_bins + 2
    pe, bins = edges_for([1.0e-3], NM)
    d = np.full((ng, NM), 1.0e-99)
    zones = [0, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, ng - 1]
    d[zones, bins[0]] = 1.0e59 / (pe[1] - pe[0])
    T = Tally(what + " field cuts")
    E, out = be.photon_synch(d, pe, SYNCH_HEAVY_MC, 6, 1.0e-82, 1)
    check_synch(T, d, pe, prob_odd.btot, SYNCH_HEAVY_MC, E, out, "heavy")
    E2, out2 = be.photon_synch(d, pe, ME * C, *SYNCH_GRID)
    check_synch(T, d, pe, prob_odd.btot, ME * C, E2, out2, "electron")
    floor_rows = np.flatnonzero((out2 == 1.0e-99).all(axis=1))
    lit = set(zones) - set(floor_rows.tolist())
    assert lit == set(zones) - {40, 41}, lit                    # 1e-21 and the ulp below 1e-20; 1e-20 itself is not below the cut
    return T


def fold_sum_structure(call, d, n_bins, floor=1.0e-99, exact_above=0.0):
    """The dense output equals, bit for bit, the floor followed by the SAME back-end's impulse outputs added in bin order.
    call(dndp) -> out [n_grid][n_photon].  Impulse b: the dense spectrum with every column but b dark.  A term is what the impulse
    output holds above the floor; exact_above > 0: an impulse output between the floor and exact_above is floor + term rounded
    and not the term itself, and the (zone, energy) pairs with such a term are left out (-> their share)."""
    dense = call(d)
    terms = np.zeros((n_bins + 1,) + dense.shape)
    terms[0] = floor
    unsure = np.zeros(dense.shape, dtype=bool)
    for b in range(n_bins):
        if not np.any(d[:, b] > 1.0e-99):
            continue
        one = np.full_like(d, 1.0e-99)
        one[:, b] = d[:, b]
        o = call(one)
        dark = d[:, b] <= 1.0e-99
        assert np.all(o[dark] == floor)
        terms[b + 1] = np.where(o > floor, o, 0.0)
        unsure |= (o > floor) & (o < exact_above)
    want = np.cumsum(terms, axis=0)[-1]
    ok = ~unsure
    n_lit = int((dense > floor).sum())
    assert n_lit > 0.2 * dense.size, n_lit
    assert np.array_equal(dense[ok].view(np.uint64), want[ok].view(np.uint64)), (int((dense[ok] != want[ok]).sum()), n_lit)
    multi = (terms[1:] > 0).sum(axis=0)
    assert (multi > 10).sum() > 0.1 * dense.size               # sums of many terms, not impulses again
    return float(unsure.mean())


def large_problem():
    """The largest binning mcs_create accepts (nm = nt = 199: 201 entries in the kernels' 208-entry tables), in the flat field.  Its
    species are protons (an electron grid of the same bins per decade has more than 199 bins); the folds take the caller's edges
    and mass, so the electron folds run on it over `electron_edges`."""
    from conftest import make_problem
    import consumers_common as cc
    prob = make_problem(16, **cc.LARGE_BINNING)
    assert prob.params.num_psd_mom_bins == 199 and prob.params.num_psd_tht_bins == 199
    prob.btot = np.full_like(np.asarray(prob.btot, dtype=np.float64), B_FLAT)
    return prob


def electron_edges(n_edges):
    """electron momenta from below 3 MeV / c to gamma = 4e10"""
    return np.geomspace(2.0e-18, 1.0e-6, n_edges)


def synch_sum_structure(be, prob, seed=3, pe=None):
    tabs = mcs.consumers.consumer_tables(prob, 1)
    pe, mc = (tabs.mom_edge_cgs, tabs.mc) if pe is None else (pe, ME * C)
    d = dense_spectrum(np.random.default_rng(seed), prob.params.n_grid, len(pe))
    d[:, :-1] = np.where(d[:, :-1] > 1.0e-60, d[:, :-1] / np.diff(pe)[None, :], d[:, :-1])
    return fold_sum_structure(lambda x: be.photon_synch(x, pe, mc, *SYNCH_GRID)[1], d, len(pe) - 1)


def shapes_rows(call, sizes=(1, 255, 256, 257, 4096)):
    """call(n_photon) -> out [n_grid][n_photon] on one energy grid: row k of every size equals row k of the largest, bit for
    bit (the strided second pass over the workgroup's 256 threads gives what a first pass would)."""
    outs = {n: call(n) for n in sizes}
    big = outs[max(sizes)]
    assert (big > big.min()).sum() > 100
    for n, o in outs.items():
        assert o.shape[1] == n and np.array_equal(o.view(np.uint64), np.ascontiguousarray(big[:, :n]).view(np.uint64)), n
    return big


# -- K7
def pion_problem(**binning):
    from conftest import make_problem
    return make_problem(16, **binning)


def pion_target(ng):
    """target densities: equal in zones 0, 50 and the last one, different elsewhere"""
    t = 0.5 + 0.01 * np.arange(ng)
    t[[0, 50, ng - 1]] = 0.75
    return t


def p_of_Tp(Tp, mc):
    return mc * math.sqrt((Tp / MPC2 + 1) ** 2 - 1)


PION_TP = (0.2797, 0.5594, 1.0, 2.0, 4.0, 5.0, 20.0, 50.0, 100.0)
PION_TP_HIT = {1.0, 2.0, 4.0, 5.0, 20.0, 50.0, 100.0}      # met exactly by a bin of the iron-like species (pion_exact_hits)
PION_CASES = ((1.0, 1), (1.0, 2), (1.0, 3), (1.0, 4), (4.0, 1), (4.0, 3), (56.0, 1), (56.0, 4))       # (A, i_data)


def pion_Egmax_exact(p, mc, aa):
    """E_gamma^max [GeV] of a bin of geometric-mean momentum p: the exact value of the reference's expression"""
    D = Decisions()
    gam = sqrt(1 + _v(p) * p / (_v(mc) * mc))
    Tp = (gam - 1) * (_v(aa) * MPC2) / aa
    s = 2 * _v(MPC2) * (Tp + 2 * _v(MPC2))
    return pion_amax(D, Tp, 1, s, _v(1.0))[0].r


def pion_exact_hits(mc, aa, n_edges):
    """Bins whose fp64 T_p IS a branch point: for every branch point, edges around p(T_p) searched over neighbouring doubles
    -> (edges, lit bins, the branch points hit)"""
    los, his, hit = [], [], []
    for Tp in PION_TP[2:]:
        p = p_of_Tp(Tp, mc)
        found = None
        for a in range(48):
            lo = float(np.nextafter(p * (1 - 1.0e-3), 0.0) if a == 0 else np.nextafter(lo, 0.0))
            hi = float(MPF(p) ** 2 / MPF(lo))
            hi = float(hi - 200 * np.spacing(hi))
            for _ in range(400):
                if pion_Tp_f64(lo, hi, mc, aa) == Tp:
                    found = (lo, hi)
                    break
                hi = float(np.nextafter(hi, np.inf))
            if found:
                break
        if found:
            los.append(found[0]); his.append(found[1]); hit.append(Tp)
    pe = np.zeros(n_edges)
    bins = []
    for k, (lo, hi) in enumerate(zip(los, his)):
        pe[2 * k], pe[2 * k + 1] = lo, hi
        bins.append(2 * k)
    pe[2 * len(los):] = 1.0 + np.arange(n_edges - 2 * len(los))
    return pe, bins, hit


def pion_limit_pairs(mc, aa, E, js=(2, 3, 4, 5)):
    """momenta at which the kinematic limit X = 1 falls on photon energy j of the grid: E_gamma^max = E_j (upper end) and
    m_pi^2 / E_gamma^max = E_j (lower end, P1)"""
    pairs = []
    lo, hi = p_of_Tp(TTH * 1.0001, mc), p_of_Tp(1.0e7, mc)
    for j in js:
        Eg = float(E[j]) / GEV
        for tgt in (Eg, MPI0 * MPI0 / Eg):
            if float(pion_Egmax_exact(lo, mc, aa)) < tgt < float(pion_Egmax_exact(hi, mc, aa)):
                p0 = solve(lambda p: pion_Egmax_exact(p, mc, aa), MPF(tgt), lo, hi)
                pairs += [(p, 1.0e30) for p in ladder(p0)]
    return pairs


def pion_term_by_term(be, prob, what, part, cases=None):
    """K7, every output against its term.  part "impulses": the sweep over the problem's own momentum grid for protons (GEANT 4) and
    helium (PYTHIA 8); "thresholds": T_p on either side of every branch point of the parametrisation for the (A, i_data) of
    `cases`, and the kinematic limit X = 1 at both ends of the spectrum."""
    tabs = mcs.consumers.consumer_tables(prob, 1)
    pe, ng = tabs.mom_edge_cgs, prob.params.n_grid
    target = pion_target(ng)
    T2 = T = Tally(what + " " + part)
    if part == "impulses":
        for aa, i_data in ((1.0, 1), (4.0, 2)):
            mc = aa * MPROT * C
            for c, d in enumerate(impulse_spectra(ng, len(pe) - 1, lambda b: _count_weight(b) / (pe[b + 1] - pe[b]))):
                E, out = be.photon_pion(d, pe, mc, aa, target, 1.0, *PION_GRID, i_data)
                check_pion(T, d, pe, mc, aa, target, 1.0, i_data, E, out, (aa, c))
        return T
    n_photon, emin, bpd = PION_GRID_THR
    for aa, i_data in (PION_CASES if cases is None else cases):
        mc = aa * MPROT * C
        pairs = [(p, 1.0e30) for Tp in PION_TP for p in ladder(p_of_Tp(Tp, mc))]
        if i_data == 1:
            E = 10.0 ** (math.log10(emin * MEV) + np.arange(n_photon) / bpd)
            pairs += pion_limit_pairs(mc, aa, E)
        for c, (pc, d) in enumerate(_crafted(ng, len(pe), pairs)):
            E, out = be.photon_pion(d, pc, mc, aa, target, 1.0, n_photon, emin, bpd, i_data)
            check_pion(T2, d, pc, mc, aa, target, 1.0, i_data, E, out, (aa, i_data, c))
        pc, bins, hit = pion_exact_hits(mc, aa, len(pe))
        T.exact_hits = getattr(T, "exact_hits", set()) | set(hit)
        d = np.full((ng, len(pe)), 1.0e-99)
        for z, b in enumerate(bins):
            d[z, b] = 1.0e30 / (pc[b + 1] - pc[b])
        E, out = be.photon_pion(d, pc, mc, aa, target, 1.0, n_photon, emin, bpd, i_data)
        check_pion(T2, d, pc, mc, aa, target, 1.0, i_data, E, out, (aa, i_data, "hit"))
    return T


def pion_sum_structure(be, prob, seed=4):
    tabs = mcs.consumers.consumer_tables(prob, 1)
    pe, ng = tabs.mom_edge_cgs, prob.params.n_grid
    d = dense_spectrum(np.random.default_rng(seed), ng, len(pe), floors=(1.0e-99,))       # (K7 has no cut at 1e-60)
    d[:, :-1] = np.where(d[:, :-1] > 1.0e-60, d[:, :-1] / np.diff(pe)[None, :], d[:, :-1])
    target = pion_target(ng)
    return fold_sum_structure(lambda x: be.photon_pion(x, pe, MPROT * C, 1.0, target, 1.0, *PION_GRID, 1)[1], d, len(pe) - 1, exact_above=2.0e-83)


# -- K6
IC_AREA = 1.0e20
IC_AREA_TINY = 1.0e-30          # the flux floor of 1e-55 then lies below every cur > 1e-60 (E^2 / (area m_e c^2) > 1e5 on IC_GRID)
IC_FIELD_BINS = (0, 30, 59)


def ic_rows(j_max):
    return (0, j_max, j_max // 2, min(1, j_max))


class IcSide:
    """One back-end with the electrons problem's tables: crafted psd cells -> get_dNdp_2D in the frame of the tallies themselves
    (gam 1, beta 0: every cell goes to its own bin) -> the d2N/dp dcos the fold reads, downloaded."""
    def __init__(self, be, prob, pe=None):
        self.be, self.prob, self.P = be, prob, prob.params
        self.L = mcs.capi.Layout(self.P)
        self.t = mcs.consumers.consumer_tables(prob, 1)
        self.pe, self.mc = (self.t.mom_edge_cgs, self.t.mc) if pe is None else (pe, ME * C)     # what the FOLD is given
        self.ng, self.NM, self.NT = self.P.n_grid, self.P.num_psd_mom_bins + 2, self.P.num_psd_tht_bins + 2
        self.is_device = type(be).__name__ == "HipBackend"
        if self.is_device:
            be.begin_iteration(1)

    def load(self, cells, pops, download=True):
        """cells: (zone, angle row, momentum bin, weight); pops[zone]: the zone's population, which a zone's cells share in
        proportion to their weights -> d2N [n_grid][NT][NM] (download=False: it stays where the fold reads it, None comes back)"""
        f = np.zeros(self.L.total)
        i = np.zeros(self.L.n_i64, dtype=np.int64)
        psd = self.L.view(f, "psd")
        for z, j, k, w in cells:
            psd[z, j, k] = w
        i[:self.ng] = 1                                        # crossings seen: no upstream population is added to the zone's
        self.t.zone_pop = np.ascontiguousarray(pops, dtype=np.float64)
        if self.is_device:
            self.be.write_tallies(f, i)
            d2 = self.be.dndp_2d(self.t, 1.0, 0.0, download=download)
            if not download:
                return None
        else:
            d2 = self.be.dndp_2d(self.t, 1.0, 0.0, tallies=(f, i))
        want = np.zeros(d2.shape, dtype=bool)
        for z, j, k, w in cells:
            want[z, j, k] = True
        assert np.array_equal(d2 > 1.0e-99, want)              # every cell stayed in its own bin
        return d2

    def fold(self, pe, j_max, alpha_in, n_in, grid, area=IC_AREA):
        n_photon, emin, bpd = grid
        return self.be.photon_ic(pe, self.mc, j_max, alpha_in, n_in, n_photon, emin, bpd, area)


def ic_threshold_pairs(mc, E, a1):
    """Crafted (momentum, zone population) pairs of K6: p = 0.005 mc (the gamma = 1 branch); gamma = alpha_out at two energies of the
    grid; q = 1 (the Jones bracket changes sign) at two; populations around cur = 1e-60 are added by the caller."""
    pairs = [(p, 1.0e40) for p in ladder(E_REL_PT * mc)]
    mec2 = ME * C * C
    for j in (5, 6):
        ao = float(E[j]) / mec2
        pairs += [(p, 1.0e40) for p in ladder(mc * math.sqrt(ao * ao - 1))]
    for j in (4, 5):
        ao = float(E[j]) / mec2
        g = (ao + math.sqrt(ao * ao + ao / a1)) / 2
        pairs += [(p, 1.0e40) for p in ladder(mc * math.sqrt(g * g - 1))]
    return pairs


def ic_term_by_term(side, what, part):
    """K6 with ONE incoming photon bin per call: the impulse sweep over the momentum grid (angle rows 0, j_max and two between),
    the crafted thresholds, alpha_out around gamma = 1 of slow electrons (by the energy grid), populations around cur = 1e-60."""
    ng, NM, nt = side.ng, side.NM, side.NT - 2
    pe, mc = side.pe, side.mc
    alpha_cmb, n_cmb = mcs.consumers.photon_field_cmb(0.0)
    T2 = T = Tally(what + " " + part)
    j_max = nt
    if part == "impulses":
        for c, d in enumerate(impulse_spectra(ng, NM - 1, lambda b: 10.0 ** (30 + (7 * b) % 40))):
            cells = [(z, ic_rows(j_max)[lit_bin_of(d[z]) % 4], lit_bin_of(d[z]), 1.0) for z in range(ng) if lit_bin_of(d[z]) is not None]
            d2 = side.load(cells, d.max(axis=1))
            for fb in IC_FIELD_BINS:
                a, n = alpha_cmb[fb:fb + 1], n_cmb[fb:fb + 1]
                E, out = side.fold(pe, j_max, a, n, IC_GRID)
                check_ic(T, d2, pe, mc, j_max, a, n, IC_AREA, E, out, (c, fb))
        return T
    j_max = nt // 2
    a, n = alpha_cmb[30:31], n_cmb[30:31]
    side.load([(0, 0, 1, 1.0)], np.full(ng, 1.0))
    E = side.fold(pe, j_max, a, n, IC_GRID)[0]
    per_call = min(ng, (NM - 1) // 2)

    def crafted(pairs, area, tag):
        for c, r in enumerate(range(0, len(pairs), per_call)):
            chunk = pairs[r:r + per_call]
            pc, bins = edges_for([p for p, _ in chunk], NM)
            cells = [(z, ic_rows(j_max)[z % 4], b, 1.0) for z, b in enumerate(bins)]
            pops = np.full(ng, 1.0)
            pops[:len(chunk)] = [pop for _, pop in chunk]
            d2 = side.load(cells, pops)
            E, out = side.fold(pc, j_max, a, n, IC_GRID, area)
            check_ic(T2, d2, pc, mc, j_max, a, n, area, E, out, (tag, c))

    crafted(ic_threshold_pairs(mc, E, float(a[0])), IC_AREA, "thr")
    p_gen = 1.0e4 * mc
    pc0, _ = edges_for([p_gen], 4)
    unit = ic_bin(np.full(j_max + 1, 1.0e40), pc0[0], pc0[1], mc, 0, IC_AREA_TINY)
    pairs = []
    for j in (3, 4):                                             # cur = 1e-60 at energy j, from the term of a population of 1e40
        u = unit(float(E[j]), a, n)
        assert u.lit
        cur40 = u.r * IC_AREA_TINY * MPF(ME * C * C) / MPF(float(E[j])) ** 2
        pairs += [(p_gen, pop) for pop in ladder(float(1.0e-20 / cur40))]
    crafted(pairs, IC_AREA_TINY, "cur")
    # slow electrons (gamma = 1 exactly) under energy grids whose last energy is m_e c^2 (1 -+ offsets)
    pc, bins = edges_for([1.0e-3 * mc], NM)
    d2 = side.load([(z, 0, bins[0], 1.0) for z in (0, 50, ng - 1)], np.full(ng, 1.0e40))
    for e1 in ladder(ME * C * C / MEV):
        E, out = side.fold(pc, j_max, a, n, (10, e1 / 1.0e9, 1))
        check_ic(T2, d2, pc, mc, j_max, a, n, IC_AREA, E, out, ("alpha=1", e1))
    return T


def ic_shapes(side, what):
    """K6: j_max 0 and NT - 2, n_nu 1 and 60; per zone one momentum bin whose column holds several lit rows, one lit row, or none
    inside the cone (lit rows beyond j_max only: the bin is skipped); every output against the reference over the cone count (a
    numpy sum in row order) and the incoming bins in order."""
    ng, NM, nt = side.ng, side.NM, side.NT - 2
    pe, mc = side.pe, side.mc
    alpha_cmb, n_cmb = mcs.consumers.photon_field_cmb(0.0)
    assert len(alpha_cmb) == 60
    T = Tally(what + " shapes")
    k0 = int(np.searchsorted(pe, 1.0e3 * mc))
    cells = []
    for z in range(0, ng, 6):
        k = k0 + (z % 40)
        kind = (z // 6) % 4
        rows = {0: (0,), 1: (0, 1, nt // 2, nt), 2: (nt,), 3: (1, 2, 3)}[kind]
        cells += [(z, j, k, 10.0 ** (-3 * n)) for n, j in enumerate(rows)]
    d2 = side.load(cells, np.full(ng, 1.0e45))
    grid = (6, 1.0e-6, 0.5)
    for j_max in (0, nt):
        for a, n in ((alpha_cmb[30:31], n_cmb[30:31]), (alpha_cmb, n_cmb)):
            E, out = side.fold(pe, j_max, a, n, grid)
            # a zone whose lit rows all lie beyond j_max holds the floor row (check_ic sees no lit bin inside the cone)
            check_ic(T, d2, pe, mc, j_max, a, n, IC_AREA, E, out, (j_max, len(a)))
    return T


def ic_sum_structure(side, seed=6, pool=32):
    """K6, all 60 incoming bins: the dense output against the ordered sum of the same back-end's impulse outputs (one momentum
    column lit at a time).  Not bit for bit, unlike K5 and K7: the fold's sum passes through the flux conversion (a division by the
    beam area and by m_e c^2 and a product with E^2: three roundings, :285-308) before it is returned, and a column's share of the
    zone's population is rounded again when the other columns go dark; the beam area is so small that the flux floor of
    1e-55 lies below every term the fold keeps.  With n lit columns, the dense output is a sum of 60 n positive terms (60 n
    roundings) and 4 more of the conversion; the other side sums n outputs of 60 terms and a conversion each (at most 60 + 4
    roundings inside every one, n between them); a column's count differs between the two by the roundings of its share, its
    population and get_dNdp_2D's normalisation on either side (at most 12).  Sums of positive terms, so the relative errors add
    at worst: |dense - sum| <= (60 n + 4 + 64 + n + 12 + ...) 2^-53, asserted as (122 n + 32) 2^-53 of the value.  Few lit columns per zone (three to
    six out of a pool of `pool` columns, the first and the last momentum bin among them), so that every column carries weight
    somewhere and the number of impulse calls stays small."""
    ng, NM, nt = side.ng, side.NM, side.NT - 2
    pe = side.pe
    alpha_cmb, n_cmb = mcs.consumers.photon_field_cmb(0.0)
    rng = np.random.default_rng(seed)
    columns = np.unique(np.concatenate([[0, NM - 2], rng.integers(0, NM - 1, pool - 2)]))
    cols = {}
    for z in range(ng):
        if z % 5 == 4:
            continue
        ks = set(rng.choice(columns, rng.integers(3, 7)).tolist())
        cols[z] = {k: [(int(j), 10.0 ** rng.uniform(-2, 0)) for j in rng.integers(0, nt + 1, 3)] for k in ks}
    pops = np.full(ng, 1.0e45)
    dp = np.diff(side.t.mom_edge_cgs)                          # get_dNdp_2D shares a zone's population by weight / dp of ITS grid

    def run(only=None):
        cells, share = [], np.ones(ng)
        for z, ck in cols.items():
            tot = sum(w / dp[k] for k, rows in ck.items() for _, w in rows)
            for k, rows in ck.items():
                if only is None or k == only:
                    seen = {}
                    for j, w in rows:
                        seen[j] = seen.get(j, 0.0) + w
                    cells += [(z, j, k, w) for j, w in seen.items()]
                    if only is not None:
                        share[z] = sum(seen.values()) / dp[k] / tot
        if not cells:
            return None
        side.load(cells, pops * share, download=False)
        return side.fold(pe, nt, alpha_cmb, n_cmb, IC_GRID, IC_AREA_TINY)[1]

    dense = run()
    total = np.zeros_like(dense)
    n_terms = np.zeros(dense.shape, dtype=int)
    for k in columns:
        o = run(int(k))
        if o is None:
            continue
        lit = o > 1.0e-99
        total = total + np.where(lit, o, 0.0)
        n_terms += lit
    lit = dense > 1.0e-99
    assert lit.sum() > 100 and (n_terms > 2).sum() > 50
    assert np.array_equal(lit, n_terms > 0)
    err = np.abs(dense[lit] - total[lit]) / dense[lit]
    bound = (122 * n_terms[lit] + 32) * U
    print("K6 sum structure: worst |dense - sum of impulses| / bound =", float((err / bound).max()))
    assert np.all(err <= bound), float((err / bound).max())


# -- shapes and zones, K5 and K7
SHAPE_SIZES = (1, 255, 256, 257, 4096)
SHAPE_JS = (0, 1, 254, 255, 256, 257, 511, 512, 1023, 2048, 4094, 4095)


def synch_shapes(be, prob, what):
    """K5 with n_photon on either side of the workgroup's 256 threads and at the ABI's largest: every size gives the rows of the
    largest, and sampled rows of the largest (the second pass among them) are held against the reference."""
    tabs = mcs.consumers.consumer_tables(prob, 1)
    pe, mc, ng = tabs.mom_edge_cgs, tabs.mc, prob.params.n_grid
    d = impulse_spectra(ng, len(pe) - 1, lambda b: _count_weight(b) / (pe[b + 1] - pe[b]))[-1]
    emin, bpd = 1.0e-16, 150.0
    big = shapes_rows(lambda n: be.photon_synch(d, pe, mc, n, emin, bpd)[1], SHAPE_SIZES)
    E = be.photon_synch(d, pe, mc, max(SHAPE_SIZES), emin, bpd)[0]
    T = Tally(what + " shapes")
    check_synch(T, d, pe, prob.btot, mc, E, big, "4096", js=SHAPE_JS)
    return T


def pion_shapes(be, prob, what):
    tabs = mcs.consumers.consumer_tables(prob, 1)
    pe, ng = tabs.mom_edge_cgs, prob.params.n_grid
    target = pion_target(ng)
    d = impulse_spectra(ng, len(pe) - 1, lambda b: _count_weight(b) / (pe[b + 1] - pe[b]))[-1]
    emin, bpd, mc = 1.0, 400.0, MPROT * C
    big = shapes_rows(lambda n: be.photon_pion(d, pe, mc, 1.0, target, 1.0, n, emin, bpd, 1)[1], SHAPE_SIZES)
    E = be.photon_pion(d, pe, mc, 1.0, target, 1.0, max(SHAPE_SIZES), emin, bpd, 1)[0]
    T = Tally(what + " shapes")
    check_pion(T, d, pe, mc, 1.0, target, 1.0, 1, E, big, "4096", js=SHAPE_JS)
    return T


def ic_shapes_n_photon(side, what):
    ng, NM, nt = side.ng, side.NM, side.NT - 2
    pe, mc = side.pe, side.mc
    alpha_cmb, n_cmb = mcs.consumers.photon_field_cmb(0.0)
    a, n = alpha_cmb[59:60], n_cmb[59:60]
    d = impulse_spectra(ng, NM - 1, lambda b: 10.0 ** (30 + (7 * b) % 40))[-1]
    cells = [(z, ic_rows(nt)[z % 4], lit_bin_of(d[z]), 1.0) for z in range(ng) if lit_bin_of(d[z]) is not None]
    d2 = side.load(cells, d.max(axis=1))
    emin, bpd = 1.0e-9, 250.0
    big = shapes_rows(lambda m: side.fold(pe, nt, a, n, (m, emin, bpd))[1], SHAPE_SIZES)
    E = side.fold(pe, nt, a, n, (max(SHAPE_SIZES), emin, bpd))[0]
    T = Tally(what + " n_photon")
    check_ic(T, d2, pe, mc, nt, a, n, IC_AREA, E, big, "4096", js=SHAPE_JS)
    return T


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def synch_zones(be, prob):
    """K5 in the flat field: the same impulse in the first, a middle and the last zone gives the same bits; the zones between
    hold the floor."""
    tabs = mcs.consumers.consumer_tables(prob, 1)
    pe, mc, ng = tabs.mom_edge_cgs, tabs.mc, prob.params.n_grid
    for b in (0, 60, len(pe) - 2):
        d = np.full((ng, len(pe)), 1.0e-99)
        d[[0, 50, ng - 1], b] = 1.0e30 / (pe[b + 1] - pe[b])
        out = be.photon_synch(d, pe, mc, *SYNCH_GRID)[1]
        assert same_bits(out[0], out[50]) and same_bits(out[0], out[ng - 1])
        assert (out[0] > 1.0e-99).any() or b == 0
        assert np.all(np.delete(out, [0, 50, ng - 1], axis=0) == 1.0e-99)


def pion_zones(be, prob):
    """K7: zones of equal target density (the first, a middle and the last one) give the same bits for the same impulse, a zone
    of another density does not; an empty zone holds 1e-99 x scaling exactly."""
    tabs = mcs.consumers.consumer_tables(prob, 1)
    pe, ng = tabs.mom_edge_cgs, prob.params.n_grid
    target = pion_target(ng)
    for aa, scaling, b in ((1.0, 1.0, 70), (4.0, 2.37, 90), (56.0, 9.1, len(pe) - 2)):
        d = np.full((ng, len(pe)), 1.0e-99)
        d[[0, 7, 50, ng - 1], b] = 1.0e30 / (pe[b + 1] - pe[b])
        out = be.photon_pion(d, pe, aa * MPROT * C, aa, target, scaling, *PION_GRID, 1)[1]
        assert same_bits(out[0], out[50]) and same_bits(out[0], out[ng - 1]) and not same_bits(out[0], out[7])
        assert (out[0] > 1.0e-99 * scaling).sum() > 3
        assert np.all(np.delete(out, [0, 7, 50, ng - 1], axis=0) == 1.0e-99 * scaling)


# -- the exemption of test_photon_pion.py::test_gpu_pion_matches_cpu_twin
PION_TWIN_SETS = ((1.0, 1.0, 120, 1.0, 10, 1), (4.0, 2.37, 45, 10.0, 4, 1), (1.0, 1.3, 300, 0.5, 25, 2), (1.0, 1.0, 120, 1.0, 10, 3), (56.0, 9.1, 120, 1.0, 10, 4))


def pion_point_undecidable(d_row, pe, mc, aa, i_data, n_t, scaling, E_j):
    """Does the reference leave a decision open in ANY lit bin of this zone at this photon energy (X within its bound of the
    kinematic limit, or T_p within its bound of a branch point)?  -> list of the bins it leaves open"""
    return [int(i) for i in np.flatnonzero(d_row[:-1] > 1.0e-99)
            if pion_bin(float(d_row[i]), float(pe[i]), float(pe[i + 1]), mc, aa, i_data, float(n_t), scaling)(float(E_j)).undecidable]
