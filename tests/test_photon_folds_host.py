"""The three photon folds term by term on the CPU twin (oracle/mcs_consumers.cpp: orc_photon_synch, orc_photon_ic, orc_photon_pion)
against the mpmath reference of photon_fold_common.py, which shares no code with include/mcs_synch.h, mcs_ic.h and mcs_pion.h.

This file proves the reference, its running error bound and the builders before the same calls go to the device
(test_gpu_photon_folds.py): every impulse and threshold output of the twin lies within the bound computed for glibc's libm, the
masks agree at every decidable point, no point of these inputs is undecidable, and a dense spectrum is bit for bit the ordered sum
of the twin's own impulse terms."""
import math

import numpy as np
import pytest

import photon_fold_common as pf
from conftest import mcs, oracle_backend, orc


@pytest.fixture(autouse=True)
def _glibc():
    pf.use_libm(pf.GLIBC)


@pytest.fixture(scope="module")
def electrons():
    prob = pf.synch_problem()
    be = oracle_backend(prob)
    yield be, prob
    be.destroy()


@pytest.fixture(scope="module")
def protons():
    prob = pf.pion_problem()
    be = oracle_backend(prob)
    yield be, prob
    be.destroy()


def test_running_bound_holds_for_python_floats():
    """The bound machinery against the arithmetic it models: expressions of random doubles in Python floats (IEEE doubles, glibc's
    libm) stay within the bound carried by the same expression of V; a cancellation widens it as it must."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(300):
        a, b, c, d = (float(x) for x in 10.0 ** rng.uniform(-3, 3, 4))
        got = (math.sqrt(a * b + c) / d - a) * math.exp(-b / 50) + math.log(c) * (a ** 1.95) - float(np.cbrt(d)) * math.hypot(a / b, 1.0)
        A, B, Cc, Dd = (pf._v(x) for x in (a, b, c, d))
        ref = (pf.sqrt(A * B + Cc) / Dd - A) * pf.exp(-(B / 50)) + pf.log(Cc) * pf.power(A, 1.95) - pf.cbrt(Dd) * pf.hypot1(A / B)
        assert ref.e > 0
        worst = max(worst, abs(float(pf.MPF(got) - ref.r)) / ref.e)
    print("running bound, Python floats: worst |error| / bound =", worst)
    assert worst <= 1.0
    x = pf._v(1.0) / 3.0
    y = 1 - x * 3                                               # 0 in exact arithmetic, with an absolute bound of a few 2^-53
    assert abs(y.r) < 1e-40 and 1e-16 < y.e < 1e-15
    D = pf.Decisions()
    assert D.lt(pf._v(1.0), 2.0) and not D.undecidable          # exact operands decide exactly, equality included
    assert D.ge(pf._v(30.0), 30.0) and not D.undecidable
    assert D.ge(x * 3, 1.0) in (True, False) and D.undecidable  # 1/3 * 3 against 1: the interval straddles the cut


def test_exactness_the_sum_tests_rely_on():
    """acc starts at 1e-99; one term above 1e-55 (K5), above 1e-60 (K6) or above 2e-83 (K7: 1e-99 is then below 2^-54 of it, half an ulp wherever it lies in its binade) absorbs it: the impulse output IS the
    term.  np.cumsum adds in order."""
    for t in (1.0e-55, np.nextafter(1.0e-55, 1.0), 1.0e-60, 2.0e-83, 3.3e-70, 1.0):
        assert 1.0e-99 + t == t
    assert 1.0e-99 + 1.0e-84 != 1.0e-84
    x = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53])
    assert np.cumsum(x)[-1] == 1.0 and np.cumsum(x[::-1])[-1] > 1.0
    assert pf.ordered_sum([1.0, 2.0 ** -53]) == 1.0


def test_first_synchrotron_function_against_mpmath():
    """The two Chebyshev fits, evaluated exactly from the committed coefficients, against mpmath's own x int_x^inf K_5/3: the 1e-13
    of include/mcs_synch.h; the twin's F(x) within its running bound of the fit."""
    lib = orc.load("det", mcs.capi)
    assert abs(pf.synch_F_exact(0.7) / pf.synch_F_exact(0.7, bessel=True) - 1) < 1e-30
    xs = np.concatenate([10.0 ** np.linspace(-6, math.log10(29.99), 24), [pf.SYNCH_X0, np.nextafter(pf.SYNCH_X0, 5.0), 1.0e-15, 29.999999]])
    fit, libm = 0.0, 0.0
    for x in xs:
        D = pf.Decisions()
        f, _ = pf.synch_F(D, pf._v(float(x)))
        fit = max(fit, abs(float(f.r / pf.synch_F_exact(float(x)) - 1)))
        libm = max(libm, abs(float(pf.MPF(lib.orc_synch_F(float(x))) - f.r)) / f.e)
    print("F(x): worst fit error", fit, "; twin against the fit, worst |error| / bound", libm)
    assert fit < 1e-13 and libm <= 1.0




def test_synch_twin_term_by_term(electrons):
    be, prob = electrons
    pf.synch_term_by_term(be, prob, "K5 twin", "impulses").check(min_lit=800, branches=pf.K5_BRANCHES[:5])
    pf.synch_term_by_term(be, prob, "K5 twin", "thresholds").check(min_lit=200, branches=pf.K5_BRANCHES)


def test_synch_twin_field_cuts():
    prob = pf.synch_problem(flat=False)
    be = oracle_backend(prob)
    pf.synch_field_cuts(be, prob, "K5 twin").check(min_lit=50, branches=("skip:B<1e-20", "skip:w_c<1e-55", "F_small"))
    be.destroy()


def test_synch_twin_sum_structure_and_shapes(electrons):
    be, prob = electrons
    assert pf.synch_sum_structure(be, prob) == 0.0
    pf.synch_zones(be, prob)
    pf.synch_shapes(be, prob, "K5 twin").check(min_lit=100)




def test_pion_twin_term_by_term(protons):
    be, prob = protons
    pf.pion_term_by_term(be, prob, "K7 twin", "impulses").check(min_lit=2000)
    T = pf.pion_term_by_term(be, prob, "K7 twin", "thresholds")
    T.check(min_lit=1000, branches=pf.K7_BRANCHES)
    assert pf.PION_TP_HIT <= T.exact_hits, T.exact_hits           # bins whose T_p IS a branch point: < against <=


def test_pion_twin_sum_structure_and_shapes(protons):
    be, prob = protons
    assert pf.pion_sum_structure(be, prob) < 0.01
    pf.pion_zones(be, prob)
    pf.pion_shapes(be, prob, "K7 twin").check(min_lit=100)




def test_ic_twin_term_by_term(electrons):
    be, prob = electrons
    side = pf.IcSide(be, prob)
    pf.ic_term_by_term(side, "K6 twin", "impulses").check(min_lit=2000)
    pf.ic_term_by_term(side, "K6 twin", "thresholds").check(min_lit=100, branches=pf.K6_BRANCHES)


def test_ic_twin_shapes_and_sum_structure(electrons):
    be, prob = electrons
    side = pf.IcSide(be, prob)
    pf.ic_shapes(side, "K6 twin").check(min_lit=150)
    pf.ic_shapes_n_photon(side, "K6 twin").check(min_lit=100)
    pf.ic_sum_structure(side)
