"""The run options of a context on the device (enum mcs_option; HipBackend(options=, use_env=), set_option / get_option / options):
contexts that differ in their options alive together in one process, the precedence built-in default < environment < caller, changes
between launches, refusals that leave the context usable, and the driver's own arguments.  The kernels the options choose between
are pinned to each other and to the oracle by test_gpu_parity.py: a difference here is an error of the option plumbing.  A few
hundred to a few thousand particles, at most nine pcuts."""
import os

import numpy as np
import pytest

from conftest import mcs, make_problem, oracle_backend, start_species, bits, assert_pop_equal, assert_tallies_close

pytestmark = pytest.mark.gpu
TALLY_RTOL = 1e-11      # of the array's maximum: the order of the atomic adds (test_gpu_parity.py)


@pytest.fixture(autouse=True)
def _no_mcs_environment(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MCS_")]:
        monkeypatch.delenv(k)


def _hip(prob, options=None, use_env=True):
    from mcs_amd import hip_backend as hb
    be = hb.HipBackend(0, debug_finals=True, options=options, use_env=use_env)
    be.create(prob)
    return be


def _assert_same_pcut(a, b, what):
    """finals, saved arrays and l_save of the last pcut of two contexts, bit for bit"""
    fa, fb = a.finals(), b.finals()
    for k in fa:
        assert np.array_equal(bits(fa[k]), bits(fb[k])), f"{what}: final {k} differs for {(fa[k] != fb[k]).sum()} particles"
    (sa, la), (sb, lb) = a.get_saved(), b.get_saved()
    assert np.array_equal(la, lb), f"{what}: l_save"
    assert_pop_equal(sa, sb, f"{what}: saved arrays")


def _assert_same_tallies(a, b):
    (Ta, Ia), (Tb, Ib) = a.read_tallies(), b.read_tallies()
    assert np.array_equal(Ia, Ib)
    assert_tallies_close(a.layout, Ta, Tb, TALLY_RTOL)


_ORACLE_I64 = {}


def _oracle_first_pcut_i64(N, fp32_exact=False):
    """The oracle's integer tallies after pcut 1 of N protons (computed once per size and state precision)."""
    if (N, fp32_exact) not in _ORACLE_I64:
        prob = make_problem(N)
        prob.params.state_fp32 = int(fp32_exact)
        ob = oracle_backend(prob, nthreads=1 if fp32_exact else 8)
        ob.f32_exact = fp32_exact
        start_species(ob, prob)
        ob.run_pcut(1, 0)
        _ORACLE_I64[(N, fp32_exact)] = ob.read_tallies()[1].copy()
        ob.destroy()
    return _ORACLE_I64[(N, fp32_exact)]


def _first_pcut_i64(be, prob):
    start_species(be, prob)
    be.run_pcut(1, 0)
    return be.read_tallies()[1]


@pytest.mark.parametrize("N", [300, 4000])
def test_two_live_contexts_run_different_kernels(N):
    """test_wave_specialised_kernel_is_bit_identical without the environment and with both contexts alive: A runs the wave-specialised
    kernel (7), B the lane-owns-particle one (1), pcut by pcut in turn.  Less than one block (300), a few sparse blocks (4000)."""
    prob = make_problem(N)
    a, b = _hip(prob, {"k1_ws": 1}, use_env=False), _hip(prob, {"k1_ws": 0}, use_env=False)
    assert a.get_option("k1_ws") == 1 and b.get_option("k1_ws") == 0
    start_species(a, prob); start_species(b, prob)
    for ip in range(1, 10):
        n = a.pop_size()
        assert b.pop_size() == n
        nsa = a.run_pcut(ip, 0)
        nsb = b.run_pcut(ip, 0)
        assert (a.last_kernel(), b.last_kernel()) == (7, 1), ip
        assert nsa == nsb
        _assert_same_pcut(a, b, f"pcut {ip}")
        if nsa == 0:
            break
        im = max(n // nsa, 1)
        assert a.new_pcut(im) == b.new_pcut(im)
    _assert_same_tallies(a, b)
    a.destroy(); b.destroy()


def test_precedence_default_environment_caller(monkeypatch):
    monkeypatch.setenv("MCS_FORCE_GENERAL", "1")
    prob = make_problem(300)
    want = _oracle_first_pcut_i64(300)
    for kw, reported, kernel in ((dict(), 1, 0), (dict(options={"force_general": 0}), 0, 1), (dict(use_env=False), 0, 1)):
        be = _hip(prob, **kw)
        assert be.get_option("force_general") == reported and be.options()["force_general"] == reported, kw
        got = _first_pcut_i64(be, prob)
        assert be.last_kernel() == kernel, kw
        assert np.array_equal(got, want), kw
        be.destroy()


def test_option_changed_between_launches():
    """force_general on for pcut 1, off for pcut 2, on one context: kernel 0, then kernel 1, and what an untouched context computes."""
    N = 4000
    prob = make_problem(N)
    x, y = _hip(prob, use_env=False), _hip(prob, use_env=False)
    start_species(x, prob); start_species(y, prob)
    x.set_option("force_general", 1)
    assert x.get_option("force_general") == 1 and y.get_option("force_general") == 0
    ns = x.run_pcut(1, 0)
    assert y.run_pcut(1, 0) == ns and ns > 0
    assert (x.last_kernel(), y.last_kernel()) == (0, 1)
    _assert_same_pcut(x, y, "pcut 1")
    x.set_option("force_general", 0)
    im = max(N // ns, 1)
    assert x.new_pcut(im) == y.new_pcut(im)
    assert_pop_equal(x.get_population(), y.get_population(), "population of pcut 2")
    assert x.run_pcut(2, 0) == y.run_pcut(2, 0)
    assert (x.last_kernel(), y.last_kernel()) == (1, 1)
    _assert_same_pcut(x, y, "pcut 2")
    assert np.array_equal(x.read_tallies()[1], y.read_tallies()[1])
    x.destroy(); y.destroy()


def test_get_option_reports_the_environment_default(monkeypatch):
    prob = make_problem(300)
    monkeypatch.setenv("MCS_DEFER_K", "1")
    monkeypatch.setenv("MCS_REFILL_MIN", "20")
    monkeypatch.setenv("MCS_TALLY_REPLICAS_OFF", "1")
    be = _hip(prob)
    assert (be.get_option("defer_k"), be.get_option("refill_min"), be.get_option("tally_replicas")) == (1, 20, 0)
    table = mcs.capi.option_table()
    assert be.options() == {**{name: d["default"] for name, d in table.items()}, "defer_k": 1, "refill_min": 20, "tally_replicas": 0}
    be.destroy()
    monkeypatch.setenv("MCS_DEFER_K", "99")      # outside 1..40: the default stays, silently
    be = _hip(prob)
    assert be.get_option("defer_k") == 8
    with pytest.raises(RuntimeError, match=r"defer_k.*1\.\.40"):
        be.set_option("defer_k", 99)
    assert be.get_option("defer_k") == 8
    be.set_option("defer_k", 40)
    assert be.get_option("defer_k") == 40
    be.destroy()
    be = _hip(prob, use_env=False)
    assert be.options() == {name: d["default"] for name, d in table.items()}
    be.destroy()


def test_refusals_leave_the_context_usable():
    N = 300
    prob = make_problem(N)
    be = _hip(prob, use_env=False)
    before = be.options()
    with pytest.raises(RuntimeError, match="tally_replicas.*creation"):
        be.set_option("tally_replicas", 0)
    with pytest.raises(RuntimeError, match="f32_exact.*fp32"):
        be.set_option("f32_exact", 1)
    with pytest.raises(RuntimeError, match="unknown option key 99"):
        be._chk(be.lib.mcs_set_option(be.h, 99, 0))
    assert be.options() == before
    assert np.array_equal(_first_pcut_i64(be, prob), _oracle_first_pcut_i64(N))
    assert be.last_kernel() == 1
    be.destroy()
    # a fp32-state context (its exact loop: the kernel the oracle restates bit for bit)
    p32 = make_problem(N)
    p32.params.state_fp32 = 1
    be = _hip(p32, {"f32_exact": 1}, use_env=False)
    before = be.options()
    with pytest.raises(RuntimeError, match="tail_budget.*fp64"):
        be.set_option("tail_budget", 4)
    with pytest.raises(RuntimeError, match="not sliced"):      # (mcs_set_tail_slicing keeps its own words)
        be.set_tail_slicing(4)
    be.set_option("tail_budget", 0)
    assert be.options() == before
    assert np.array_equal(_first_pcut_i64(be, p32), _oracle_first_pcut_i64(N, fp32_exact=True))
    assert be.last_kernel() == 9
    be.destroy()


def test_ab_switches_through_options():
    """The option form of test_parking_and_tail_consolidation_do_not_change_results: waiting, consolidation, the tail ring, deferral and
    the tally replicas all off on one context, all on (the defaults) on another; few blocks, so that every lane is refilled often."""
    N = 4000
    prob = make_problem(N)
    off = {"park": 0, "tail_merge": 0, "tail_ring": 0, "defer_k": 1, "tally_replicas": 0}
    a, b = _hip(prob, off, use_env=False), _hip(prob, use_env=False)
    assert {k: a.get_option(k) for k in off} == off
    for be in (a, b):
        be.set_launch(4, 256)
        start_species(be, prob)
    for ip in range(1, 7):
        ns = a.run_pcut(ip, 0)
        assert b.run_pcut(ip, 0) == ns and ns > 0
        _assert_same_pcut(a, b, f"pcut {ip}")
        im = max(N // ns, 1)
        assert a.new_pcut(im) == b.new_pcut(im)
    assert_pop_equal(a.get_population(), b.get_population(), "population after pcut 6")
    _assert_same_tallies(a, b)
    a.destroy(); b.destroy()


def test_fp32_exact_kernel_by_option():
    N = 300
    prob = make_problem(N)
    prob.params.state_fp32 = 1
    be = _hip(prob, {"f32_exact": 1}, use_env=False)
    assert be.get_option("f32_exact") == 1 and be.get_option("f32_loop") == 0
    got = _first_pcut_i64(be, prob)
    assert be.last_kernel() == 9
    assert np.array_equal(got, _oracle_first_pcut_i64(N, fp32_exact=True))
    be.set_option("f32_exact", 0)
    be.set_option("f32_loop", 1)
    start_species(be, prob)
    be.run_pcut(1, 0)
    assert be.last_kernel() == 4
    be.destroy()


def test_driver_fused_chunk_argument_and_recorded_options():
    N = 2000
    res = []
    for kw in (dict(), dict(fused_chunk=3)):
        prob = make_problem(N)
        be = _hip(prob, {"tail_loop": 10}, use_env=False)
        r = mcs.driver.run(prob, be, n_itrs=1, max_pcuts=8, **kw)
        assert r.options == {**be.options(), "fused_pcuts": True, "fused_chunk": kw.get("fused_chunk", 12), "long_draws": 0,
                             "long_imult_max": 8}
        assert r.options["tail_loop"] == 10 and r.options["k1_ws"] == 2
        res.append(r)
        be.destroy()
    a, b = res
    row = lambda s: (s.i_iter, s.i_ion, s.i_pcut, s.n_pts_use, s.n_saved, s.i_mult)
    assert len(a.stats) == 8 and [row(s) for s in a.stats] == [row(s) for s in b.stats]
    assert np.array_equal(a.tallies_i64, b.tallies_i64)
