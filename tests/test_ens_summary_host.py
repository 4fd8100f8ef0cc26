"""The summary of word ranges and the stop rule without a GPU: ensemble.HostEnsemble.summarize against the restatement of
ens_summary_common.py on the crafted buffers, ensemble.Trigger, the exported symbol, and driver.run(triggers=...) through the CPU
oracle (one thread: its runs repeat bit for bit)."""
import ctypes as ct
import math

import numpy as np
import pytest

from conftest import mcs, make_problem, oracle_backend
from ensemble_common import AS_IS, INCREMENTS, bits_equal, crafted_buffers
from ens_summary_common import (as_dict, assert_exact, assert_sums, iteration_offsets, restate, same_bits, slot_vectors, species_offsets,
                                value_of)
ens = mcs.ensemble


class _Buffers:
    """The least a backend is to the host accumulator: the parameters and a tally buffer to read and write."""

    def __init__(self, prob):
        self.P = prob.params
        self.layout = mcs.capi.Layout(self.P)
        self.f, self.i = np.zeros(self.layout.total), np.zeros(self.layout.n_i64, dtype=np.int64)

    def read_tallies(self):
        return self.f.copy(), self.i.copy()

    def write_tallies(self, f, i):
        self.f, self.i = np.array(f, dtype=np.float64), np.array(i, dtype=np.int64)


@pytest.fixture(scope="module")
def fed():
    """A host accumulator fed the five crafted buffers as species samples (slot 0) and as iteration samples (slot 1)."""
    prob = make_problem(64)
    L = mcs.capi.Layout(prob.params)
    be = _Buffers(prob)
    e = ens.HostEnsemble(prob.params, 1)
    prev = np.zeros(L.total)
    for f, i in crafted_buffers(L):
        be.write_tallies(prev, i)
        e.begin_iteration(be)
        be.write_tallies(f, i)
        e.add_species(be, 0)
        e.add_iteration(be)
        prev = f
    return prob, L, e


def test_host_summary_equals_the_restatement(fed):
    prob, L, e = fed
    sp_off, sp_total = species_offsets(L)
    it_off, it_total = iteration_offsets(L, INCREMENTS + AS_IS)
    assert sp_total == e.layout.species_total and it_total == e.layout.iteration_total
    ng = prob.params.n_grid
    for slot, table in ((0, sp_off), (1, it_off)):
        mean, m2 = slot_vectors(e, slot)
        # (floor_frac = 0 selects nearly every word: on the parts below 10^5 words, where the exact sums are quick)
        reqs = [ens.Request(name, None, ff, 0.05) for name in table for ff in (0.0, 1e-3, 1.0) if ff > 0 or np.prod(table[name][1]) < 1e5]
        reqs += [ens.Request(name, (3, ng - 5), 1e-3, 0.2) for name in table if name in ens.ZONE_PARTS]
        got = e.summarize(slot, reqs)
        assert len(got) == len(reqs)
        for q, s in zip(reqs, got):
            first, shape = table[q.name]
            count = int(np.prod(shape))
            if q.zones is not None:
                per = count // shape[0]
                first, count = first + q.zones[0] * per, (q.zones[1] - q.zones[0]) * per
            assert e.word_range(slot, q.name, q.zones) == (first, count)
            want = restate(mean[first:first + count], m2[first:first + count], 5, q.floor_frac, q.tol)
            assert s.n == 5 and want["n_selected"] >= 1
            assert_exact(as_dict(s), want, f"slot {slot} {q}")
            assert_sums(as_dict(s), want, f"slot {slot} {q}")
    # an empty zone slice, and non-finite words
    s = e.summarize(0, [ens.Request("pxx_flux", (7, 7))])[0]
    assert as_dict(s) == restate([], [], 5, 1e-3, 0.0) and s.argmax == -1 and s.amax == 0.0
    with pytest.raises(ValueError, match="two samples"):
        ens.HostEnsemble(prob.params, 1).summarize(0, [ens.Request("psd")])
    with pytest.raises(KeyError):
        e.summarize(1, [ens.Request("psd")])
    with pytest.raises(ValueError, match="zones"):
        e.summarize(0, [ens.Request("pxx_flux", (0, ng + 1))])
    with pytest.raises(ValueError, match="at most"):
        e.summarize(0, [ens.Request("pxx_flux")] * 257)


def test_summary_of_handles_non_finite_words_and_ties():
    mean = np.array([1.0, -4.0, np.nan, 2.0, 4.0, np.inf, 8.0, 0.0, 1e-9])
    m2 = np.array([0.5, 8.0, 1.0, np.nan, 8.0, 1.0, np.inf, 3.0, 1e-18])
    for ff, tol in ((0.0, 0.1), (1e-3, 0.3), (1.0, 0.0)):
        got, want = as_dict(ens.summary_of(mean, m2, 4, ff, tol)), restate(mean, m2, 4, ff, tol)
        assert_exact(got, want)
        assert_sums(got, want)
        assert got["n_nonfinite"] == 4 and got["amax"] == 4.0       # (the 8.0 has an infinite M2: it is no finite word)
    s = ens.summary_of(mean, m2, 4, 1.0, 0.0)
    assert s.n_selected == 2 and s.argmax == 1                      # words 1 and 4 tie; the lower one is reported
    assert ens.summary_of(mean, m2, 4, 0.0, 0.0).n_selected == 4    # (the zero mean is never selected)


def test_trigger_values_and_refusals():
    T = ens.Trigger
    s = ens.Summary(amax=10.0, max_rel=0.2, sum_se=3.0, sum_abs_mean=60.0, sum_rel2=0.09, n_selected=9, n_over=3, n_nonfinite=0, argmax=4, n=5)
    cases = (("max", 0.2), ("rms", math.sqrt(0.09 / 9)), ("weighted", 3.0 / 60.0), ("fraction_over", 3 / 9))
    for stat, want in cases:
        t = T(0, "psd_mom", stat, want, tol=0.1)
        assert same_bits(t.value(s), want) and t.met(s)
        tight = T(0, "psd_mom", stat, want / 2, tol=0.1)
        assert not tight.met(s)
        assert tight.predicted_samples(s) == (None if stat == "fraction_over" else 20)       # 5 * 2^2
        assert t.request == ens.Request("psd_mom", None, 1e-3, 0.1)
    t = T(0, "psd_mom", "max", 0.5)
    assert t.predicted_samples(s) == math.ceil(5 * (0.2 / 0.5) ** 2) == 1
    import dataclasses
    for kw in (dict(n=1), dict(n_selected=0), dict(n_nonfinite=1)):
        assert not t.met(dataclasses.replace(s, **kw)), kw
    assert math.isnan(t.value(dataclasses.replace(s, n_selected=0))) and t.predicted_samples(dataclasses.replace(s, n_selected=0)) is None
    assert T(0, "psd", "max", 0.1, zones=(2, 5)).request.zones == (2, 5)
    for args, kw in ((("psd", "median", 0.1), {}), (("psd", "max", 0.0), {}), (("psd", "max", -1.0), {}), (("psd", "fraction_over", 0.1), {}),
                     (("esc_psd_up", "max", 0.1), dict(zones=(0, 2))), (("scalars", "max", 0.1), dict(zones=(0, 2))),
                     (("px_esc_feb", "max", 0.1), {}), (("no_such_part", "max", 0.1), {}), (("psd", "max", 0.1), dict(floor_frac=1.5)),
                     (("psd", "max", 0.1), dict(tol=-1.0))):
        with pytest.raises(ValueError):
            T(0, *args, **kw)
    with pytest.raises(ValueError):
        T(-1, "psd", "max", 0.1)
    # which slot is the iteration slot only an ensemble knows
    e = ens.HostEnsemble(make_problem(64).params, 1)
    e.check_trigger(T(0, "psd", "max", 0.1)); e.check_trigger(T(1, "spectra_sf", "max", 0.1, zones=(0, 3)))
    for bad in (T(1, "psd", "max", 0.1), T(0, "spectra_sf", "max", 0.1), T(0, "pxx_flux", "max", 0.1, zones=(0, 1000))):
        with pytest.raises((KeyError, ValueError)):
            e.check_trigger(bad)
    with pytest.raises(ValueError):
        e.check_trigger(T(2, "psd", "max", 0.1))


def test_symbol_is_exported_and_refuses_without_an_accumulator():
    lib = mcs.capi.load_library()
    assert hasattr(lib, "mcs_ens_summarize") and "mcs_ens_summarize" in mcs.capi.EXPORTED_SYMBOLS
    assert ct.sizeof(mcs.capi.McsEnsRange) == 32 and ct.sizeof(mcs.capi.McsEnsSummary) == 72
    r, out = mcs.capi.McsEnsRange(0, 1, 0.0, 0.0), mcs.capi.McsEnsSummary()
    assert lib.mcs_ens_summarize(None, 0, 1, ct.byref(r), ct.byref(out)) != 0
    assert b"mcs_ens_summarize" in lib.mcs_last_error() and b"null argument" in lib.mcs_last_error()


N_ITRS = 6


@pytest.fixture(scope="module")
def oracle_runs():
    """A plain run of N_ITRS iterations on the oracle, the "max" value of pxx_flux recorded at every iteration end."""
    prob = make_problem(300, num_iterations=N_ITRS)
    be = oracle_backend(prob)
    e = ens.Ensemble.for_backend(be, 1)
    seq = {}

    def record(it):
        if e.count(0) >= 2:
            r = restate(e.mean(0, "pxx_flux"), e.m2(0, "pxx_flux"), e.count(0), 1e-3, 0.0)
            seq[it] = (r, value_of("max", r, e.count(0)))
    plain = mcs.driver.run(prob, be, n_itrs=N_ITRS, max_pcuts=4, ensemble=e, on_iteration_end=record)
    assert plain.convergence is None
    yield prob, seq
    be.destroy()


def _run(prob, **kw):
    be = oracle_backend(prob)
    e = ens.Ensemble.for_backend(be, 1)
    res = mcs.driver.run(prob, be, max_pcuts=4, ensemble=e, **kw)
    be.destroy()
    return res, e


def test_driver_stops_where_the_trigger_is_met(oracle_runs):
    prob, seq = oracle_runs
    assert sorted(seq) == list(range(2, N_ITRS + 1))
    threshold = seq[4][1]
    expected = next(it for it in range(2, N_ITRS + 1) if seq[it][1] <= threshold)
    print("max relative error of pxx_flux by iteration:", {it: v for it, (r, v) in seq.items()}, "expected stop:", expected)
    assert 2 < expected < N_ITRS
    trig = ens.Trigger(0, "pxx_flux", "max", threshold)
    res, e = _run(prob, n_itrs=N_ITRS, triggers=[trig])
    c = res.convergence
    assert c.stopped_at == expected and c.satisfied and [it for it, _ in c.checks] == list(range(2, expected + 1))
    for it, rows in c.checks:
        (row,) = rows
        assert row.trigger is trig and row.summary.n == it
        assert_exact(as_dict(row.summary), seq[it][0], f"iteration {it}")
        assert_sums(as_dict(row.summary), seq[it][0], f"iteration {it}")
        assert same_bits(row.value, seq[it][1]) and row.met == (it == expected)
        assert row.predicted_samples == math.ceil(it * (seq[it][1] / threshold) ** 2)
    # the prefix property: exactly what a run of `expected` iterations does
    short, es = _run(prob, n_itrs=expected)
    assert len(res.per_species) == len(short.per_species) == expected and e.count(0) == es.count(0) == expected
    for (ia, sa, fa, ja), (ib, sb, fb, jb) in zip(res.per_species, short.per_species):
        assert (ia, sa) == (ib, sb) and bits_equal(fa, fb) and np.array_equal(ja, jb)
    assert bits_equal(res.tallies_f64, short.tallies_f64) and np.array_equal(res.tallies_i64, short.tallies_i64)
    for slot in (0, 1):
        for a, b in zip(slot_vectors(e, slot), slot_vectors(es, slot)):
            assert bits_equal(a, b), slot
    # min_iterations and check_every: the checks fall on iterations 3, 5, and the run stops at the first of them that meets it
    res2, _ = _run(prob, n_itrs=N_ITRS, triggers=[trig], min_iterations=3, check_every=2)
    stop = next((it for it in (3, 5) if seq[it][1] <= threshold), N_ITRS)
    assert [it for it, _ in res2.convergence.checks] == [it for it in (3, 5) if it <= stop] and res2.convergence.stopped_at == stop


def test_driver_runs_to_the_cap_when_a_trigger_is_out_of_reach(oracle_runs):
    prob, seq = oracle_runs
    met, never = ens.Trigger(0, "pxx_flux", "max", 1e9), ens.Trigger(0, "pxx_flux", "rms", 1e-12, zones=(0, prob.params.n_grid))
    other_slot = ens.Trigger(1, "spectra_sf", "fraction_over", 1.0, tol=0.5)
    res, e = _run(prob, n_itrs=4, triggers=[met, never, other_slot])
    c = res.convergence
    assert c.stopped_at == 4 and not c.satisfied and [it for it, _ in c.checks] == [2, 3, 4] and e.count(0) == 4
    for it, rows in c.checks:
        assert [row.trigger for row in rows] == [met, never, other_slot]
        assert rows[0].met and not rows[1].met and rows[1].predicted_samples > 4
        assert rows[2].predicted_samples is None and rows[2].summary.n == it


def test_driver_refusals(oracle_runs):
    prob, seq = oracle_runs
    be = oracle_backend(prob)
    e = ens.Ensemble.for_backend(be, 1)
    t = ens.Trigger(0, "pxx_flux", "max", 0.1)
    with pytest.raises(ValueError, match="triggers"):
        mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, triggers=[t])
    for kw in (dict(min_iterations=1), dict(check_every=0)):
        with pytest.raises(ValueError, match="triggers"):
            mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, ensemble=e, triggers=[t], **kw)
    with pytest.raises(KeyError):
        mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, ensemble=e, triggers=[ens.Trigger(1, "pxx_flux", "max", 0.1)])
    with pytest.raises(ValueError, match="ensemble"):
        mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, ensemble=e, triggers=[t], tcut_print=True)
    assert e.count(0) == 0 and e.count(1) == 0
    assert mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, ensemble=e, triggers=[]).convergence is None
    be.destroy()
