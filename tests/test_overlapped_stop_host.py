"""The stop rule of an overlapped run without a GPU: the exported mcs_ens_summarize_merged and its refusals that need no device,
ensemble.HostEnsemble.summarize_merged against a numpy fold written here and the restatement of ens_summary_common.py, and
driver.run_overlapped(triggers=...) through the CPU oracle (one thread per context: its runs repeat bit for bit)."""
import ctypes as ct

import numpy as np
import pytest

from conftest import mcs, make_problem, oracle_backend
from ensemble_common import bits_equal, crafted_buffers
from ens_summary_common import as_dict, assert_exact, assert_sums, restate, same_bits, slot_vectors

ens = mcs.ensemble
SPLITS = ((2, 2, 2), (3, 2), (1, 1), (0, 3, 0, 2))
OVERFLOW_WORD = 11          # of psd: 1e160 and -1e160 in turn by accumulator that is fed, so that d * d of a merge is not finite


def test_symbol_is_exported_and_refuses_without_an_accumulator():
    lib = mcs.capi.load_library()
    assert hasattr(lib, "mcs_ens_summarize_merged") and "mcs_ens_summarize_merged" in mcs.capi.EXPORTED_SYMBOLS
    assert ens.MAX_MERGED == 8
    r, out, n = mcs.capi.McsEnsRange(0, 1, 0.0, 0.0), mcs.capi.McsEnsSummary(), ct.c_int64(-7)
    nine = (ct.c_void_p * 9)()
    one = (ct.c_void_p * 1)()
    for what, call in (("a null list", lambda: lib.mcs_ens_summarize_merged(1, None, 0, 1, ct.byref(r), ct.byref(out), ct.byref(n))),
                       ("n_ens = 0", lambda: lib.mcs_ens_summarize_merged(0, nine, 0, 1, ct.byref(r), ct.byref(out), ct.byref(n))),
                       ("n_ens = 9", lambda: lib.mcs_ens_summarize_merged(9, nine, 0, 1, ct.byref(r), ct.byref(out), ct.byref(n))),
                       ("a null entry", lambda: lib.mcs_ens_summarize_merged(1, one, 0, 1, ct.byref(r), ct.byref(out), ct.byref(n)))):
        assert call() != 0, what
        assert b"mcs_ens_summarize_merged" in lib.mcs_last_error(), (what, lib.mcs_last_error())
        assert n.value == -7, what


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


def _fold(parts, slot):
    """The definition of the header, written out: (mean, M2, n) of the left fold over the accumulators that have samples."""
    m = q = None
    na = 0
    for e in parts:
        nb = e.count(slot)
        if nb == 0:
            continue
        mb, qb = slot_vectors(e, slot)
        if na == 0:
            m, q = mb, qb
        else:
            n = float(na + nb)
            f_mean, f_m2 = float(nb) / n, float(na) * float(nb) / n
            with np.errstate(over="ignore", invalid="ignore"):
                d = mb - m
                m = m + d * f_mean
                q = (q + qb) + (d * d) * f_m2
        na += nb
    return m, q, na


@pytest.fixture(scope="module")
def small():
    """A small layout (two bins per decade, 9 + 2 angle bins) and six crafted buffers on it."""
    prob = make_problem(64, num_psd_bins_per_decade=(2, 2), psd_linear_cosine_bins=9, psd_log_theta_decs=1)
    L = mcs.capi.Layout(prob.params)
    return prob, L, crafted_buffers(L, 6)


@pytest.mark.parametrize("counts", SPLITS, ids=lambda c: "-".join(map(str, c)))
def test_host_merged_summary(small, counts):
    prob, L, bufs = small
    be = _Buffers(prob)
    parts = [ens.HostEnsemble(prob.params, 1) for _ in counts]
    k = 0
    prev = np.zeros(L.total)
    fed = [a for a, c in enumerate(counts) if c]
    for a, (e, c) in enumerate(zip(parts, counts)):
        for _ in range(c):
            f, i = bufs[k][0].copy(), bufs[k][1]
            f[L.offsets["psd"] + OVERFLOW_WORD] = 1e160 if fed.index(a) % 2 == 0 else -1e160
            be.write_tallies(prev, i)
            e.begin_iteration(be)
            be.write_tallies(f, i)
            e.add_species(be, 0)
            e.add_iteration(be)
            prev, k = f, k + 1
    before = [[slot_vectors(e, s) for s in (0, 1)] for e in parts]
    ng, n_total = prob.params.n_grid, sum(counts)
    into = ens.HostEnsemble(prob.params, 1)
    with np.errstate(over="ignore", invalid="ignore"):          # (the overflow word)
        for e in parts:
            into.merge(e)
    for slot in (0, 1):
        names = parts[0].names(slot)
        reqs = [ens.Request(name, None, ff, 0.05) for name in names for ff in (0.0, 1e-3, 1.0)]
        reqs += [ens.Request(name, (3, ng - 5), 1e-3, 0.2) for name in names if name in ens.ZONE_PARTS]
        reqs += [ens.Request("pxx_flux" if slot == 0 else "spectra_sf", (7, 7))]
        got = parts[0].summarize_merged(parts[1:], slot, reqs)
        mean, m2, n = _fold(parts, slot)
        assert n == n_total and len(got) == len(reqs)
        via_merge = into.summarize(slot, reqs)
        selected = 0
        for q, s, t in zip(reqs, got, via_merge):
            first, count = parts[0].word_range(slot, q.name, q.zones)
            want = restate(mean[first:first + count], m2[first:first + count], n, q.floor_frac, q.tol)
            assert s.n == n_total
            assert_exact(as_dict(s), want, f"{counts} slot {slot} {q}")
            assert_sums(as_dict(s), want, f"{counts} slot {slot} {q}")
            for key, x in as_dict(s).items():
                y = getattr(t, key)
                assert same_bits(x, y) if isinstance(x, float) else x == y, (counts, slot, q, key)
            assert t.n == s.n
            selected += want["n_selected"]
        assert selected > 0
        if slot == 0:
            # the word that is finite in every part and not in the merge
            w = OVERFLOW_WORD
            for e in parts:
                if e.count(0):
                    assert np.isfinite(e.mean(0, "psd").ravel()[w]) and np.isfinite(e.m2(0, "psd").ravel()[w])
            assert np.isfinite(mean[w]) and np.isinf(m2[w])
            s = got[[q.name for q in reqs].index("psd")]
            assert s.n_nonfinite == 1
            assert parts[0].summarize_merged(parts[1:], 0, [ens.Request("psd", (1, ng))])[0].n_nonfinite == 0
    # nothing was changed, and an empty list is summarize
    for e, b in zip(parts, before):
        for slot in (0, 1):
            for x, y in zip(slot_vectors(e, slot), b[slot]):
                assert bits_equal(x, y)
    assert [e.count(0) for e in parts] == list(counts)
    assert into.summarize_merged([], 0, reqs[:0] + [ens.Request("pxx_flux")]) == into.summarize(0, [ens.Request("pxx_flux")])


def test_host_merged_summary_refusals(small):
    prob, L, bufs = small
    be = _Buffers(prob)
    a, b, wide = ens.HostEnsemble(prob.params, 1), ens.HostEnsemble(prob.params, 1), ens.HostEnsemble(prob.params, 2)
    other = ens.HostEnsemble(make_problem(64).params, 1)
    be.write_tallies(*bufs[0])
    a.add_species(be, 0)
    req = [ens.Request("pxx_flux")]
    with pytest.raises(ValueError, match="two samples"):
        a.summarize_merged([b], 0, req)
    be.write_tallies(*bufs[1])
    b.add_species(be, 0)
    assert a.summarize_merged([b], 0, req)[0].n == 2
    for others in ([a], [b, b], [wide], [other], [object()], [ens.HostEnsemble(prob.params, 1) for _ in range(8)]):
        with pytest.raises(ValueError, match="merged summary"):
            a.summarize_merged(others, 0, req)
    with pytest.raises(KeyError):
        a.summarize_merged([b], 1, req)
    with pytest.raises(ValueError, match="slot"):
        a.summarize_merged([b], 2, req)
    assert a.count(0) == 1 and b.count(0) == 1


N_ITRS = 6


def _overlapped(prob, K, **kw):
    bes = [oracle_backend(prob) for _ in range(K)]
    res = mcs.driver.run_overlapped(prob, bes, ensemble=True, **kw)
    for be in bes:
        be.destroy()
    return res


def _values(conv):
    return {it: rows[0].value for it, rows in conv.checks}


def earliest_record_round(values, rounds):
    """The earliest of `rounds`, from the second on, whose value lies below every earlier one by more than (1 + 1e-6)^2."""
    for k in range(1, len(rounds)):
        if all(values[rounds[k]] < values[r] / (1.0 + 1e-6) ** 2 for r in rounds[:k]):
            return rounds[k]
    return None


def test_overlapped_run_stops_at_the_round_that_meets_the_trigger():
    prob = make_problem(300, num_iterations=N_ITRS)
    K = 2
    never = ens.Trigger(0, "therm_sf_mom", "rms", 1e-12)
    first = _overlapped(prob, K, n_itrs=N_ITRS, triggers=[never])
    c1 = first.convergence
    rounds = [2, 4, 6]
    assert [it for it, _ in c1.checks] == rounds and c1.stopped_at == N_ITRS and not c1.satisfied
    v = _values(c1)
    print("rms relative error of therm_sf_mom by round end:", v)
    stop = earliest_record_round(v, rounds)
    assert stop is not None and stop >= 4, v
    trig = ens.Trigger(0, "therm_sf_mom", "rms", v[stop] * (1.0 + 1e-6))
    seen = []
    res = _overlapped(prob, K, n_itrs=N_ITRS, triggers=[trig], on_iteration_end=seen.append)
    c = res.convergence
    assert c.stopped_at == stop and c.satisfied and [it for it, _ in c.checks] == [r for r in rounds if r <= stop]
    assert seen == list(range(1, stop + 1)) and len(res.iter_finals) == stop
    for (it, rows), (it1, rows1) in zip(c.checks, c1.checks):
        assert it == it1 and rows[0].summary == rows1[0].summary and same_bits(rows[0].value, rows1[0].value)
        assert rows[0].summary.n == it and rows[0].met == (it == stop)
    # the prefix property: what a run of that length on fresh contexts hands back
    short = _overlapped(prob, K, n_itrs=stop)
    assert short.convergence is None
    assert bits_equal(res.tallies_f64, short.tallies_f64) and np.array_equal(res.tallies_i64, short.tallies_i64)
    assert len(res.per_species) == len(short.per_species) == stop
    for (ia, sa, fa, ja), (ib, sb, fb, jb) in zip(res.per_species, short.per_species):
        assert (ia, sa) == (ib, sb) and bits_equal(fa, fb) and np.array_equal(ja, jb)
    for slot in (0, 1):
        assert res.ensemble.count(slot) == short.ensemble.count(slot) == stop
        for a, b in zip(slot_vectors(res.ensemble, slot), slot_vectors(short.ensemble, slot)):
            assert bits_equal(a, b), slot
    assert res.ensemble.finalize_count == short.ensemble.finalize_count == stop
    for name in ens.FINALIZE_NAMES:
        assert bits_equal(res.ensemble.finalize_mean[name], short.ensemble.finalize_mean[name])
        assert bits_equal(res.ensemble.finalize_stderr[name], short.ensemble.finalize_stderr[name])
    assert res.steps_helix == short.steps_helix and res.steps_retro == short.steps_retro


def test_schedule_and_refusals():
    prob = make_problem(100, num_iterations=N_ITRS)
    trigs = [ens.Trigger(0, "pxx_flux", "max", 1e-12), ens.Trigger(1, "spectra_sf", "rms", 1e-12)]
    # one context: run's schedule and run's values
    be = oracle_backend(prob)
    e = ens.Ensemble.for_backend(be, 1)
    plain = mcs.driver.run(prob, be, n_itrs=5, max_pcuts=4, ensemble=e, triggers=trigs, min_iterations=2, check_every=2)
    be.destroy()
    one = _overlapped(prob, 1, n_itrs=5, max_pcuts=4, triggers=trigs, min_iterations=2, check_every=2)
    assert [it for it, _ in one.convergence.checks] == [it for it, _ in plain.convergence.checks] == [2, 4]
    assert one.convergence.stopped_at == plain.convergence.stopped_at == 5 and not one.convergence.satisfied
    for (_, rows), (_, rows_p) in zip(one.convergence.checks, plain.convergence.checks):
        for a, b in zip(rows, rows_p):
            assert a.summary == b.summary and same_bits(a.value, b.value) and a.met == b.met and a.predicted_samples == b.predicted_samples
    # a cap that is no multiple of K: rounds of 2, 2 and 1
    two = _overlapped(prob, 2, n_itrs=5, max_pcuts=4, triggers=trigs)
    assert [(it, rows[0].summary.n) for it, rows in two.convergence.checks] == [(2, 2), (4, 4), (5, 5)]
    assert two.convergence.stopped_at == 5 and two.ensemble.count(0) == 5 and len(two.iter_finals) == 5
    # min_iterations and check_every count iterations, checks fall on round ends: 3 -> the round end 4; the next one is due
    # from 4 + 3 = 7 iterations on, and the cap of 6 ends the run before that
    late = _overlapped(prob, 2, n_itrs=6, max_pcuts=4, triggers=trigs, min_iterations=3, check_every=3)
    assert [it for it, _ in late.convergence.checks] == [4]
    # refusals, before any iteration runs
    bes = [oracle_backend(prob), oracle_backend(prob)]
    ran = []
    for kw, match in ((dict(triggers=trigs), "ensemble=True"), (dict(triggers=trigs, ensemble=True, min_iterations=1), "min_iterations"),
                      (dict(triggers=trigs, ensemble=True, check_every=0), "check_every")):
        with pytest.raises(ValueError, match=match):
            mcs.driver.run_overlapped(prob, bes, n_itrs=2, max_pcuts=1, on_iteration_end=ran.append, **kw)
    with pytest.raises(KeyError):
        mcs.driver.run_overlapped(prob, bes, n_itrs=2, max_pcuts=1, ensemble=True, triggers=[ens.Trigger(1, "pxx_flux", "max", 0.1)],
                                  on_iteration_end=ran.append)
    assert ran == []
    for kw in (dict(), dict(triggers=[]), dict(triggers=None)):
        assert mcs.driver.run_overlapped(prob, bes, n_itrs=2, max_pcuts=1, ensemble=True, **kw).convergence is None
    for be in bes:
        be.destroy()
