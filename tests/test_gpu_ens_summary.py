"""mcs_ens_summarize (csrc/mcs_ensemble.hip) and what is built on it -- ensemble.HipEnsemble.summarize, ensemble.Trigger,
driver.run(triggers=...) -- against the plain-numpy restatement of ens_summary_common.py, on the crafted buffers of
test_gpu_ensemble.py: five samples on the stock binning, 100 decades of dynamic range, the 1e-99 floor in every seventh word,
one word in twenty the same in all samples (M2 = 0)."""
import math

import numpy as np
import pytest

from conftest import mcs, make_problem, hip_backend
from ensemble_common import AS_IS, INCREMENTS, assert_tail_is_exercised, bits_equal, crafted_buffers
from ens_summary_common import (FIELDS, as_dict, assert_exact, assert_sums, iteration_offsets, restate, same_bits, slot_vectors,
                                species_offsets, value_of)

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
N = 5


def feed(hb, e, bufs, L):
    """Every buffer as a species sample of slot 0 and as an iteration sample (every section changes between snapshot and sample)."""
    prev = np.zeros(L.total)
    for f, i in bufs:
        hb.write_tallies(prev, i)
        e.begin_iteration(hb)
        hb.write_tallies(f, i)
        e.add_species(hb, 0)
        e.add_iteration(hb)
        prev = f


def raw_summarize(e, slot, ranges):
    """One mcs_ens_summarize call for ranges [(first, count, floor_frac, tol)] -> [dict of FIELDS]."""
    rs = (mcs.capi.McsEnsRange * len(ranges))(*[mcs.capi.McsEnsRange(*r) for r in ranges])
    out = (mcs.capi.McsEnsSummary * len(ranges))()
    rc = e.lib.mcs_ens_summarize(e.h, slot, len(ranges), rs, out)
    assert rc == 0, e.lib.mcs_last_error().decode()
    return [{k: getattr(o, k) for k in FIELDS} for o in out]


def species_ranges(L, sp_off, total):
    """(ranges, pairs): the ranges of the exact-fields test for the species slot; pairs: indices (floor 0, floor 1e-3) of one range."""
    n_psd = int(np.prod(L.shapes["psd"]))
    per_zone = n_psd // L.n_grid
    r = [(0, total, 0.0, 0.1), (0, total, 1e-3, 0.1), (0, total, 1.0, 0.1)]
    pairs = [(0, 1)]
    for name, (first, shape) in sp_off.items():
        n = int(np.prod(shape))
        r += [(first, n, 1e-3, 0.05), (first, n, 1.0, 0.05)]
        # (not the marginals: each is about its largest term, and those all lie within three decades of one another)
        if 50 <= n < 100000 and not name.endswith(("_mom", "_tht")):
            r.append((first, n, 0.0, 0.05))
            pairs.append((len(r) - 1, len(r) - 3))
    r += [(12345, 1, 1e-3, 0.0), (777, 0, 1e-3, 0.0), (total, 0, 0.0, 0.0), (total - 1, 1, 0.0, 0.0),
          (4097, 300000, 1e-3, 0.2), (4097, 300001, 1e-3, 0.2), (4096, 300001, 1e-3, 0.2),       # odd .. odd, odd .. even, even .. odd
          (5, 2, 0.0, 0.0), (5, 1, 0.0, 0.0), (6, 1, 1.0, 0.0), (3, 4, 0.0, 0.0),
          (10 * per_zone, 27 * per_zone, 1e-3, 0.1),                                             # psd, zones 10 .. 36
          (1000, 50000, 1e-3, 0.1), (30000, 50000, 1e-3, 0.1)]                                   # overlapping
    return r, pairs


@pytest.fixture(scope="module")
def crafted():
    prob = make_problem(64)
    L = mcs.capi.Layout(prob.params)
    assert_tail_is_exercised(ens.EnsLayout(prob.params).fields)
    bufs = crafted_buffers(L, N)
    hb = hip_backend(prob)
    e = ens.HipEnsemble(hb, 1)
    feed(hb, e, bufs, L)
    sp_off, sp_total = species_offsets(L)
    it_off, it_total = iteration_offsets(L, INCREMENTS + AS_IS)
    assert sp_total == e.layout.species_total and it_total == e.layout.iteration_total
    assert sp_total % 256 != 0 and it_total % 256 != 0
    vec = {slot: slot_vectors(e, slot) for slot in (0, 1)}
    # the ranges of both slots, one call each, and the restatement of every range: computed once, shared by the tests
    ranges = {}
    ranges[0], pairs0 = species_ranges(L, sp_off, sp_total)
    ranges[1] = [(0, it_total, ff, 0.1) for ff in (0.0, 1e-3, 1.0)]
    for name, (first, shape) in it_off.items():
        ranges[1] += [(first, int(np.prod(shape)), 1e-3, 0.05), (first, int(np.prod(shape)), 1.0, 0.05)]
    ranges[1] += [(1, it_total - 2, 1e-3, 0.3), (it_total - 1, 1, 0.0, 0.0)]
    pairs = {0: pairs0, 1: [(0, 1)]}
    want = {slot: [restate(vec[slot][0][f:f + c], vec[slot][1][f:f + c], N, ff, tol) for f, c, ff, tol in ranges[slot]] for slot in (0, 1)}
    got = {slot: raw_summarize(e, slot, ranges[slot]) for slot in (0, 1)}
    yield dict(prob=prob, L=L, bufs=bufs, hb=hb, e=e, sp_off=sp_off, it_off=it_off, vec=vec, ranges=ranges, pairs=pairs, want=want, got=got)
    e.destroy(); hb.destroy()


def test_exact_fields(crafted):
    c = crafted
    for slot in (0, 1):
        assert len(c["ranges"][slot]) <= 256
        for r, got, want in zip(c["ranges"][slot], c["got"][slot], c["want"][slot]):
            assert_exact(got, want, f"slot {slot} range {r}")
            assert r[1] == 0 or want["n_selected"] >= 1, r
            assert want["n_nonfinite"] == 0
        for k0, k1 in c["pairs"][slot]:
            assert c["ranges"][slot][k0][:2] == c["ranges"][slot][k1][:2] and c["ranges"][slot][k0][2] == 0.0 and c["ranges"][slot][k1][2] == 1e-3
            assert c["want"][slot][k1]["n_selected"] < c["want"][slot][k0]["n_selected"], c["ranges"][slot][k0]
    # constant words are there (rel = 0 is a value like any other), and Ensemble.summarize maps names and zones to these ranges
    mean, m2 = c["vec"][0]
    assert np.count_nonzero((m2 == 0) & (mean > 1e-90)) > mean.size // 30
    e, ng = c["e"], c["prob"].params.n_grid
    reqs = [ens.Request(name, None, 1e-3, 0.05) for name in c["sp_off"]] + [ens.Request("psd", (10, 37), 1e-3, 0.1)]
    got = e.summarize(0, reqs)
    for q, s in zip(reqs, got):
        first, count = e.word_range(0, q.name, q.zones)
        k = c["ranges"][0].index((first, count, q.floor_frac, q.tol))
        assert as_dict(s) == c["got"][0][k] and s.n == N, q
    with pytest.raises(ValueError, match="zone"):
        e.summarize(0, [ens.Request("esc_psd_up", (0, 1))])
    first, shape = c["it_off"]["spectra_sf"]
    k = c["ranges"][1].index((first, int(np.prod(shape)), 1e-3, 0.05))
    full, zoned = e.summarize(1, [ens.Request("spectra_sf", None, 1e-3, 0.05), ens.Request("spectra_sf", (0, ng), 1e-3, 0.05)])
    assert as_dict(full) == as_dict(zoned) == c["got"][1][k]


def test_sums_and_repeatability(crafted):
    c = crafted
    worst = 0.0
    for slot in (0, 1):
        for r, got, want in zip(c["ranges"][slot], c["got"][slot], c["want"][slot]):
            assert_sums(got, want, f"slot {slot} range {r}")
            for k in ("sum_se", "sum_abs_mean", "sum_rel2"):
                if want[k] > 0:
                    worst = max(worst, abs(got[k] - want[k]) / want[k] / 2.0 ** -53)
        again = raw_summarize(c["e"], slot, c["ranges"][slot])
        for r, a, b in zip(c["ranges"][slot], again, c["got"][slot]):
            for k in FIELDS:
                assert same_bits(a[k], b[k]) if isinstance(b[k], float) else a[k] == b[k], (slot, r, k)
    print(f"sums against fsum: worst difference {worst:.2f} units of 2^-53 relative (the bound is n_selected of them)")


def test_ties_keep_the_lower_word(crafted):
    c = crafted
    L = c["L"]
    n_psd = int(np.prod(L.shapes["psd"]))
    k = c["ranges"][0].index((0, n_psd, 1e-3, 0.05))            # psd is the first part of both the buffer and the sample vector
    wa = c["want"][0][k]["argmax"]
    assert 0 <= wa < n_psd - 2
    higher = [wa + 1, n_psd - 1]
    bufs = [(f.copy(), i) for f, i in c["bufs"]]
    for f, _ in bufs:
        f[higher] = f[wa]
    hb = hip_backend(c["prob"])
    e = ens.HipEnsemble(hb, 1)
    feed(hb, e, bufs, L)
    mean, m2 = slot_vectors(e, 0)
    for w in higher:
        assert same_bits(mean[w], mean[wa]) and same_bits(m2[w], m2[wa])
    ranges = [(0, n_psd, 1e-3, 0.05), (0, mean.size, 1e-3, 0.05), (wa, n_psd - wa, 1e-3, 0.05), (wa | 1, n_psd - (wa | 1), 1.0, 0.0)]
    got = raw_summarize(e, 0, ranges)
    for r, g in zip(ranges, got):
        want = restate(mean[r[0]:r[0] + r[1]], m2[r[0]:r[0] + r[1]], N, r[2], r[3])
        assert_exact(g, want, f"range {r}")
    assert got[0]["argmax"] == wa and got[2]["argmax"] == 0 and same_bits(got[0]["max_rel"], c["want"][0][k]["max_rel"])
    e.destroy(); hb.destroy()


def test_non_finite_words_are_counted_and_left_out(crafted):
    c = crafted
    L = c["L"]
    n_psd = int(np.prod(L.shapes["psd"]))
    bufs = [(f.copy(), i) for f, i in c["bufs"]]
    nan_words, inf_words, huge = [5, 4098, 100001], [6, 250000, n_psd - 1], 9001
    bufs[2][0][nan_words] = np.nan
    bufs[2][0][inf_words] = [np.inf, -np.inf, np.inf]
    bufs[3][0][huge] = 1e200            # a finite mean, 2.5e199, the largest of all -- with an infinite M2: no finite word
    flux = L.offsets["pxx_flux"]
    bufs[1][0][flux + 40] = np.nan
    hb = hip_backend(c["prob"])
    e = ens.HipEnsemble(hb, 1)
    feed(hb, e, bufs, L)
    mean, m2 = slot_vectors(e, 0)
    assert np.isfinite(mean[huge]) and np.isinf(m2[huge]) and abs(mean[huge]) == np.abs(mean[np.isfinite(mean)]).max()
    sp = c["sp_off"]
    ranges = [(0, n_psd, 1e-3, 0.05), (0, n_psd, 0.0, 0.05), (0, mean.size, 1e-3, 0.05), (5, 2, 0.0, 0.0), (5, 1, 0.0, 0.0),
              (sp["pxx_flux"][0], L.n_grid, 1e-3, 0.05), (sp["psd_mom"][0], int(np.prod(sp["psd_mom"][1])), 1e-3, 0.05), (8000, 2001, 1.0, 0.0)]
    got = raw_summarize(e, 0, ranges)
    for r, g in zip(ranges, got):
        want = restate(mean[r[0]:r[0] + r[1]], m2[r[0]:r[0] + r[1]], N, r[2], r[3])
        assert_exact(g, want, f"range {r}")
        assert_sums(g, want, f"range {r}")
    assert got[0]["n_nonfinite"] == 7 and got[3]["n_nonfinite"] == 2 and got[3]["n_selected"] == 0 and got[3]["argmax"] == -1
    assert got[5]["n_nonfinite"] == 1 and got[5]["n_selected"] >= 1 and got[6]["n_nonfinite"] >= 1
    assert got[0]["amax"] < 1e42 and got[0]["n_selected"] >= 1 and got[7]["n_selected"] >= 1
    # a trigger on such a part is not met, whatever its value
    for name in ("psd", "pxx_flux"):
        t = ens.Trigger(0, name, "max", 1e9)
        s = e.summarize(0, [t.request])[0]
        assert s.n_nonfinite > 0 and t.value(s) <= t.threshold and not t.met(s)
    t = ens.Trigger(0, "pxz_flux", "max", 1e9)
    assert t.met(e.summarize(0, [t.request])[0])
    e.destroy(); hb.destroy()


def test_refusals_change_nothing(crafted):
    c = crafted
    hb, e = c["hb"], c["e"]
    lib, R, S = e.lib, mcs.capi.McsEnsRange, mcs.capi.McsEnsSummary
    wide = ens.HipEnsemble(hb, 2)                       # slot 1 of it: a species slot with one sample
    hb.write_tallies(*c["bufs"][-1])
    wide.add_species(hb, 1)
    total = c["vec"][0][0].size
    out = (S * 257)()
    nan = float("nan")

    def one(first, count, ff=1e-3, tol=0.0):
        return (R * 1)(R(first, count, ff, tol))
    refused = [
        lambda: lib.mcs_ens_summarize(None, 0, 1, one(0, 1), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, None, out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, one(0, 1), None),
        lambda: lib.mcs_ens_summarize(e.h, 2, 1, one(0, 1), out),
        lambda: lib.mcs_ens_summarize(e.h, -1, 1, one(0, 1), out),
        lambda: lib.mcs_ens_summarize(wide.h, 1, 1, one(0, 1), out),            # n = 1
        lambda: lib.mcs_ens_summarize(wide.h, 0, 1, one(0, 1), out),            # n = 0
        lambda: lib.mcs_ens_summarize(e.h, 0, -1, one(0, 1), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 257, (R * 257)(), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, one(-1, 2), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, one(total - 1, 2), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, one(total + 1, 0), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, one(0, -1), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, one(2 ** 62, 2 ** 62), out),
        lambda: lib.mcs_ens_summarize(e.h, 1, 1, one(0, c["vec"][1][0].size + 1), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, one(0, 1, nan), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, one(0, 1, -0.1), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, one(0, 1, 1.5), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, one(0, 1, 1e-3, -1.0), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 1, one(0, 1, 1e-3, nan), out),
        lambda: lib.mcs_ens_summarize(e.h, 0, 2, (R * 2)(R(0, 1, 0.0, 0.0), R(0, 1, 2.0, 0.0)), out),     # the second range of a call
    ]
    for k, call in enumerate(refused):
        assert call() != 0, k
        assert b"mcs_ens_summarize" in lib.mcs_last_error(), (k, lib.mcs_last_error())
    assert lib.mcs_ens_summarize(e.h, 0, 0, None, None) == 0                     # nothing to do
    for slot in (0, 1):
        mean, m2 = slot_vectors(e, slot)
        assert bits_equal(mean, c["vec"][slot][0]) and bits_equal(m2, c["vec"][slot][1])
        assert e.count(slot) == N
    # the context and the accumulator go on working
    k = 1
    assert raw_summarize(e, 0, [c["ranges"][0][k]])[0] == c["got"][0][k]
    wide.add_species(hb, 1)
    assert wide.summarize(1, [ens.Request("pxx_flux")])[0].n == 2
    wide.destroy()


N_ITRS, N_PCUTS = 6, 6          # (the driver fixture of test_gpu_ensemble.py: 2000 protons, its N_PCUTS; six iterations)
# Two runs of the transport differ in the last bits of their fp64 tallies by the order in which its waves' atomic adds arrive (1e-11 of
# an array's maximum is what every comparison of two GPU runs in this suite allows, test_gpu_parity.py).  A test that holds one run
# against another bit for bit therefore gives every launch ONE wave (mcs_set_launch: one workgroup of 64 threads): the adds then come
# in that wave's program order.  With the default geometry the "max" value of pxx_flux after iteration 4 was measured as
# 0.015321411467651857 in one run and 0.01532141146765186 in the next.
ONE_WAVE = (1, 64)


def _restated_max(e):
    n = e.count(0)
    r = restate(e.mean(0, "pxx_flux"), e.m2(0, "pxx_flux"), n, 1e-3, 0.0)
    return r, value_of("max", r, n)


@pytest.fixture(scope="module")
def plain_run():
    """A run without triggers, one wave per launch (ONE_WAVE); at every iteration end the restatement's "max" value of pxx_flux from
    the slot as it then stands."""
    prob = make_problem(2000, num_iterations=N_ITRS)
    hb = hip_backend(prob)
    hb.set_launch(*ONE_WAVE)
    e = ens.Ensemble.for_backend(hb, 1)
    seq = {}

    def record(it):
        if e.count(0) >= 2:
            seq[it] = _restated_max(e)
    res = mcs.driver.run(prob, hb, n_itrs=N_ITRS, max_pcuts=N_PCUTS, ensemble=e, on_iteration_end=record, fused_pcuts=False)
    assert res.convergence is None
    e.destroy(); hb.destroy()
    return prob, seq


def _run(prob, launch=None, **kw):
    hb = hip_backend(prob)
    if launch:
        hb.set_launch(*launch)
        kw["fused_pcuts"] = False           # (the fused loop takes no explicit launch geometry)
    e = ens.Ensemble.for_backend(hb, 1)
    res = mcs.driver.run(prob, hb, max_pcuts=N_PCUTS, ensemble=e, **kw)
    vec = [slot_vectors(e, slot) for slot in (0, 1)]
    n = [e.count(0), e.count(1)]
    e.destroy(); hb.destroy()
    return res, vec, n


def test_driver_stops_at_the_expected_iteration(plain_run):
    """The stop rule against a SECOND run, bit for bit: the threshold is the value the plain run recorded after iteration 4, the run
    with the trigger has to stop where the recorded sequence first meets it, show the recorded rows, and leave what a plain run of
    that length leaves.

    Both runs, and the plain run of that length, give every launch one wave (ONE_WAVE), so that a run repeats bit for bit;
    test_rows_are_the_restatement_of_the_slot_they_were_taken_from checks the rows with the default geometry, against the
    accumulator of the run they were taken in."""
    prob, seq = plain_run
    assert sorted(seq) == list(range(2, N_ITRS + 1))
    threshold = seq[4][1]
    expected = next(it for it in range(2, N_ITRS + 1) if seq[it][1] <= threshold)
    print("max relative error of pxx_flux by iteration:", {it: v for it, (r, v) in seq.items()}, "-> expected stop", expected)
    assert 2 < expected < N_ITRS
    trig = ens.Trigger(0, "pxx_flux", "max", threshold)
    own = {}
    res, vec, n = _run(prob, ONE_WAVE, n_itrs=N_ITRS, triggers=[trig], on_iteration_end=lambda it: own.__setitem__(it, None))
    conv = res.convergence
    print("checks of the run with the trigger:", [(it, rows[0].value, rows[0].met) for it, rows in conv.checks], "stopped at", conv.stopped_at)
    assert conv.stopped_at == expected and conv.satisfied and [it for it, _ in conv.checks] == list(range(2, expected + 1))
    assert sorted(own) == list(range(1, expected + 1))
    for it, rows in conv.checks:
        (row,) = rows
        assert row.trigger is trig and row.summary.n == it
        assert_exact(as_dict(row.summary), seq[it][0], f"iteration {it}")
        assert_sums(as_dict(row.summary), seq[it][0], f"iteration {it}")
        assert same_bits(row.value, seq[it][1]) and row.met == (it == expected)
        assert row.predicted_samples == math.ceil(it * (seq[it][1] / threshold) ** 2)
    # the prefix property
    short, vec_s, n_s = _run(prob, ONE_WAVE, n_itrs=expected)
    assert n == n_s == [expected, expected] and len(res.per_species) == len(short.per_species) == expected
    for (ia, sa, fa, ja), (ib, sb, fb, jb) in zip(res.per_species, short.per_species):
        assert (ia, sa) == (ib, sb) and bits_equal(fa, fb) and np.array_equal(ja, jb), (ia, sa)
    for slot in (0, 1):
        for a, b in zip(vec[slot], vec_s[slot]):
            assert bits_equal(a, b), slot


def test_rows_are_the_restatement_of_the_slot_they_were_taken_from(plain_run):
    """The run with a trigger against ITSELF: every check's row equals the restatement of the accumulator as it stands at that
    iteration end (the check comes before on_iteration_end), and the run stops at the first check that meets the threshold."""
    prob, seq = plain_run
    threshold = seq[4][1] * (1.0 + 1e-6)          # (two GPU runs differ in the last bits of their tallies: clear of them)
    hb = hip_backend(prob)
    e = ens.Ensemble.for_backend(hb, 1)
    own = {}
    trig = ens.Trigger(0, "pxx_flux", "max", threshold)
    res = mcs.driver.run(prob, hb, n_itrs=N_ITRS, max_pcuts=N_PCUTS, ensemble=e, triggers=[trig],
                         on_iteration_end=lambda it: own.__setitem__(it, _restated_max(e) if e.count(0) >= 2 else None))
    conv = res.convergence
    assert conv.satisfied and 2 < conv.stopped_at < N_ITRS and e.count(0) == e.count(1) == conv.stopped_at
    assert [it for it, _ in conv.checks] == list(range(2, conv.stopped_at + 1))
    for it, rows in conv.checks:
        r, v = own[it]
        assert_exact(as_dict(rows[0].summary), r, f"iteration {it}")
        assert_sums(as_dict(rows[0].summary), r, f"iteration {it}")
        assert same_bits(rows[0].value, v) and rows[0].met == (v <= threshold) == (it == conv.stopped_at)
        assert abs(v - seq[it][1]) <= 1e-6 * seq[it][1]          # (tallies to 1e-11 of their maximum, relative errors of 1e-2 of them)
    e.destroy(); hb.destroy()


def test_driver_runs_to_the_cap_when_the_threshold_is_out_of_reach(plain_run):
    prob, seq = plain_run
    n_itrs = 3
    trig = ens.Trigger(0, "pxx_flux", "max", 1e-13)
    res, vec, n = _run(prob, n_itrs=n_itrs, triggers=[trig])
    conv = res.convergence
    assert conv.stopped_at == n_itrs and not conv.satisfied and n == [n_itrs, n_itrs] and len(res.per_species) == n_itrs
    assert [it for it, _ in conv.checks] == [2, 3]
    for it, rows in conv.checks:
        assert not rows[0].met and rows[0].predicted_samples > n_itrs
    hb = hip_backend(prob)
    with pytest.raises(ValueError, match="triggers"):
        mcs.driver.run(prob, hb, n_itrs=1, max_pcuts=1, triggers=[trig])
    with pytest.raises(ValueError, match="min_iterations"):
        mcs.driver.run(prob, hb, n_itrs=1, max_pcuts=1, ensemble=ens.HostEnsemble(prob.params, 1), triggers=[trig], min_iterations=1)
    hb.destroy()
