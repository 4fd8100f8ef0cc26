"""The tcuts sample of the ensemble statistics on the device (mcs_ens_add_tcuts in csrc/mcs_ensemble.hip, through
ensemble.HipEnsemble) against ensemble.HostEnsemble fed the same TcutSpectra: count, mean and M2 of crafted samples bit for bit, the
merge, a summary of a momentum window of one spectrum row, a trigger on a quantile, a comparison of two slots, the refusals, and a
run of three iterations."""
import numpy as np
import pytest

import ens_compare_common as cmpc
import tcuts_common as tc
from conftest import mcs, make_problem, hip_backend
from ensemble_common import same_words
from ens_summary_common import as_dict, assert_exact, assert_sums, restate

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
EPS = 2.0 ** -53
SAMPLES = ("99_cuts_every_row", "99_cuts_three_live_apart", "99_cuts_two_live_apart")


@pytest.fixture(scope="module")
def fed():
    """One context of two species, three crafted samples of 99 cuts, and a device and a numpy accumulator that took each into the
    tcuts slot of species slot 1."""
    prob = tc.two_ion_problem(make_problem)
    hb = hip_backend(prob)
    e, h = ens.HipEnsemble(hb, 2), ens.HostEnsemble(prob.params, 2)
    specs = []
    for name in SAMPLES:
        tc.load_rows(hb, prob, 2, tc.scenarios(prob.params.num_psd_mom_bins)[name])
        spec = mcs.consumers.tcut_spectra(prob, hb, 2)
        e.add_tcuts(hb, 1, spec)
        h.add_tcuts(hb, 1, spec)
        specs.append(spec)
    yield prob, hb, e, h, specs
    e.destroy(); hb.destroy()


def test_count_mean_and_m2(fed):
    prob, hb, e, h, specs = fed
    s = e.tcuts_slot(1)
    assert e.count(s) == 3 and e.count(e.tcuts_slot(0)) == 0 and e.count(1) == 0 and e.count(e.escape_slot(1)) == 0 and e.tcuts_n == 99
    total = e.layout.tcuts_fields(99)["total"]
    assert total % 256 != 0            # (the tail of the grid-stride loop runs)
    for name in ens.TCUTS_NAMES:
        assert same_words(e.mean(s, name), h.mean(s, name)), f"mean of {name}"
        assert same_words(e.m2(s, name), h.m2(s, name)), f"M2 of {name}"
    assert same_words(e._read(s, 0, 0, total), h._read(s, 0, 0, total)) and same_words(e._read(s, 1, 0, total), h._read(s, 1, 0, total))
    assert h.m2(s, "spectrum").max() > 0 and np.isfinite(h.m2(s, "number")).all() and np.isnan(h.mean(s, "quantile")).any()
    with np.errstate(invalid="ignore"):
        assert same_words(e.stderr(s, "number"), np.sqrt(h.m2(s, "number") / 6.0))


def test_merge(fed):
    """Two accumulators with 2 + 1 samples merged: bit for bit the numpy ensemble's merge (Chan's formula), and the accumulator that
    took all three within the existing merge tests' bound (16 n 2^-53 of |mean|, and of the sum of squares for M2)."""
    prob, hb, e, h, specs = fed
    s = e.tcuts_slot(1)
    a, b, c = (ens.HipEnsemble(hb, 2) for _ in range(3))
    ha, hb_ = ens.HostEnsemble(prob.params, 2), ens.HostEnsemble(prob.params, 2)
    for k, name in enumerate(SAMPLES):
        tc.load_rows(hb, prob, 2, tc.scenarios(prob.params.num_psd_mom_bins)[name])
        spec = mcs.consumers.tcut_spectra(prob, hb, 2)
        (a if k < 2 else b).add_tcuts(hb, 1, spec)
        (ha if k < 2 else hb_).add_tcuts(hb, 1, spec)
    ha.merge(hb_)
    a.merge(b)
    c.merge(a)                                     # an accumulator without tcuts samples takes the source's number of cuts
    assert a.count(s) == 3 and b.count(s) == 1 and c.count(s) == 3 and c.tcuts_n == 99
    for acc in (a, c):
        for name in ens.TCUTS_NAMES:
            assert same_words(acc.mean(s, name), ha.mean(s, name)) and same_words(acc.m2(s, name), ha.m2(s, name)), name
    n = 3
    for name in ("spectrum", "number", "weight"):
        mean, m2 = a.mean(s, name), a.m2(s, name)
        sum_x2 = sum(getattr(p, name) * getattr(p, name) for p in specs)
        assert np.all(np.abs(mean - e.mean(s, name)) <= 16 * n * EPS * np.abs(e.mean(s, name))), name
        assert np.all(np.abs(m2 - e.m2(s, name)) <= 16 * n * EPS * sum_x2), name
    # another number of cuts: refused
    other = ens.HipEnsemble(hb, 2)
    tc.load_rows(hb, prob, 2, tc.scenarios(prob.params.num_psd_mom_bins)["three_cuts_three_live"])
    other.add_tcuts(hb, 1, mcs.consumers.tcut_spectra(prob, hb, 2))
    assert other.tcuts_n == 3
    with pytest.raises(RuntimeError, match="mcs_ens_merge: the accumulators' tcuts samples differ in n_tcuts"):
        a.merge(other)
    for acc in (a, b, c, other):
        acc.destroy()


def test_summary_trigger_and_comparison(fed):
    prob, hb, e, h, specs = fed
    NM = prob.params.num_psd_mom_bins + 2
    s = e.tcuts_slot(1)
    total = e.layout.tcuts_fields(99)["total"]
    mean, m2 = e._read(s, 0, 0, total), e._read(s, 1, 0, total)
    reqs = [ens.Request("spectrum", e.tcuts_row(0), 0.0, 0.3, (0, 60)), ens.Request("spectrum", e.tcuts_row(98), 1e-3, 0.1),
            ens.Request("number"), ens.Request("weight", e.tcuts_row(0), 0.0, 0.5), ens.Request("quantile", (1, 2), 0.0, 0.1, e.tcuts_row(0)),
            ens.Request("quantile", (0, 1)), ens.Request("index"), ens.Request("mean_log_p", e.tcuts_row(0))]
    got, host = e.summarize(s, reqs), h.summarize(s, reqs)
    for q, r, hr in zip(reqs, got, host):
        first, count = e.word_range(s, q.name, q.zones, q.bins)
        assert (first, count) == h.word_range(s, q.name, q.zones, q.bins)
        want = restate(mean[first:first + count], m2[first:first + count], 3, q.floor_frac, q.tol)
        assert r.n == 3 and hr.n == 3
        assert_exact(as_dict(r), want, repr(q)); assert_sums(as_dict(r), want, repr(q))
        assert_exact(as_dict(hr), want, repr(q)); assert_sums(as_dict(hr), want, repr(q))
    assert e.word_range(s, "spectrum", e.tcuts_row(0), (0, 60)) == (0, 60) and e.word_range(s, "spectrum", e.tcuts_row(98)) == (98 * NM, NM)
    assert got[0].n_selected > 3 and got[4].n_selected == 1 and got[4].n_nonfinite == 0 and got[5].n_nonfinite > 50 and got[6].n_nonfinite == 3
    # a trigger on the median momentum reached by the first cut (live in all three samples), and on a cut that was dead in one
    loose, tight, dead = (ens.Trigger(s, "quantile", "max", thr, zones=(0, 1), bins=e.tcuts_row(k), floor_frac=0.0) for thr, k in ((1.0, 0), (1e-9, 0), (1.0, 50)))
    for acc in (e, h):
        rows = mcs.driver._check_triggers(acc, [loose, tight, dead])
        assert [r.met for r in rows] == [True, False, False], [r.value for r in rows]
    dev, hst = mcs.driver._check_triggers(e, [loose])[0], mcs.driver._check_triggers(h, [loose])[0]
    assert cmpc.same_bits(dev.value, hst.value) and dev.value > 0
    # another accumulator with other samples: per-word z-scores of one cut
    b, hb_ = ens.HipEnsemble(hb, 2), ens.HostEnsemble(prob.params, 2)
    for name in ("99_cuts_three_live_apart", "99_cuts_every_row"):
        tc.load_rows(hb, prob, 2, tc.scenarios(prob.params.num_psd_mom_bins)[name])
        spec = mcs.consumers.tcut_spectra(prob, hb, 2)
        b.add_tcuts(hb, 0, spec); hb_.add_tcuts(hb, 0, spec)
    s0 = b.tcuts_slot(0)
    mb, qb = b._read(s0, 0, 0, total), b._read(s0, 1, 0, total)
    creqs = [ens.CompareRequest("spectrum", e.tcuts_row(0), 0.0, 2.0), ens.CompareRequest("number", None, 0.0, 1.0),
             ens.CompareRequest("quantile", (2, 3), 0.0, 1.0, e.tcuts_row(0))]
    diffs, hdiffs = e.compare(b, s, creqs, other_slot=s0), h.compare(hb_, s, creqs, other_slot=s0)
    for q, d, hd in zip(creqs, diffs, hdiffs):
        first, count = e.word_range(s, q.name, q.zones, q.bins)
        sl = slice(first, first + count)
        want = cmpc.restate(mean[sl], m2[sl], 3, mb[sl], qb[sl], 2, q.floor_frac, q.zcut)
        assert d.n_a == 3 and d.n_b == 2
        for res in (d, hd):
            cmpc.assert_exact(cmpc.as_dict(res), want, repr(q))
            cmpc.assert_sums(cmpc.as_dict(res), want, repr(q))
    assert diffs[0].n_selected >= 1 and diffs[1].n_selected > 3
    with pytest.raises(ValueError):
        e.compare(b, s, creqs, other_slot=b.escape_slot(0))
    # two slots of one accumulator
    tc.load_rows(hb, prob, 2, tc.scenarios(prob.params.num_psd_mom_bins)["99_cuts_every_row"])
    for _ in range(2):
        e.add_tcuts(hb, 0, mcs.consumers.tcut_spectra(prob, hb, 2))
    same = e.compare(e, s, [ens.CompareRequest("number")], other_slot=e.tcuts_slot(0))[0]
    assert same.n_a == 3 and same.n_b == 2
    b.destroy()


def test_refusals(fed):
    prob, hb, e, h, specs = fed
    s = e.tcuts_slot(1)
    nm = prob.params.num_psd_mom_bins
    before = (e.mean(s, "spectrum"), e.m2(s, "spectrum"))
    n0 = e.count(e.tcuts_slot(0))
    fresh = ens.HipEnsemble(hb, 2)
    tc.load_rows(hb, prob, 2, tc.scenarios(nm)["99_cuts_every_row"])
    # wrong order: begin_species, no mcs_tcut_spectra yet
    with pytest.raises(RuntimeError, match="mcs_ens_add_tcuts: the context needs an mcs_tcut_spectra since its last mcs_begin_species"):
        fresh.add_tcuts(hb, 0)
    mcs.consumers.tcut_spectra(prob, hb, 2)
    fresh.add_tcuts(hb, 0)
    assert fresh.count(fresh.tcuts_slot(0)) == 1 and fresh.tcuts_n == 99
    refused = [
        ("mcs_ens_add_tcuts", lambda: fresh.add_tcuts(hb, 0)),                                                  # a second sample from one call
        ("mcs_ens_add_tcuts", lambda: (mcs.consumers.tcut_spectra(prob, hb, 2), fresh.add_tcuts(hb, 2))),       # the iteration slot
        ("mcs_ens_add_tcuts", lambda: fresh.add_tcuts(hb, fresh.tcuts_slot(0))),                                # out of range
        ("mcs_ens_read", lambda: fresh.stderr(fresh.tcuts_slot(0), "number")),                                  # n = 1
        ("mcs_ens_read", lambda: fresh._read(fresh.tcuts_slot(1), 0, 0, 4)),                                    # never sampled
        ("mcs_ens_load_mean", lambda: e.load_mean(s, hb)),
    ]
    for who, call in refused:
        with pytest.raises(RuntimeError, match=who):
            call()
    # another number of cuts than the accumulator's first sample had
    tc.load_rows(hb, prob, 2, tc.scenarios(nm)["three_cuts_three_live"])
    mcs.consumers.tcut_spectra(prob, hb, 2)
    with pytest.raises(RuntimeError, match="had 3 time cuts, the accumulator's tcuts samples have 99"):
        fresh.add_tcuts(hb, 1)
    three = ens.HipEnsemble(hb, 2)
    for _ in range(2):
        three.add_tcuts(hb, 1)
        mcs.consumers.tcut_spectra(prob, hb, 2)
    assert three.tcuts_n == 3 and three.count(three.tcuts_slot(1)) == 2
    with pytest.raises(RuntimeError, match="mcs_ens_compare: the accumulators' tcuts samples differ in n_tcuts"):
        e.compare(three, s, [ens.CompareRequest("index")])
    with pytest.raises(RuntimeError, match="mcs_ens_summarize_merged: the accumulators' tcuts samples differ in n_tcuts"):
        e.summarize_merged([three], s, [ens.Request("index")])
    assert e.count(s) == 3 and e.count(e.tcuts_slot(0)) == n0
    assert same_words(before[0], e.mean(s, "spectrum")) and same_words(before[1], e.m2(s, "spectrum"))
    fresh.destroy(); three.destroy()


def test_a_run_of_three_iterations():
    """driver.run(finalize=True, tcuts=True, ensemble=HipEnsemble, n_itrs=3) at 4000 protons: three samples per species, three
    entries in RunResult.tcuts, and the ensemble's mean of number within 2 ulp per word of the mean of the three entries."""
    prob = make_problem(4000, num_iterations=3)
    hb = hip_backend(prob)
    e = ens.HipEnsemble(hb, 1)
    try:
        with pytest.raises(ValueError, match="tcuts slot needs tcuts=True"):
            mcs.driver.run(prob, hb, n_itrs=3, max_pcuts=12, finalize=True, ensemble=e, triggers=[ens.Trigger(e.tcuts_slot(0), "number", "max", 0.1)])
        res = mcs.driver.run(prob, hb, n_itrs=3, max_pcuts=12, finalize=True, tcuts=True, ensemble=e)
        s = e.tcuts_slot(0)
        assert e.count(s) == 3 and [(it, ion) for it, ion, _ in res.tcuts] == [(1, 1), (2, 1), (3, 1)] and e.tcuts_n == len(prob.tcuts)
        numbers = np.array([spec.number for _, _, spec in res.tcuts])
        assert all(spec.diag[1] == 0 for _, _, spec in res.tcuts) and np.all((numbers[:, 0] > 0.5) & (numbers[:, 0] < 1.5))
        want = (numbers[0] + numbers[1] + numbers[2]) / 3.0
        got = e.mean(s, "number")
        print("number, mean of three:", want.tolist(), "ensemble:", got.tolist(), "stderr:", e.stderr(s, "number").tolist())
        assert np.all(np.abs(got - want) <= 2 * np.spacing(np.abs(want)))
        h = ens.HostEnsemble(prob.params, 1)
        for _, _, spec in res.tcuts:
            h.add_tcuts(hb, 0, spec)
        for name in ens.TCUTS_NAMES:
            assert same_words(e.mean(s, name), h.mean(s, name)) and same_words(e.m2(s, name), h.m2(s, name)), name
        assert not np.array_equal(numbers[0], numbers[1])
    finally:
        e.destroy(); hb.destroy()
