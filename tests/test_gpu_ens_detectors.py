"""The detectors sample of the ensemble statistics on the device (mcs_ens_add_detectors in csrc/mcs_ensemble.hip, through
ensemble.HipEnsemble): count, mean and M2 of three crafted samples word for word against the update rule of include/mcs.h restated
here and against ensemble.HostEnsemble fed the same DetectorSpectra, the NaN words, the merge of two accumulators, a summary and a
comparison over gradient and over quantile, and the refusals."""
import numpy as np
import pytest

import ens_compare_common as cmpc
import detectors_common as dc
from conftest import mcs, make_problem, hip_backend
from ensemble_common import same_words
from ens_summary_common import as_dict, assert_exact, assert_sums, restate

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
EPS = 2.0 ** -53
SAMPLES = ("three_upstream_dense", "three_one_dead", "three_upstream_dense_b")       # (the same positions and window)


def sample_scenarios(prob):
    nm = prob.params.num_psd_mom_bins
    S = dc.scenarios(nm, prob.params.n_grid)
    R = dc.crafted_rows(nm, seed=1)
    S["three_upstream_dense_b"] = dc.Scenario([R["dense_0"], R["dense_1"], R["dense_2"]], [R["full_0"], R["full_1"], R["full_2"]], [-0.5, -0.3, -0.1],
                                              (0, nm + 1))
    R0 = dc.crafted_rows(nm)
    S["three_one_dead"] = dc.Scenario([R0["full_0"], R0["full_1"], R0["full_2"]], [R0["dead"], R0["dense_4"], R0["dead"]], [-0.5, -0.3, -0.1], (0, nm + 1))
    return S


def spectra(prob, hb, name):
    sc = sample_scenarios(prob)[name]
    dc.load_rows(hb, prob, 2, sc)
    return mcs.consumers.detector_spectra(prob, hb, 2, window=sc.window)


@pytest.fixture(scope="module")
def fed():
    """One context of two species, three crafted samples of three detectors, and a device and a numpy accumulator that took each into
    the detectors slot of species slot 1."""
    prob = dc.two_ion_problem(make_problem)
    prob.rg0 = dc.X_UNIT
    hb = hip_backend(prob)
    e, h = ens.HipEnsemble(hb, 2), ens.HostEnsemble(prob.params, 2)
    specs = []
    for name in SAMPLES:
        spec = spectra(prob, hb, name)
        e.add_detectors(hb, 1, spec)
        h.add_detectors(hb, 1, spec)
        specs.append(spec)
    yield prob, hb, e, h, specs
    e.destroy(); hb.destroy()


def test_count_mean_and_m2(fed):
    """n += 1; d = x - mean; mean = mean + d / n; M2 = M2 + d * (x - mean), per word (include/mcs.h)."""
    prob, hb, e, h, specs = fed
    s = e.detectors_slot(1)
    assert e.count(s) == 3 and e.count(e.detectors_slot(0)) == 0 and e.count(1) == 0 and e.count(e.tcuts_slot(1)) == 0
    assert e.detectors_settings == specs[0].settings() and e.detectors_settings[0] == 3
    total = e.layout.detectors_fields(3)["total"]
    assert total == specs[0].words().size and total % 256 != 0            # (the tail of the grid-stride loop runs)
    mean, m2 = np.zeros(total), np.zeros(total)
    with np.errstate(invalid="ignore"):
        for n, spec in enumerate(specs, 1):
            x = spec.words()
            d = x - mean
            mean = mean + d / float(n)
            m2 = m2 + d * (x - mean)
    assert same_words(e._read(s, 0, 0, total), mean) and same_words(e._read(s, 1, 0, total), m2)
    for name in ens.DETECTORS_NAMES:
        assert same_words(e.mean(s, name), h.mean(s, name)), f"mean of {name}"
        assert same_words(e.m2(s, name), h.m2(s, name)), f"M2 of {name}"
    assert h.m2(s, "spectrum").max() > 0 and np.isfinite(h.m2(s, "number")).all() and np.isnan(h.mean(s, "quantile")).any()
    assert np.isnan(mean).sum() == np.isnan(np.sum([p.words() for p in specs], axis=0)).sum() > 0      # a NaN in any sample stays


def test_nan_words_meet_no_trigger(fed):
    prob, hb, e, h, specs = fed
    NM = prob.params.num_psd_mom_bins + 2
    s = e.detectors_slot(1)
    # rows (1, 0) and (1, 2) were dead in the second sample, row (0, 2) live in all; gradient[nmom+1] is NaN in every sample
    reqs = [ens.Request("mean_log_p", zones=e.detectors_row(1, 0)), ens.Request("mean_log_p", zones=e.detectors_row(0, 2)),
            ens.Request("gradient", zones=(NM - 1, NM)), ens.Request("quantile", (0, 1), bins=e.detectors_row(1, 2))]
    for acc in (e, h):
        got = acc.summarize(s, reqs)
        assert [r.n_nonfinite for r in got] == [1, 0, 1, 1] and [r.n_selected for r in got] == [0, 1, 0, 0]
    dead, alive, grad = (ens.Trigger(s, "mean_log_p", "max", 1e30, zones=e.detectors_row(1, 0)), ens.Trigger(s, "mean_log_p", "max", 1e30, zones=e.detectors_row(0, 2)),
                         ens.Trigger(s, "gradient", "max", 1e30, zones=(NM - 1, NM)))
    for acc in (e, h):
        rows = mcs.driver._check_triggers(acc, [dead, alive, grad])
        assert [r.met for r in rows] == [False, True, False], [r.value for r in rows]


def test_merge(fed):
    """Two accumulators with 2 + 1 samples merged: bit for bit the numpy ensemble's merge (Chan's formula), and the accumulator that
    took all three within the existing merge tests' bound (16 n 2^-53 of |mean|, and of the sum of squares for M2)."""
    prob, hb, e, h, specs = fed
    s = e.detectors_slot(1)
    a, b, c = (ens.HipEnsemble(hb, 2) for _ in range(3))
    ha, hb_ = ens.HostEnsemble(prob.params, 2), ens.HostEnsemble(prob.params, 2)
    for k, name in enumerate(SAMPLES):
        spec = spectra(prob, hb, name)
        (a if k < 2 else b).add_detectors(hb, 1, spec)
        (ha if k < 2 else hb_).add_detectors(hb, 1, spec)
    ha.merge(hb_)
    a.merge(b)
    c.merge(a)                                     # an accumulator without detectors samples takes the source's settings
    assert a.count(s) == 3 and b.count(s) == 1 and c.count(s) == 3 and c.detectors_settings == specs[0].settings()
    for acc in (a, c):
        for name in ens.DETECTORS_NAMES:
            assert same_words(acc.mean(s, name), ha.mean(s, name)) and same_words(acc.m2(s, name), ha.m2(s, name)), name
    n = 3
    for name in ("spectrum", "number", "dndp"):
        mean, m2 = a.mean(s, name), a.m2(s, name)
        sum_x2 = sum(getattr(p, name) * getattr(p, name) for p in specs).reshape(mean.shape)
        assert np.all(np.abs(mean - e.mean(s, name)) <= 16 * n * EPS * np.abs(e.mean(s, name))), name
        assert np.all(np.abs(m2 - e.m2(s, name)) <= 16 * n * EPS * sum_x2), name
    # other settings (five detectors): refused; c took a's settings with the merge, so a sample with others is refused there too
    other = ens.HipEnsemble(hb, 2)
    other.add_detectors(hb, 1, spectra(prob, hb, "five_unsorted"))
    assert other.detectors_settings[0] == 5
    with pytest.raises(RuntimeError, match="mcs_ens_merge: the settings of the accumulators' detectors samples differ"):
        a.merge(other)
    with pytest.raises(RuntimeError, match="mcs_ens_add_detectors: the settings of the context's mcs_detector_spectra"):
        c.add_detectors(hb, 0, spectra(prob, hb, "five_unsorted"))
    for acc in (a, b, c, other):
        acc.destroy()


def test_summary_and_comparison(fed):
    prob, hb, e, h, specs = fed
    NM = prob.params.num_psd_mom_bins + 2
    s = e.detectors_slot(1)
    total = e.layout.detectors_fields(3)["total"]
    mean, m2 = e._read(s, 0, 0, total), e._read(s, 1, 0, total)
    reqs = [ens.Request("gradient", (0, NM), 0.0, 0.3), ens.Request("gradient", (3, 40), 1e-3, 0.1), ens.Request("quantile", (1, 2), 0.0, 0.1, e.detectors_row(0, 2)),
            ens.Request("quantile", (0, 1)), ens.Request("spectrum", e.detectors_row(1, 1), 0.0, 0.3, (0, 60)), ens.Request("dndp", e.detectors_row(0, 2)),
            ens.Request("number"), ens.Request("slope"), ens.Request("mean_log_p", e.detectors_row(1, 1))]
    got, host = e.summarize(s, reqs), h.summarize(s, reqs)
    for q, r, hr in zip(reqs, got, host):
        first, count = e.word_range(s, q.name, q.zones, q.bins)
        assert (first, count) == h.word_range(s, q.name, q.zones, q.bins)
        want = restate(mean[first:first + count], m2[first:first + count], 3, q.floor_frac, q.tol)
        assert r.n == 3 and hr.n == 3
        assert_exact(as_dict(r), want, repr(q)); assert_sums(as_dict(r), want, repr(q))
        assert_exact(as_dict(hr), want, repr(q)); assert_sums(as_dict(hr), want, repr(q))
    assert e.word_range(s, "gradient", (0, NM)) == (12 * NM + 36, NM) and e.word_range(s, "spectrum", e.detectors_row(1, 1), (0, 60)) == (4 * NM, 60)
    assert 1 <= got[0].n_nonfinite < NM - NM // 3 and got[2].n_selected == 1 and got[2].n_nonfinite == 0 and got[3].n_nonfinite >= 2
    # another accumulator with other samples: per-word z-scores of the gradient and of a quantile
    b, hb_ = ens.HipEnsemble(hb, 2), ens.HostEnsemble(prob.params, 2)
    for name in ("three_upstream_dense_b", "three_upstream_dense"):
        spec = spectra(prob, hb, name)
        b.add_detectors(hb, 0, spec); hb_.add_detectors(hb, 0, spec)
    s0 = b.detectors_slot(0)
    mb, qb = b._read(s0, 0, 0, total), b._read(s0, 1, 0, total)
    creqs = [ens.CompareRequest("gradient", None, 0.0, 2.0), ens.CompareRequest("quantile", (2, 3), 0.0, 1.0, e.detectors_row(0, 2)),
             ens.CompareRequest("quantile", (0, 1), 0.0, 1.0), ens.CompareRequest("number", None, 0.0, 1.0)]
    diffs, hdiffs = e.compare(b, s, creqs, other_slot=s0), h.compare(hb_, s, creqs, other_slot=s0)
    for q, d, hd in zip(creqs, diffs, hdiffs):
        first, count = e.word_range(s, q.name, q.zones, q.bins)
        sl = slice(first, first + count)
        want = cmpc.restate(mean[sl], m2[sl], 3, mb[sl], qb[sl], 2, q.floor_frac, q.zcut)
        assert d.n_a == 3 and d.n_b == 2
        for res in (d, hd):
            cmpc.assert_exact(cmpc.as_dict(res), want, repr(q))
            cmpc.assert_sums(cmpc.as_dict(res), want, repr(q))
    assert diffs[3].n_selected >= 1 and np.isfinite(mean[12 * NM + 36:12 * NM + 36 + NM]).sum() >= NM // 3
    with pytest.raises(ValueError):
        e.compare(b, s, creqs, other_slot=b.tcuts_slot(0))
    b.destroy()


def test_refusals(fed):
    prob, hb, e, h, specs = fed
    s = e.detectors_slot(1)
    nm = prob.params.num_psd_mom_bins
    before = (e.mean(s, "spectrum"), e.m2(s, "spectrum"))
    n0 = e.count(e.detectors_slot(0))
    fresh = ens.HipEnsemble(hb, 2)
    sc = sample_scenarios(prob)["three_upstream_dense"]
    dc.load_rows(hb, prob, 2, sc)
    # wrong order: begin_species, no mcs_detector_spectra yet
    with pytest.raises(RuntimeError, match="mcs_ens_add_detectors: the context needs an mcs_detector_spectra since its last mcs_begin_species"):
        fresh.add_detectors(hb, 0)
    first = mcs.consumers.detector_spectra(prob, hb, 2, window=sc.window)
    fresh.add_detectors(hb, 0, first)
    assert fresh.count(fresh.detectors_slot(0)) == 1 and fresh.detectors_settings == first.settings()
    again = lambda window=sc.window: mcs.consumers.detector_spectra(prob, hb, 2, window=window)
    refused = [
        ("mcs_ens_add_detectors", lambda: fresh.add_detectors(hb, 0)),                                              # a second sample from one call
        ("mcs_ens_add_detectors", lambda: (again(), fresh.add_detectors(hb, 2))),                                   # the iteration slot
        ("mcs_ens_add_detectors", lambda: fresh.add_detectors(hb, fresh.detectors_slot(0))),                        # out of range
        ("mcs_ens_read", lambda: fresh.stderr(fresh.detectors_slot(0), "number")),                                  # n = 1
        ("mcs_ens_read", lambda: fresh._read(fresh.detectors_slot(1), 0, 0, 4)),                                    # never sampled
        ("mcs_ens_load_mean", lambda: e.load_mean(s, hb)),
        ("window \\[3, 50\\)", lambda: (again((3, 50)), fresh.add_detectors(hb, 1))),                               # another window
    ]
    for who, call in refused:
        with pytest.raises(RuntimeError, match=who):
            call()
    # another x_unit, then another number of detectors than the accumulator's first sample had
    hb.detector_spectra(mcs.consumers.consumer_tables(prob, 2), sc.window[0], sc.window[1], dc.up(dc.X_UNIT))
    with pytest.raises(RuntimeError, match="mcs_ens_add_detectors: the settings of the context's mcs_detector_spectra"):
        fresh.add_detectors(hb, 1)
    spectra(prob, hb, "five_unsorted")
    with pytest.raises(RuntimeError, match="\\(5 detectors, window .* \\(3 detectors, window"):
        fresh.add_detectors(hb, 1)
    five = ens.HipEnsemble(hb, 2)
    for _ in range(2):
        five.add_detectors(hb, 1, spectra(prob, hb, "five_unsorted"))
    assert five.detectors_settings[0] == 5 and five.count(five.detectors_slot(1)) == 2
    with pytest.raises(RuntimeError, match="mcs_ens_compare: the settings of the accumulators' detectors samples differ"):
        e.compare(five, s, [ens.CompareRequest("gradient")])
    with pytest.raises(RuntimeError, match="mcs_ens_summarize_merged: the settings of the accumulators' detectors samples differ"):
        e.summarize_merged([five], s, [ens.Request("gradient")])
    assert e.count(s) == 3 and e.count(e.detectors_slot(0)) == n0
    assert same_words(before[0], e.mean(s, "spectrum")) and same_words(before[1], e.m2(s, "spectrum"))
    fresh.destroy(); five.destroy()
