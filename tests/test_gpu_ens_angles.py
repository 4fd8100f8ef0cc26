"""The angles sample of the ensemble statistics on the device (mcs_ens_add_angles in csrc/mcs_ensemble.hip, through
ensemble.HipEnsemble) against the numpy ensemble fed the same AngleDistributions, word for word; the refusals, the merge and the
merged summary over two accumulators, a comparison of two species' angles slots, and triggers on <mu> of one row: one that is met,
and one on a row that no particle reached, which never is."""
import numpy as np
import pytest

import angles_common as ac
import consumers_common as cc
import ens_compare_common as cmpc
from conftest import mcs, make_problem, hip_backend
from ensemble_common import same_words, stat_of
from ens_summary_common import as_dict, assert_exact, assert_sums, restate

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
NAMES = ("dist", "number", "mean_mu", "mean_mu2")
LIT, DARK = 6, 4             # zones (0-based) of cc.dense_tallies: zone 5 (1-based) stays dark


def windows_of(nm):
    return ((0, nm + 1), (4, 9), (nm - 2, nm + 1))


def take(prob, hb, e, k, slot, windows=None):
    """Dense tallies number k written, the distributions made, one angles sample of them -> the AngleDistributions."""
    f, i = cc.dense_tallies(prob, seed=200 + k, decades=30.0)
    hb.write_tallies(f, i)
    d = mcs.consumers.angle_distributions(prob, hb, 1, windows or windows_of(prob.params.num_psd_mom_bins))
    e.add_angles(hb, slot, d)
    return d


def lo_hi(windows):
    return [w[0] for w in windows], [w[1] for w in windows]


def all_words(e, slot):
    n = e._len(slot)
    return e._read(slot, 0, 0, n), e._read(slot, 1, 0, n)


@pytest.fixture(scope="module")
def fed():
    """One context on the small binning with dense_gammas as its profile, a device accumulator that took three angles samples into
    the angles slot of species slot 1, and the numpy accumulator fed the same AngleDistributions."""
    prob = cc.small_problem()
    nm = prob.params.num_psd_mom_bins
    cc.set_gammas(prob, cc.dense_gammas(prob.params.n_grid))
    hb = hip_backend(prob)
    hb.begin_iteration(1)
    e, h = ens.HipEnsemble(hb, 2), ens.HostEnsemble(prob.params, 2)
    for acc in (e, h):
        acc.set_angle_windows(*lo_hi(windows_of(nm)))
    ds = [take(prob, hb, e, k, 1) for k in range(3)]
    with np.errstate(invalid="ignore"):
        for d in ds:
            h.add_angles(None, 1, d)
    yield prob, hb, e, h, ds
    e.destroy(); hb.destroy()


def test_device_samples_equal_the_host_ensemble(fed):
    prob, hb, e, h, ds = fed
    s = e.angles_slot(1)
    assert e.count(s) == 3 == h.count(s) and e.count(e.angles_slot(0)) == 0 and e.count(1) == 0 and e.count(e.escape_slot(1)) == 0
    assert e._len(s) == h._len(s) and e._len(s) % 256 != 0          # (the tail of the grid-stride loop runs)
    for got, want in zip(all_words(e, s), all_words(h, s)):
        assert same_words(got, want)
    rows = 3 * prob.params.n_grid * 3
    with np.errstate(invalid="ignore"):
        want = stat_of([dict(dist=d.dist.reshape(rows, -1), number=d.number.ravel(), mean_mu=d.mean_mu.ravel(), mean_mu2=d.mean_mu2.ravel()) for d in ds])
    for name in NAMES:
        assert same_words(e.mean(s, name), want.mean[name]) and same_words(e.m2(s, name), want.m2[name]), name
    lit, dark = e.angles_row(1, LIT, 0)[0], e.angles_row(1, DARK, 0)[0]
    assert want.m2["number"][lit] > 0 and np.isfinite(want.mean["mean_mu"][lit]) and np.isnan(want.mean["mean_mu"][dark]) and want.mean["number"][dark] == 0
    with np.errstate(invalid="ignore"):
        assert same_words(e.stderr(s, "number"), np.sqrt(want.m2["number"] / 6.0))
    # each sample is what the restatement gives on the tallies it was made from
    f, i = cc.dense_tallies(prob, seed=202, decades=30.0)
    t = mcs.consumers.consumer_tables(prob, 1)
    ac.assert_equal_to_reference(ds[2], ac.reference(prob, t, f, i, ds[2].windows), "sample 2")


def test_refusals(fed):
    prob, hb, e, h, ds = fed
    nm = prob.params.num_psd_mom_bins
    win = windows_of(nm)
    s = e.angles_slot(1)
    before = all_words(e, s)
    fresh = ens.HipEnsemble(hb, 2)                 # (no windows)
    mcs.consumers.angle_distributions(prob, hb, 1, win)
    with pytest.raises(RuntimeError, match="no angle windows"):
        fresh.add_angles(hb, 0)
    other = ens.HipEnsemble(hb, 2)
    other.set_angle_windows([0, 4, nm - 2], [nm + 1, 10, nm + 1])
    with pytest.raises(RuntimeError, match="windows of the context's mcs_angle_dist differ"):
        other.add_angles(hb, 0)
    e.add_angles(hb, 0)                            # (the call's result is still there: the refusals took nothing)
    assert e.count(e.angles_slot(0)) == 1
    again = lambda: mcs.consumers.angle_distributions(prob, hb, 1, win)
    refused = [
        ("mcs_ens_add_angles", lambda: e.add_angles(hb, 0)),                              # a second sample from one call
        ("mcs_ens_add_angles", lambda: (again(), e.add_angles(hb, 2))),                   # the iteration slot
        ("mcs_ens_add_angles", lambda: e.add_angles(hb, e.angles_slot(0))),               # out of range
        ("mcs_ens_set_angle_windows", lambda: e.set_angle_windows(*lo_hi(win))),          # after the first angles sample
        ("mcs_ens_set_angle_windows", lambda: fresh._set_angle_windows([3], [3])),        # an empty window
        ("mcs_ens_set_angle_windows", lambda: fresh._set_angle_windows([0] * 9, [1] * 9)),
        ("mcs_ens_read", lambda: fresh._read(fresh.angles_slot(0), 0, 0, 1)),             # never sampled
        ("mcs_ens_read", lambda: e.stderr(e.angles_slot(0), "number")),                   # n = 1
        ("mcs_ens_load_mean", lambda: e.load_mean(s, hb)),
    ]
    for who, call in refused:
        with pytest.raises(RuntimeError, match=who):
            call()
    # no mcs_angle_dist since mcs_begin_species, and none since a write of the tallies
    again()
    hb.begin_species(1, 1, 1.0, 1.0, prob.pmax, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="mcs_angle_dist since its last mcs_begin_species"):
        e.add_angles(hb, 0)
    f, i = cc.dense_tallies(prob, seed=200, decades=30.0)
    hb.write_tallies(f, i)
    again()
    hb.write_tally("psd", mcs.capi.Layout(prob.params).view(f, "psd"))
    with pytest.raises(RuntimeError, match="mcs_angle_dist since its last mcs_begin_species"):
        e.add_angles(hb, 0)
    assert e.count(s) == 3 and e.count(e.angles_slot(0)) == 1 and fresh.count(fresh.angles_slot(0)) == 0
    assert all(same_words(a, b) for a, b in zip(before, all_words(e, s)))
    fresh.set_angle_windows([0], [5]); fresh.set_angle_windows(*lo_hi(win))              # (may be repeated before the first sample)
    fresh.destroy(); other.destroy()


def test_merge_and_merged_summary(fed):
    """Two accumulators with 2 + 1 samples: Chan's formula bit for bit against the numpy ensembles merged the same way, the merged
    summary of the two equal to the summary of their merge, and the window rules."""
    prob, hb, e, h, ds = fed
    nm = prob.params.num_psd_mom_bins
    win = windows_of(nm)
    s = e.angles_slot(1)
    a, b, c = (ens.HipEnsemble(hb, 2) for _ in range(3))
    ha, hb_ = ens.HostEnsemble(prob.params, 2), ens.HostEnsemble(prob.params, 2)
    for acc in (a, b, ha, hb_):
        acc.set_angle_windows(*lo_hi(win))
    with np.errstate(invalid="ignore"):
        for k in range(3):
            d = take(prob, hb, a if k < 2 else b, k, 1)
            (ha if k < 2 else hb_).add_angles(None, 1, d)
        reqs = [ens.Request("dist", e.angles_row(1, LIT, 0), 0.0, 0.3), ens.Request("number", None, 0.0, 0.2),
                ens.Request("mean_mu", e.angles_row(2, LIT, 0), 0.0, 0.1), ens.Request("mean_mu2", e.angles_row(0, DARK, 0), 0.0)]
        merged = a.summarize_merged([b], s, reqs)
        a.merge(b)
        c.merge(a)                                 # an accumulator without windows takes the ones the samples were made with
        ha.merge(hb_)
        assert a.count(s) == 3 and b.count(s) == 1 and c.count(s) == 3 and c.angle_windows == a.angle_windows == lo_hi_t(win)
        for acc in (a, c):
            for got, want in zip(all_words(acc, s), all_words(ha, s)):
                assert same_words(got, want)
        mean, m2 = all_words(a, s)
        for q, r, r2 in zip(reqs, merged, a.summarize(s, reqs)):
            first, count = a.word_range(s, q.name, q.zones, q.bins)
            want = restate(mean[first:first + count], m2[first:first + count], 3, q.floor_frac, q.tol)
            assert r.n == 3 and r == r2
            assert_exact(as_dict(r), want, repr(q))
            assert_sums(as_dict(r), want, repr(q))
    assert merged[0].n_selected > 3 and merged[2].n_selected == 1 and merged[2].n_nonfinite == 0 and merged[3].n_nonfinite == 1
    with pytest.raises(RuntimeError, match="the windows stay"):
        c.set_angle_windows(*lo_hi(win))
    other = ens.HipEnsemble(hb, 2)
    other.set_angle_windows([0, 4, nm - 2], [nm + 1, 10, nm + 1])
    for k in (0, 1):
        take(prob, hb, other, k, 1, ((0, nm + 1), (4, 10), (nm - 2, nm + 1)))
    with pytest.raises(RuntimeError, match="angle windows differ"):
        a.merge(other)
    with pytest.raises(RuntimeError, match="angle windows differ"):
        a.summarize_merged([other], s, reqs)
    with pytest.raises(RuntimeError, match="angle windows differ"):
        a.compare(other, s, [ens.CompareRequest("number", None, 0.0)])
    for acc in (a, b, c, other):
        acc.destroy()


def lo_hi_t(windows):
    return tuple(w[0] for w in windows), tuple(w[1] for w in windows)


def test_compare_two_species_slots(fed):
    prob, hb, e, h, ds = fed
    s1 = e.angles_slot(1)
    b = ens.HipEnsemble(hb, 2)
    b.set_angle_windows(*lo_hi(windows_of(prob.params.num_psd_mom_bins)))
    for k in (5, 6):
        take(prob, hb, b, k, 0)
    s0 = b.angles_slot(0)
    (ma, qa), (mb, qb) = all_words(e, s1), all_words(b, s0)
    creqs = [ens.CompareRequest("dist", e.angles_row(2, LIT, 0), 0.0, 2.0), ens.CompareRequest("mean_mu", None, 0.0, 1.0),
             ens.CompareRequest("number", e.angles_row(0, LIT, 1), 0.0, 1.0)]
    diffs = e.compare(b, s1, creqs, other_slot=s0)
    for q, d in zip(creqs, diffs):
        first, count = e.word_range(s1, q.name, q.zones, q.bins)
        sl = slice(first, first + count)
        with np.errstate(invalid="ignore"):
            want = cmpc.restate(ma[sl], qa[sl], 3, mb[sl], qb[sl], 2, q.floor_frac, q.zcut)
        assert d.n_a == 3 and d.n_b == 2
        cmpc.assert_exact(cmpc.as_dict(d), want, repr(q))
        cmpc.assert_sums(cmpc.as_dict(d), want, repr(q))
    assert diffs[0].n_selected > 3 and diffs[1].n_nonfinite > 0 and diffs[2].n_selected == 1
    with pytest.raises(ValueError, match="angles slot with a"):
        e.compare(b, s1, creqs, other_slot=b.escape_slot(0))
    with pytest.raises(ValueError, match="at least two samples"):
        e.compare(b, s1, creqs, other_slot=b.angles_slot(1))
    b.destroy()


def test_triggers_on_the_mean_cosine_in_a_run():
    """driver.run(finalize=True, angles=[...], ensemble=..., triggers=...): a stop rule on <mu> of the downstream end in the plasma
    frame, loose enough to be met at the first check -- and one on a window far above every momentum a 200-particle run reaches, whose
    <mu> is NaN in every sample: never met, so the run goes on to its last iteration."""
    prob = make_problem(200, num_iterations=5)
    P = prob.params
    nm = P.num_psd_mom_bins
    x = 10.0 ** ens.bin_centres_log10(prob)
    angles = [(x[0] * 0.5, x[-1] * 2.0), (x[nm] * 0.999, x[nm] * 1.001)]
    hb = hip_backend(prob)
    e = ens.Ensemble.for_backend(hb, 1)
    e.set_angle_windows([0, nm], [nm + 1, nm + 1])
    s = e.angles_slot(0)
    z = P.n_grid - 1
    met = ens.Trigger(s, "mean_mu", "max", 1.0e3, zones=e.angles_row(1, z, 0), floor_frac=0.0)
    never = ens.Trigger(s, "mean_mu", "max", 1.0e3, zones=e.angles_row(1, z, 1), floor_frac=0.0)
    try:
        with pytest.raises(ValueError, match="angles slot needs angles="):
            mcs.driver.run(prob, hb, n_itrs=3, finalize=True, ensemble=e, triggers=[met])
        res = mcs.driver.run(prob, hb, n_itrs=5, finalize=True, angles=angles, ensemble=e, triggers=[met], min_iterations=2)
        c = res.convergence
        assert c.satisfied and c.stopped_at == 2 and e.count(s) == 2 and len(res.angles) == 2
        (row,) = c.checks[0][1]
        mus = [d.mean_mu[1, z, 0] for _, _, d in res.angles]
        want = stat_of([dict(n=np.array([v])) for v in mus])
        assert row.met and row.summary.n == 2 and row.summary.n_selected == 1 and np.isfinite(mus[0]) and mus[0] != mus[1]
        assert cmpc.same_bits(row.summary.amax, abs(float(want.mean["n"][0])))
        assert cmpc.same_bits(row.value, float(np.sqrt(want.m2["n"][0] / 2.0) / abs(want.mean["n"][0])))
        assert all(np.isnan(d.mean_mu[1, z, 1]) and d.number[1, z, 1] == 0 for _, _, d in res.angles)
        res = mcs.driver.run(prob, hb, n_itrs=2, first_iter=3, finalize=True, angles=angles, ensemble=e, triggers=[never], min_iterations=2,
                             iter_state=res.iter_state)
        c = res.convergence
        assert not c.satisfied and c.checks and e.count(s) == 4 and all(not r.met and r.summary.n_nonfinite == 1 for _, rows in c.checks for r in rows)
    finally:
        e.destroy(); hb.destroy()
