"""The escape sample of the ensemble statistics on the device (mcs_ens_add_escape in csrc/mcs_ensemble.hip, through
ensemble.HipEnsemble) against plain numpy and Python floats: count, mean and M2 of crafted samples bit for bit, the slopes by the
products slot's rule, the refusals, the merge, a summary and a comparison of one door and frame, and a trigger that ends a run."""
import numpy as np
import pytest

import consumers_common as cc
import ens_compare_common as cmpc
import escape_common as ec
from conftest import mcs, make_problem, hip_backend
from ensemble_common import same_words, stat_of
from ens_summary_common import as_dict, assert_exact, assert_sums, restate

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
EPS = 2.0 ** -53
GAM_PF = (1.5, 1.03142)
NAMES = ("dNdp", "number", "slope")


def slopes_restated(hb, dndp, l_lo, l_hi, x_log):
    """The slope definition of include/mcs.h ("products sample") for every row of dndp [6][nmom+2] -> [6]: y from the device's own
    log10, the sums serial in Python floats."""
    rows = dndp.reshape(-1, dndp.shape[-1])
    valid = rows > 1.0e-99
    y = np.zeros_like(rows)
    y[valid] = hb.eval_fn("log10", rows[valid])
    out = np.full(len(rows), np.nan)
    for r in range(len(rows)):
        ls = [l for l in range(l_lo, l_hi) if valid[r, l]]
        k = len(ls)
        if k < 3:
            continue
        sx = sy = 0.0
        for l in ls:
            sx = sx + float(x_log[l])
            sy = sy + float(y[r, l])
        xbar, ybar = sx / k, sy / k
        sxx = sxy = 0.0
        for l in ls:
            dx = float(x_log[l]) - xbar
            sxx = sxx + dx * dx
            sxy = sxy + dx * (float(y[r, l]) - ybar)
        out[r] = sxy / sxx
    return out


def crafted_slabs(nm, nt, k):
    """Sample k: dense slabs; door 1 holds only two lit momentum columns (frames 1 and 2 spread them over a few
    bins, frame 0 has exactly two valid bins: no slope), door 0 is lit all over."""
    s = ec.dense_slabs(nm, nt, 100 + k, decades=30.0)
    keep = np.zeros(ec.PM, dtype=bool)
    keep[[nm // 2, nm // 2 + 1]] = True
    s[1][:, ~keep] = ec.FLOOR
    s[1][:nt + 1, keep] = np.abs(s[1][:nt + 1, keep]) + 1.0
    return s


def take(hb, e, t, slabs, slot):
    ec.write_slabs(hb, slabs)
    dndp, number, diag = hb.dndp_esc(t, GAM_PF)
    e.add_escape(hb, slot)
    return dndp, number


def parts_of(hb, dndp, number, window, x_log):
    return dict(dNdp=dndp.reshape(6, -1), number=number.ravel(), slope=slopes_restated(hb, dndp, *window, x_log))


@pytest.fixture(scope="module")
def fed():
    """One context on the small binning, three crafted pairs of slabs, and an accumulator that took an escape sample of each into
    the escape slot of species slot 1."""
    prob = cc.small_problem()
    nm, nt = prob.params.num_psd_mom_bins, prob.params.num_psd_tht_bins
    hb = hip_backend(prob)
    t = ec.escape_tables(prob, 1)
    x_log = ens.bin_centres_log10(prob)
    window = (0, nm + 1)
    e = ens.HipEnsemble(hb, 2)
    e.set_slope_window(*window, x_log)
    outs = [take(hb, e, t, crafted_slabs(nm, nt, k), 1) for k in range(3)]
    parts = [parts_of(hb, d, n, window, x_log) for d, n in outs]
    yield prob, hb, t, x_log, window, e, parts
    e.destroy(); hb.destroy()


def test_count_mean_and_m2(fed):
    prob, hb, t, x_log, window, e, parts = fed
    s = e.escape_slot(1)
    assert e.count(s) == 3 and e.count(e.escape_slot(0)) == 0 and e.count(1) == 0 and e.count(e.products_slot(1)) == 0
    assert e.layout.escape_total % 256 != 0            # (the tail of the grid-stride loop runs)
    want = stat_of(parts)
    for name in NAMES:
        assert same_words(e.mean(s, name), want.mean[name]), f"mean of {name}"
        assert same_words(e.m2(s, name), want.m2[name]), f"M2 of {name}"
    assert want.m2["dNdp"].max() > 0 and want.m2["number"].min() > 0
    with np.errstate(invalid="ignore"):
        assert same_words(e.stderr(s, "number"), np.sqrt(want.m2["number"] / 6.0))


def test_slopes_follow_the_products_rule(fed):
    prob, hb, t, x_log, window, e, parts = fed
    s = e.escape_slot(1)
    slope = e.mean(s, "slope")
    valid = (parts[0]["dNdp"][:, window[0]:window[1]] > 1.0e-99).sum(axis=1)
    print("valid bins per row:", valid.tolist(), "slopes of the first sample:", parts[0]["slope"].tolist())
    assert valid[3] == 2 and np.isnan(slope[3]) and np.all(valid[[0, 1, 2]] >= 3) and np.all(np.isfinite(slope[:3]))
    # a narrower window, one sample: the mean is the sample
    nm, nt = prob.params.num_psd_mom_bins, prob.params.num_psd_tht_bins
    narrow = (5, 17)
    f = ens.HipEnsemble(hb, 1)
    f.set_slope_window(*narrow, x_log)
    dndp, number = take(hb, f, t, crafted_slabs(nm, nt, 0), 0)
    want = slopes_restated(hb, dndp, *narrow, x_log)
    assert same_words(f.mean(f.escape_slot(0), "slope"), want) and np.isfinite(want).sum() >= 3
    assert same_words(f.mean(f.escape_slot(0), "dNdp"), dndp.reshape(6, -1)) and not np.any(f.m2(f.escape_slot(0), "number"))
    f.destroy()


def test_refusals(fed):
    prob, hb, t, x_log, window, e, parts = fed
    nm = prob.params.num_psd_mom_bins
    s = e.escape_slot(1)
    before = (e.mean(s, "dNdp"), e.m2(s, "dNdp"))
    fresh = ens.HipEnsemble(hb, 2)                 # (no window)
    hb.dndp_esc(t, GAM_PF)
    with pytest.raises(RuntimeError, match="no slope window"):
        fresh.add_escape(hb, 0)
    e.add_escape(hb, 0)                            # (the call's result is still there: the refusal took nothing)
    assert e.count(e.escape_slot(0)) == 1
    refused = [
        ("mcs_ens_add_escape", lambda: e.add_escape(hb, 0)),                              # a second sample from one call
        ("mcs_ens_add_escape", lambda: (hb.dndp_esc(t, GAM_PF), e.add_escape(hb, 2))),    # the iteration slot
        ("mcs_ens_add_escape", lambda: e.add_escape(hb, e.escape_slot(0))),               # out of range
        ("mcs_ens_set_slope_window", lambda: e.set_slope_window(0, 10, x_log)),           # after the first escape sample
        ("mcs_ens_read", lambda: fresh.mean(fresh.escape_slot(0), "number")),             # never sampled
        ("mcs_ens_read", lambda: e.stderr(e.escape_slot(0), "number")),                   # n = 1
        ("mcs_ens_load_mean", lambda: e.load_mean(s, hb)),
    ]
    for who, call in refused:
        with pytest.raises(RuntimeError, match=who):
            call()
    # no mcs_dndp_esc since mcs_begin_species
    hb.dndp_esc(t, GAM_PF)
    hb.begin_species(1, 1, 1.0, 1.0, prob.pmax, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="mcs_dndp_esc since its last mcs_begin_species"):
        e.add_escape(hb, 0)
    assert e.count(s) == 3 and e.count(e.escape_slot(0)) == 1 and fresh.count(fresh.escape_slot(0)) == 0
    assert same_words(before[0], e.mean(s, "dNdp")) and same_words(before[1], e.m2(s, "dNdp"))
    fresh.destroy()


def test_merge(fed):
    """Two accumulators with 2 + 1 samples merged: Chan's formula bit for bit, and the accumulator that took all three within the
    existing merge test's bound (16 n 2^-53 of |mean|, and of the sum of squares for M2)."""
    prob, hb, t, x_log, window, e, parts = fed
    nm, nt = prob.params.num_psd_mom_bins, prob.params.num_psd_tht_bins
    s = e.escape_slot(1)
    a, b, c = (ens.HipEnsemble(hb, 2) for _ in range(3))
    a.set_slope_window(*window, x_log); b.set_slope_window(*window, x_log)
    for k in range(3):
        take(hb, a if k < 2 else b, t, crafted_slabs(nm, nt, k), 1)
    with np.errstate(invalid="ignore"):
        want = stat_of(parts[:2]).merged_with(stat_of(parts[2:]))
    a.merge(b)
    c.merge(a)                                     # an accumulator without a window takes the one the samples were made with
    assert a.count(s) == 3 and b.count(s) == 1 and c.count(s) == 3 and c.window[:2] == window
    for acc in (a, c):
        for name in NAMES:
            assert same_words(acc.mean(s, name), want.mean[name]) and same_words(acc.m2(s, name), want.m2[name]), name
    n = 3
    for name in ("dNdp", "number"):
        mean, m2 = a.mean(s, name), a.m2(s, name)
        sum_x2 = sum(p[name] * p[name] for p in parts)
        assert np.all(np.abs(mean - e.mean(s, name)) <= 16 * n * EPS * np.abs(e.mean(s, name))), name
        assert np.all(np.abs(m2 - e.m2(s, name)) <= 16 * n * EPS * sum_x2), name
    other = ens.HipEnsemble(hb, 2)
    other.set_slope_window(1, nm + 1, x_log)
    take(hb, other, t, crafted_slabs(nm, nt, 0), 1)
    with pytest.raises(RuntimeError, match="slope windows differ"):
        a.merge(other)
    for acc in (a, b, c, other):
        acc.destroy()


def test_summary_and_comparison_of_one_door_and_frame(fed):
    prob, hb, t, x_log, window, e, parts = fed
    nm, nt = prob.params.num_psd_mom_bins, prob.params.num_psd_tht_bins
    NM = nm + 2
    s = e.escape_slot(1)
    total = e.layout.escape_total
    mean, m2 = e._read(s, 0, 0, total), e._read(s, 1, 0, total)
    reqs = [ens.Request("dNdp", e.escape_row(0, 2), 0.0, 0.3), ens.Request("dNdp", e.escape_row(1, 1), 0.0, 0.1, (3, nm)),
            ens.Request("number", e.escape_row(0, 2), 0.0, 0.5), ens.Request("number"), ens.Request("slope", e.escape_row(0, 0), 0.0, 0.1),
            ens.Request("slope")]
    got = e.summarize(s, reqs)
    for q, r in zip(reqs, got):
        first, count = e.word_range(s, q.name, q.zones, q.bins)
        want = restate(mean[first:first + count], m2[first:first + count], 3, q.floor_frac, q.tol)
        assert r.n == 3
        assert_exact(as_dict(r), want, repr(q))
        assert_sums(as_dict(r), want, repr(q))
    assert got[0].n_selected > 3 and got[2].n_selected == 1 and got[5].n_nonfinite == 1
    first, count = e.word_range(s, "dNdp", e.escape_row(0, 2))
    assert (first, count) == (2 * NM, NM)
    # another accumulator with other samples: per-word z-scores of one door and frame
    b = ens.HipEnsemble(hb, 2)
    b.set_slope_window(*window, x_log)
    for k in (5, 6):
        take(hb, b, t, crafted_slabs(nm, nt, k), 1)
    mb, qb = b._read(s, 0, 0, total), b._read(s, 1, 0, total)
    creqs = [ens.CompareRequest("dNdp", e.escape_row(0, 2), 0.0, 2.0), ens.CompareRequest("number", e.escape_row(1, 0), 0.0, 1.0)]
    diffs = e.compare(b, s, creqs)
    for q, d in zip(creqs, diffs):
        first, count = e.word_range(s, q.name, q.zones, q.bins)
        sl = slice(first, first + count)
        want = cmpc.restate(mean[sl], m2[sl], 3, mb[sl], qb[sl], 2, q.floor_frac, q.zcut)
        assert d.n_a == 3 and d.n_b == 2
        cmpc.assert_exact(cmpc.as_dict(d), want, repr(q))
        cmpc.assert_sums(cmpc.as_dict(d), want, repr(q))
    assert diffs[0].n_selected > 3
    with pytest.raises(ValueError, match="escape slot with a products slot"):
        e.compare(b, s, creqs, other_slot=b.products_slot(1))
    b.destroy()


def test_a_trigger_on_the_number_ends_a_run():
    """driver.run(finalize=True, escape=True, ensemble=..., triggers=...): a stop rule on the number of the upstream door in the ISM
    frame, loose enough to be met at the first check."""
    prob = make_problem(200, num_iterations=5)
    hb = hip_backend(prob)
    e = ens.Ensemble.for_backend(hb, 1)
    s = e.escape_slot(0)
    trig = ens.Trigger(s, "number", "max", 10.0, zones=e.escape_row(0, 2), floor_frac=0.0)
    try:
        with pytest.raises(ValueError, match="escape slot needs escape=True"):
            mcs.driver.run(prob, hb, n_itrs=3, finalize=True, ensemble=e, triggers=[trig])
        res = mcs.driver.run(prob, hb, n_itrs=5, finalize=True, escape=True, ensemble=e, triggers=[trig], min_iterations=2)
        c = res.convergence
        assert c.satisfied and c.stopped_at == 2 and e.count(s) == 2 and len(res.escape) == 2
        (row,) = c.checks[0][1]
        numbers = [spec.number[0, 2] for _, _, spec in res.escape]
        want = stat_of([dict(n=np.array([v])) for v in numbers])
        assert row.met and row.summary.n == 2 and row.summary.n_selected == 1 and numbers[0] > 0 and numbers[0] != numbers[1]
        assert cmpc.same_bits(row.summary.amax, abs(float(want.mean["n"][0])))
        assert cmpc.same_bits(row.value, float(np.sqrt(want.m2["n"][0] / 2.0) / abs(want.mean["n"][0])))
    finally:
        e.destroy(); hb.destroy()
