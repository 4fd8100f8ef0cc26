"""The products sample of the ensemble statistics on the device (csrc/mcs_ensemble.hip: mcs_k_ens_slope, mcs_k_ens_add_products,
through ensemble.HipEnsemble) against plain numpy and Python floats: the update and the slope bit for bit, the refusals, the
summaries of a products slot, the lazy allocation, and the driver's samples."""
import ctypes as ct

import numpy as np
import pytest

from conftest import mcs, make_problem, hip_backend
from ensemble_common import bits_equal, crafted_buffers, same_words, species_parts, stat_of
from ens_summary_common import as_dict, assert_exact, assert_sums, restate, same_bits

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
THREADS, MAX_BLOCKS = 256, 2048          # ENS_THREADS, ENS_MAX_BLOCKS of csrc/mcs_ensemble.hip
DNDP = ("dNdp_sf", "dNdp_pf", "dNdp_isf")
SCALARS = ("P_psd_par", "P_psd_perp", "energy_density_psd")
SLOPES = ("slope_sf", "slope_pf", "slope_isf")
NAMES = DNDP + SCALARS + SLOPES


def slopes_restated(hb, dndp, l_lo, l_hi, x_log):
    """The slope definition of include/mcs.h for every row of dndp [3][n_grid][nmom+2] -> [3][n_grid]: y from the device's own
    log10 (mcs_eval_fn), the sums serial in Python floats."""
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
    return out.reshape(dndp.shape[:-1])


def consume(hb, tabs):
    """dndp_cr + thermo_calcs on the context's tallies -> the device's own bits on the host."""
    dndp, _ = hb.dndp_cr(tabs)
    return (dndp,) + tuple(hb.thermo_calcs(tabs))


def parts_of(out, slopes):
    dndp, ppar, pperp, edens = out
    p = {name: dndp[m] for m, name in enumerate(DNDP)}
    p.update(P_psd_par=ppar, P_psd_perp=pperp, energy_density_psd=edens)
    p.update({name: slopes[m] for m, name in enumerate(SLOPES)})
    return p


def shaped_buffers(L, seed):
    """Tallies whose shock-frame dN/dp has, inside the momentum bins 60..100: nothing above the floor in zone 0, exactly three
    bins in zone 1, every other bin in zone 2, and a third of all cells, at random, from zone 3 on."""
    rng = np.random.default_rng(seed)
    f, i = np.zeros(L.total), np.zeros(L.n_i64, dtype=np.int64)
    psd = L.view(f, "psd")
    psd[...] = 1e-99
    ng, nt, nm = psd.shape
    vals = lambda n: rng.uniform(1, 10, n) * 10.0 ** rng.integers(-8, 3, n)
    for l in (62, 75, 90):
        psd[1, rng.integers(1, nt - 1), l] = vals(1)[0]
    for l in range(60, 100, 2):
        psd[2, rng.integers(1, nt - 1), l] = vals(1)[0]
    n = (nt - 2) * (nm - 2)
    for z in range(3, ng):
        psd[z, 1:nt - 1, 1:nm - 1] = (vals(n) * (rng.random(n) < 0.3)).reshape(nt - 2, nm - 2) + 1e-99
    L.view(f, "therm_pf")[...] = rng.uniform(0, 5, L.view(f, "therm_pf").shape)
    i[:ng] = rng.integers(0, 1000, ng)
    return f, i


def slot_words(e, slot):
    return e._read(slot, 0, 0, e.layout.products_total), e._read(slot, 1, 0, e.layout.products_total)


@pytest.fixture(scope="module")
def fed():
    """One context, five crafted tally buffers, the consumers' results of each as the device returned them, and an accumulator with
    the window [0, nmom + 1) that took a products sample of each into slot 1."""
    prob = make_problem(64)
    L = mcs.capi.Layout(prob.params)
    total = ens.EnsLayout(prob.params).products_total
    ng, NM = prob.params.n_grid, prob.params.num_psd_mom_bins + 2
    # the tail of the grid-stride loop runs, in one stride (the products vector is never longer than one)
    assert total == 3 * ng * NM + 6 * ng and total % THREADS != 0 and total < MAX_BLOCKS * THREADS
    hb = hip_backend(prob)
    tabs = mcs.consumers.consumer_tables(prob, 1)
    x_log = ens.bin_centres_log10(prob)
    window = (0, NM - 1)
    e = ens.HipEnsemble(hb, 2)
    e.set_slope_window(*window, x_log)
    outs = []
    for f, i in crafted_buffers(L):
        hb.write_tallies(f, i)
        outs.append(consume(hb, tabs))
        e.add_products(hb, 1)
    parts = [parts_of(o, slopes_restated(hb, o[0], *window, x_log)) for o in outs]
    yield prob, L, hb, tabs, x_log, e, outs, parts
    e.destroy(); hb.destroy()


def test_update_is_bit_exact(fed):
    prob, L, hb, tabs, x_log, e, outs, parts = fed
    ps = e.products_slot(1)
    assert e.count(ps) == 5 and e.count(e.products_slot(0)) == 0 and e.count(0) == 0 and e.count(1) == 0 and e.count(2) == 0
    want = stat_of(parts)
    finite = np.mean([np.isfinite(want.mean[name]).mean() for name in DNDP + SCALARS])
    print(f"finite words of the first six parts: {finite:.3f}")
    assert finite > 0.9
    for name in NAMES:
        assert same_words(e.mean(ps, name), want.mean[name]), f"mean of {name}"
        assert same_words(e.m2(ps, name), want.m2[name]), f"M2 of {name}"
    for name in DNDP + SCALARS:
        with np.errstate(invalid="ignore"):
            assert same_words(e.stderr(ps, name), np.sqrt(want.m2[name] / 20.0)), name
    assert np.isfinite(want.mean["slope_sf"]).mean() > 0.5 and want.m2["slope_sf"][np.isfinite(want.m2["slope_sf"])].max() > 0
    # the samples left the context's tallies as they were
    f, i = hb.read_tallies()
    f_last, i_last = crafted_buffers(L)[-1]
    assert bits_equal(f, f_last) and np.array_equal(i, i_last)


def test_slope_is_bit_exact(fed):
    prob, L, hb, tabs, x_log, e_fed, outs, parts = fed
    NM = prob.params.num_psd_mom_bins + 2
    hb.write_tallies(*shaped_buffers(L, 3))
    seen = dict(floor=0, three=0, gaps=0)
    for window in ((0, NM - 1), (60, 100), (61, 64), (70, 73)):
        e = ens.HipEnsemble(hb, 1)
        e.set_slope_window(*window, x_log)
        out = consume(hb, tabs)
        e.add_products(hb, 0)
        ps = e.products_slot(0)
        want = slopes_restated(hb, out[0], *window, x_log)
        got = np.array([e.mean(ps, name) for name in SLOPES])
        assert same_words(got, want), window
        assert same_words(e.mean(ps, "dNdp_pf"), out[0][1]) and not np.any(e.m2(ps, "dNdp_sf"))      # (one sample: the mean is the sample)
        k = (out[0][:, :, window[0]:window[1]] > 1e-99).sum(axis=2)
        width = window[1] - window[0]
        seen["floor"] += int(np.sum(k == 0)); seen["three"] += int(np.sum(k == 3)); seen["gaps"] += int(np.sum((k > 3) & (k < width)))
        assert np.all(np.isnan(got[k < 3])) and np.all(np.isfinite(got[k >= 3]))
        e.destroy()
    print("rows by case:", seen)
    # every case was met: a window entirely on the floor, exactly three valid bins, gaps between the valid bins; the window
    # [0, nmom + 1) is the first of the list (and that of `fed`, five samples deep)
    assert seen["floor"] > 0 and seen["three"] > 0 and seen["gaps"] > 0


def test_refusals_change_nothing(fed):
    prob, L, hb, tabs, x_log, e, outs, parts = fed
    ps = e.products_slot(1)
    before = slot_words(e, ps)
    fresh = ens.HipEnsemble(hb, 2)            # (no window)
    consume(hb, tabs)
    with pytest.raises(RuntimeError, match="no slope window"):
        fresh.add_products(hb, 0)
    e.add_products(hb, 0)                      # (the consumers' results are still there: the refusal took nothing)
    assert e.count(e.products_slot(0)) == 1
    refused = [
        ("mcs_ens_add_products", lambda: e.add_products(hb, 0)),                      # a second sample without fresh consumer calls
        ("mcs_ens_add_products", lambda: (hb.dndp_cr(tabs), e.add_products(hb, 0))),   # one consumer alone
        ("mcs_ens_add_products", lambda: e.add_products(hb, 2)),                      # the iteration slot
        ("mcs_ens_add_products", lambda: e.add_products(hb, e.products_slot(0))),     # out of range
        ("mcs_ens_set_slope_window", lambda: e.set_slope_window(0, 10, x_log)),       # after the first sample
        ("mcs_ens_set_slope_window", lambda: fresh._set_slope_window(5, 7, x_log)),                  # (past the wrapper's own check)
        ("mcs_ens_set_slope_window", lambda: fresh._set_slope_window(0, len(x_log) + 1, x_log)),
        ("mcs_ens_set_slope_window", lambda: fresh._set_slope_window(-1, 5, x_log)),
        ("mcs_ens_read", lambda: fresh.mean(fresh.products_slot(0), "dNdp_pf")),       # never sampled
        ("mcs_ens_read", lambda: e.stderr(e.products_slot(0), "dNdp_pf")),             # n = 1
        ("mcs_ens_count", lambda: e._chk(e.lib.mcs_ens_count(e.h, (1 << 30) | 2, ct.byref(ct.c_int64(0))))),       # no species slot 2
        ("mcs_ens_load_mean", lambda: e.load_mean(ps, hb)),
    ]
    for who, call in refused:
        with pytest.raises(RuntimeError, match=who):
            call()
    # after mcs_begin_species the results of the earlier consumer calls no longer count
    consume(hb, tabs)
    hb.begin_species(1, 1, 1.0, 1.0, prob.pmax, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="mcs_ens_add_products"):
        e.add_products(hb, 0)
    assert e.count(ps) == 5 and e.count(e.products_slot(0)) == 1 and fresh.count(fresh.products_slot(0)) == 0
    after = slot_words(e, ps)
    assert same_words(before[0], after[0]) and same_words(before[1], after[1])
    fresh.destroy()


def test_summaries_of_a_products_slot(fed):
    prob, L, hb, tabs, x_log, e, outs, parts = fed
    ps = e.products_slot(1)
    ng, NM = prob.params.n_grid, prob.params.num_psd_mom_bins + 2
    mean, m2 = slot_words(e, ps)
    reqs = [ens.Request("dNdp_pf"), ens.Request("dNdp_sf", (3, 40), 1e-6, 0.3), ens.Request("P_psd_par", None, 0.0, 0.5),
            ens.Request("energy_density_psd", (10, 11)), ens.Request("slope_sf", None, 0.0, 0.1), ens.Request("slope_isf", (5, 50), 0.5),
            ens.Request("dNdp_isf", (ng - 1, ng), 1e-3, 0.2, (60, 111)), ens.Request("dNdp_pf", (0, 1), 0.0, 0.0, (1, 2)),
            ens.Request("dNdp_sf", (7, 8), 1e-9, 1.0, (0, NM))]
    got = e.summarize(ps, reqs)
    for q, s in zip(reqs, got):
        first, count = e.word_range(ps, q.name, q.zones, q.bins)
        want = restate(mean[first:first + count], m2[first:first + count], 5, q.floor_frac, q.tol)
        assert s.n == 5
        assert_exact(as_dict(s), want, repr(q))
        assert_sums(as_dict(s), want, repr(q))
    assert sum(s.n_selected for s in got) > 1000
    # merged over three accumulators with 2 + 0 + 3 samples: what merging them into an empty one and summarising it gives
    accs = [ens.HipEnsemble(hb, 2) for _ in range(4)]
    for a in accs[:3]:
        a.set_slope_window(0, NM - 1, x_log)
    mine = []                 # (the consumers add with atomics: a second run over the same tallies need not repeat the first's bits)
    for k, (f, i) in enumerate(crafted_buffers(L)):
        hb.write_tallies(f, i)
        out = consume(hb, tabs)
        mine.append({name: out[0][m] for m, name in enumerate(DNDP)} | dict(zip(SCALARS, out[1:])))
        accs[0 if k < 2 else 2].add_products(hb, 1)
    merged = accs[0].summarize_merged(accs[1:3], ps, reqs)
    for a in accs[:3]:
        accs[3].merge(a)
    assert [a.count(ps) for a in accs] == [2, 0, 3, 5]
    direct = accs[3].summarize(ps, reqs)
    for q, a, b in zip(reqs, merged, direct):
        da, db = as_dict(a), as_dict(b)
        assert a.n == b.n == 5
        for key in da:
            assert same_bits(da[key], db[key]) if isinstance(db[key], float) else da[key] == db[key], (q, key, da[key], db[key])
    # the merge itself is Chan's, words of the first six parts
    wa, wb = stat_of(mine[:2]), stat_of(mine[2:])
    with np.errstate(invalid="ignore", over="ignore"):
        want = wa.merged_with(wb)
    for name in DNDP + SCALARS:
        assert same_words(accs[3].mean(ps, name), want.mean[name]) and same_words(accs[3].m2(ps, name), want.m2[name]), name
    # accumulators whose windows differ are refused, in a merge and in a merged summary
    other = ens.HipEnsemble(hb, 2)
    other.set_slope_window(1, NM - 1, x_log)
    consume(hb, tabs)
    other.add_products(hb, 1)
    with pytest.raises(RuntimeError, match="slope windows differ"):
        accs[0].merge(other)
    with pytest.raises(RuntimeError, match="slope windows differ"):
        accs[0].summarize_merged([other], ps, reqs)
    assert accs[0].count(ps) == 2
    for a in accs + [other]:
        a.destroy()


def test_an_accumulator_without_products_is_what_it_was(fed):
    prob, L, hb, tabs, x_log, e_fed, outs, parts = fed
    bufs = crafted_buffers(L, 3)
    plain, both = ens.HipEnsemble(hb, 1), ens.HipEnsemble(hb, 1)
    both.set_slope_window(10, 50, x_log)
    for f, i in bufs:
        hb.write_tallies(f, i)
        plain.add_species(hb, 0)
        both.add_species(hb, 0)
        consume(hb, tabs)
        both.add_products(hb, 0)
    sp = [species_parts(L, f, i) for f, i in bufs]
    want = stat_of(sp)
    ps = plain.products_slot(0)
    assert plain.count(ps) == 0 and both.count(ps) == 3 and plain.count(0) == both.count(0) == 3
    into_plain, into_both = ens.HipEnsemble(hb, 1), ens.HipEnsemble(hb, 1)
    into_plain.merge(plain)
    into_both.merge(both)
    assert into_plain.count(ps) == 0 and into_both.count(ps) == 3
    for name in sp[0]:
        for acc in (plain, both, into_plain, into_both):
            assert bits_equal(acc.mean(0, name), want.mean[name]) and bits_equal(acc.m2(0, name), want.m2[name]), name
    with pytest.raises(RuntimeError, match="mcs_ens_read"):
        plain.mean(ps, "dNdp_sf")
    with pytest.raises(RuntimeError, match="mcs_ens_read"):
        into_plain.mean(ps, "dNdp_sf")
    assert same_words(into_both.mean(ps, "dNdp_sf"), both.mean(ps, "dNdp_sf")) and same_words(into_both.m2(ps, "slope_sf"), both.m2(ps, "slope_sf"))
    for acc in (plain, both, into_plain, into_both):
        acc.destroy()


N_PCUTS = 6


def fin_parts(fin):
    p = {name: np.asarray(fin.dNdp_cr[m], dtype=np.float64) for m, name in enumerate(DNDP)}
    p.update({name: np.asarray(getattr(fin, name), dtype=np.float64) for name in SCALARS})
    return p


def test_driver_feeds_the_products_slot():
    prob = make_problem(2000, num_iterations=6)
    NM = prob.params.num_psd_mom_bins + 2
    hb = hip_backend(prob)
    e = ens.Ensemble.for_backend(hb, 1)
    ps = e.products_slot(0)
    res = mcs.driver.run(prob, hb, n_itrs=3, max_pcuts=N_PCUTS, finalize=True, ensemble=e)
    assert e.count(ps) == 3 and e.count(0) == 3 and e.window[:2] == (0, NM - 1)
    want = stat_of([fin_parts(fin) for _, _, fin in res.iter_finals])
    assert want.m2["dNdp_sf"].max() > 0 and want.m2["P_psd_par"].max() > 0
    for name in DNDP + SCALARS:
        assert same_words(e.mean(ps, name), want.mean[name]) and same_words(e.m2(ps, name), want.m2[name]), name
    slopes = stat_of([{"s": slopes_restated(hb, np.asarray(fin.dNdp_cr), 0, NM - 1, e.window[2])} for _, _, fin in res.iter_finals])
    assert same_words(np.array([e.mean(ps, name) for name in SLOPES]), slopes.mean["s"])
    with pytest.raises(ValueError, match="finalize"):
        mcs.driver.run(prob, hb, n_itrs=2, max_pcuts=1, ensemble=e, triggers=[ens.Trigger(ps, "P_psd_par", "max", 1.0)])
    e.destroy()
    # two contexts, a products trigger: checks at the round ends with 4 iterations done; context 0 took 1 and 3, context 1 took 2 and 4
    z = prob.params.n_grid - 1
    trig = ens.Trigger(ps, "dNdp_sf", "max", 10.0, zones=(z, z + 1), bins=(1, NM - 1))
    bes = [hb, hip_backend(prob)]
    ovl = mcs.driver.run_overlapped(prob, bes, n_itrs=6, max_pcuts=N_PCUTS, ensemble=True, triggers=[trig], min_iterations=3)
    c, eo = ovl.convergence, ovl.ensemble
    assert c.satisfied and c.stopped_at == 4 and [it for it, _ in c.checks] == [4] and eo.count(ps) == 4 and eo.finalize_count == 4
    fins = {it: fin_parts(fin) for it, _, fin in ovl.iter_finals}
    with np.errstate(invalid="ignore", over="ignore"):
        merged = stat_of([fins[1], fins[3]]).merged_with(stat_of([fins[2], fins[4]]))
    for name in DNDP + SCALARS:
        assert same_words(eo.mean(ps, name), merged.mean[name]) and same_words(eo.m2(ps, name), merged.m2[name]), name
    (row,) = c.checks[0][1]
    first, count = eo.word_range(ps, "dNdp_sf", (z, z + 1), (1, NM - 1))
    want = restate(merged.mean["dNdp_sf"][z, 1:NM - 1], merged.m2["dNdp_sf"][z, 1:NM - 1], 4, 1e-3, 0.0)
    assert count == NM - 2 and row.met and row.summary.n == 4 and want["n_selected"] > 0
    assert_exact(as_dict(row.summary), want, "the check of the merged products")
    assert_sums(as_dict(row.summary), want, "the check of the merged products")
    eo.destroy()
    for be in bes:
        be.destroy()
