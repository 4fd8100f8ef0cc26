"""The photons slot of the ensemble statistics on the device (csrc/mcs_ensemble.hip: mcs_k_ens_add_photons, through
ensemble.HipEnsemble) against plain numpy: the sample vector and its update bit for bit, the summaries, the merged summary and the
comparison on photons ranges, the lazy allocation, the refusals, and the driver's samples."""
import numpy as np
import pytest

from conftest import mcs, make_problem, hip_backend
from ensemble_common import bits_equal, crafted_buffers, species_parts, stat_of
from ens_summary_common import as_dict, assert_exact, assert_sums, restate, same_bits
import ens_compare_common as cmpc
from photon_observed_common import BETAS, tables
from test_gpu_ens_products import NAMES as PRODUCT_NAMES, consume, parts_of as product_parts, same_words, slopes_restated

pytestmark = pytest.mark.gpu

cons, ens = mcs.consumers, mcs.ensemble
N_PHOTON = {"synch": 24, "ic": 18, "pion": 12}
LAYOUT = cons.PhotonLayout(3, {p: n - 1 for p, n in N_PHOTON.items()}, {"synch": 0, "ic": 9, "pion": 20}, 31)
ENDS = [1, 4, 9, 30]
# which processes each of the five crafted observations holds
PLAN = (("synch", "ic"), ("pion",), ("synch", "ic", "pion"), ("ic",), ("pion", "synch"))


def observe(hb, processes, seed, n_photon=N_PHOTON, ends=ENDS):
    """mcs_photon_observe of seeded random emission for the named processes -> process -> the device's own words on the host."""
    ng = hb.P.n_grid
    rng = np.random.default_rng(seed)
    out = {}
    for p in processes:
        tabs = tables(p, ng, n_photon[p], BETAS, ends)
        flux = np.where(rng.random((ng, n_photon[p])) < 0.7, 10.0 ** rng.uniform(-14, -2, (ng, n_photon[p])), 1e-99)
        emis = flux * tabs["energy_div"][None, :] * (cons.MEV_ERG if p == "ic" else tabs["area"] * (cons.MEV_ERG if p == "synch" else 1.0))
        out[p] = hb.photon_observe(p, emis=emis, **tabs)
    return out


def total_restated(per):
    """The total section from the statement in include/mcs.h, word by word in Python floats."""
    ns = LAYOUT.n_shells
    tot = np.empty((ns + 1, LAYOUT.n_pts))
    for t in range(LAYOUT.n_pts):
        col = 0.0
        for s in range(ns):
            x = 1.0e-99
            for p in ("pion", "synch", "ic"):
                if p in per and LAYOUT.start[p] <= t < LAYOUT.start[p] + LAYOUT.n[p]:
                    v = float(per[p][s, t - LAYOUT.start[p]])
                    x = x + (v if v > 1.0e-99 else 0.0)
            tot[s, t] = x
            col = col + x
        tot[ns, t] = col
    return tot


def parts_of(per):
    p = {name: per[name] if name in per else np.full((LAYOUT.rows, LAYOUT.n[name]), 1e-99) for name in cons.PHOTON_PROCESSES}
    p["total"] = total_restated(per)
    return p


def slot_words(e, slot):
    n = LAYOUT.offsets()["_total"]
    return e._read(slot, 0, 0, n), e._read(slot, 1, 0, n)


def feed(hb, e, slot, plan, seed):
    parts = []
    for k, processes in enumerate(plan):
        parts.append(parts_of(observe(hb, processes, seed + k)))
        e.add_photons(hb, slot)
    return parts


@pytest.fixture(scope="module")
def fed():
    prob = make_problem(64)
    hb = hip_backend(prob)
    e = ens.HipEnsemble(hb, 2)
    e.set_photon_layout(cons.PhotonLayout(2, LAYOUT.n, LAYOUT.start, 40))      # (may be called again until the first sample)
    e.set_photon_layout(LAYOUT)
    parts = feed(hb, e, 1, PLAN, 0)
    yield prob, hb, e, parts
    e.destroy(); hb.destroy()


def test_update_is_bit_exact(fed):
    prob, hb, e, parts = fed
    hs = e.photons_slot(1)
    assert e.count(hs) == 5 and e.count(e.photons_slot(0)) == 0 and e.count(e.products_slot(1)) == 0 and e.count(1) == 0 and e.count(2) == 0
    want = stat_of(parts)
    for name in ens.PHOTON_NAMES:
        assert bits_equal(e.mean(hs, name), want.mean[name]), f"mean of {name}"
        assert bits_equal(e.m2(hs, name), want.m2[name]), f"M2 of {name}"
        assert bits_equal(e.stderr(hs, name), np.sqrt(want.m2[name] / 20.0)), name
    assert want.m2["total"].max() > 0 and (want.mean["total"] > 1e-90).mean() > 0.5
    # an absent process reads 1e-99: one sample of pion alone
    one = ens.HipEnsemble(hb, 1)
    one.set_photon_layout(LAYOUT)
    per = observe(hb, ("pion",), 77)
    one.add_photons(hb, 0)
    h0 = one.photons_slot(0)
    assert np.all(one.mean(h0, "synch") == 1e-99) and np.all(one.mean(h0, "ic") == 1e-99) and bits_equal(one.mean(h0, "pion"), per["pion"])
    assert bits_equal(one.mean(h0, "total"), total_restated(per)) and bits_equal(one.mean(h0, "total"), cons.photon_total(per, LAYOUT))
    assert not np.any(one.m2(h0, "total"))
    one.destroy()


def test_refusals_change_nothing(fed):
    prob, hb, e, parts = fed
    hs = e.photons_slot(1)
    before = slot_words(e, hs)
    fresh = ens.HipEnsemble(hb, 2)            # (no layout)
    observe(hb, ("synch",), 5)
    with pytest.raises(RuntimeError, match="no photon layout"):
        fresh.add_photons(hb, 0)
    # a refused mcs_photon_observe leaves the previous result where it was: the sample that follows is that result's
    kept = observe(hb, ("pion",), 6)
    tabs = tables("pion", hb.P.n_grid, N_PHOTON["pion"], BETAS, ENDS)
    bad = np.array(tabs["beta_ef"]); bad[3] = 1.0
    with pytest.raises(RuntimeError, match="beta_ef"):
        hb.photon_observe("pion", emis=np.ones((hb.P.n_grid, N_PHOTON["pion"])), **dict(tabs, beta_ef=bad))
    fresh.set_photon_layout(LAYOUT)
    fresh.add_photons(hb, 0)
    assert bits_equal(fresh.mean(fresh.photons_slot(0), "pion"), kept["pion"]) and fresh.count(fresh.photons_slot(0)) == 1
    other_shells = tables("ic", hb.P.n_grid, N_PHOTON["ic"], BETAS, [1, 4, 9])
    refused = [
        ("mcs_ens_add_photons", lambda: e.add_photons(hb, 1)),                        # a second sample without a fresh observation
        ("mcs_ens_add_photons", lambda: (observe(hb, ("ic",), 1), e.add_photons(hb, 2))),           # the iteration slot
        ("mcs_ens_add_photons", lambda: e.add_photons(hb, hs)),                       # out of range
        ("mcs_ens_add_photons", lambda: (hb.photon_observe("ic", emis=np.ones((hb.P.n_grid, N_PHOTON["ic"])), **other_shells), e.add_photons(hb, 1))),
        ("mcs_ens_set_photon_layout", lambda: e.set_photon_layout(LAYOUT)),           # after the first sample
        ("mcs_ens_set_photon_layout", lambda: fresh._set_photon_layout(cons.PhotonLayout(0, LAYOUT.n, LAYOUT.start, 31))),
        ("mcs_ens_set_photon_layout", lambda: ens.HipEnsemble._set_photon_layout(e2, cons.PhotonLayout(3, LAYOUT.n, LAYOUT.start, 30))),
        ("mcs_ens_read", lambda: e.mean(e.photons_slot(0), "total")),                 # never sampled
        ("mcs_ens_read", lambda: fresh.stderr(fresh.photons_slot(0), "total")),       # n = 1
        ("mcs_ens_count", lambda: e.count((1 << 29) | 2)),                            # no species slot 2
        ("mcs_ens_load_mean", lambda: e.load_mean(hs, hb)),
    ]
    e2 = ens.HipEnsemble(hb, 1)
    for who, call in refused:
        with pytest.raises(RuntimeError, match=who):
            call()
    # after mcs_begin_species the earlier observation no longer counts
    observe(hb, ("synch",), 8)
    hb.begin_species(1, 1, 1.0, 1.0, prob.pmax, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="mcs_ens_add_photons"):
        e.add_photons(hb, 1)
    after = slot_words(e, hs)
    assert e.count(hs) == 5 and bits_equal(before[0], after[0]) and bits_equal(before[1], after[1])
    fresh.destroy(); e2.destroy()


def test_summaries_and_comparison_of_a_photons_slot(fed):
    prob, hb, e, parts = fed
    hs = e.photons_slot(1)
    mean, m2 = slot_words(e, hs)
    reqs = [ens.Request("total"), ens.Request("total", (3, 4), 1e-6, 0.5, (5, 25)), ens.Request("synch", (0, 2), 0.0, 0.3),
            ens.Request("pion", None, 1e-3, 0.1), ens.Request("ic", (1, 2), 0.5, 1.0, (0, 17)), ens.Request("total", (0, 1), 1.0, 0.0, (30, 31))]
    for q, s in zip(reqs, e.summarize(hs, reqs)):
        first, count = e.word_range(hs, q.name, q.zones, q.bins)
        want = restate(mean[first:first + count], m2[first:first + count], 5, q.floor_frac, q.tol)
        assert s.n == 5 and want["n_selected"] > 0
        assert_exact(as_dict(s), want, repr(q))
        assert_sums(as_dict(s), want, repr(q))
    assert e.word_range(hs, "total", (3, 4), (5, 25)) == (LAYOUT.offsets()["total"][0] + 3 * 31 + 5, 20)
    # merged over two accumulators with 2 + 3 samples: what merging them into an empty one and summarising it gives; the merge is Chan's
    a, b, into = (ens.HipEnsemble(hb, 2) for _ in range(3))
    a.set_photon_layout(LAYOUT); b.set_photon_layout(LAYOUT)
    pa, pb = feed(hb, a, 1, PLAN[:2], 40), feed(hb, b, 1, PLAN[2:], 42)
    merged = a.summarize_merged([b], hs, reqs)
    assert into.count(hs) == 0 and into.photon_layout is None
    into.merge(a); into.merge(b)                                   # (allocates in the destination, which takes the layout)
    assert [x.count(hs) for x in (a, b, into)] == [2, 3, 5] and into.photon_layout is LAYOUT
    for q, x, y in zip(reqs, merged, into.summarize(hs, reqs)):
        dx, dy = as_dict(x), as_dict(y)
        assert x.n == y.n == 5
        for key in dx:
            assert same_bits(dx[key], dy[key]) if isinstance(dy[key], float) else dx[key] == dy[key], (q, key)
    want = stat_of(pa).merged_with(stat_of(pb))
    for name in ens.PHOTON_NAMES:
        assert bits_equal(into.mean(hs, name), want.mean[name]) and bits_equal(into.m2(hs, name), want.m2[name]), name
    # the comparison of two photons slots
    mb, qb = slot_words(into, hs)
    creqs = [ens.CompareRequest("total", None, 1e-9, 2.0), ens.CompareRequest("ic", (3, 4), 0.0, 1.0, (2, 15)), ens.CompareRequest("synch", (0, 3), 1e-3, 3.0)]
    for q, d in zip(creqs, e.compare(into, hs, creqs)):
        first, count = e.word_range(hs, q.name, q.zones, q.bins)
        sl = slice(first, first + count)
        w = cmpc.restate(mean[sl], m2[sl], 5, mb[sl], qb[sl], 5, q.floor_frac, q.zcut)
        assert w["n_selected"] > 0
        cmpc.assert_exact(cmpc.as_dict(d), w, repr(q))
        cmpc.assert_sums(cmpc.as_dict(d), w, repr(q))
    with pytest.raises(RuntimeError, match="differ in kind"):
        e._compare(into, hs, 1, 5, 5, [(0, 1, 0.0, 1.0)])              # (past the wrapper, which refuses first)
    # other layouts are refused: merge, merged summary, comparison
    odd = ens.HipEnsemble(hb, 2)
    odd.set_photon_layout(cons.PhotonLayout(3, LAYOUT.n, {"synch": 1, "ic": 9, "pion": 20}, 31))
    feed(hb, odd, 1, PLAN[:2], 60)
    for call in (lambda: a.merge(odd), lambda: odd.merge(a), lambda: a.summarize_merged([odd], hs, reqs), lambda: a.compare(odd, hs, creqs)):
        with pytest.raises(RuntimeError, match="photon layouts differ"):
            call()
    assert a.count(hs) == 2 and odd.count(hs) == 2
    for x in (a, b, into, odd):
        x.destroy()


def test_an_accumulator_without_photons_is_what_it_was(fed):
    prob, hb, e_fed, parts = fed
    L = mcs.capi.Layout(prob.params)
    tabs_c = cons.consumer_tables(prob, 1)
    x_log = ens.bin_centres_log10(prob)
    bufs = crafted_buffers(L, 3)
    plain, both = ens.HipEnsemble(hb, 1), ens.HipEnsemble(hb, 1)
    both.set_photon_layout(LAYOUT)
    for acc in (plain, both):
        acc.set_slope_window(10, 50, x_log)
    prev = np.zeros(L.total)
    fed_plain, fed_both = [], []                  # what each accumulator's products slot was fed: the consumers' own bits of that run
    for k, (f, i) in enumerate(bufs):
        hb.write_tallies(prev, i)
        plain.begin_iteration(hb)
        both.begin_iteration(hb)
        hb.write_tallies(f, i)
        fed_plain.append(consume(hb, tabs_c))
        observe(hb, PLAN[k], 90 + k)
        plain.add_species(hb, 0); both.add_species(hb, 0)
        both.add_photons(hb, 0)
        plain.add_products(hb, 0)
        fed_both.append(consume(hb, tabs_c))
        both.add_products(hb, 0)
        plain.add_iteration(hb); both.add_iteration(hb)
        prev = f
    hs, ps = plain.photons_slot(0), plain.products_slot(0)
    assert plain.count(hs) == 0 and both.count(hs) == 3 and plain.count(0) == both.count(0) == 3 and plain.count(1) == both.count(1) == 3
    want = stat_of([species_parts(L, f, i) for f, i in bufs])
    for name in want.mean:
        for acc in (plain, both):
            assert bits_equal(acc.mean(0, name), want.mean[name]) and bits_equal(acc.m2(0, name), want.m2[name]), name
    n_it = plain.layout.iteration_total
    for what in (0, 1):
        assert bits_equal(plain._read(1, what, 0, n_it), both._read(1, what, 0, n_it))
    # the products slots: the consumers add with atomics, so the two accumulators took different runs of them and are not compared
    # with each other; each holds, in every part, the statistics of exactly what it was fed -- with a photons slot beside it or not
    assert plain.count(ps) == both.count(ps) == 3
    for acc, outs in ((plain, fed_plain), (both, fed_both)):
        want_p = stat_of([product_parts(o, slopes_restated(hb, o[0], 10, 50, x_log)) for o in outs])
        for name in PRODUCT_NAMES:
            assert same_words(acc.mean(ps, name), want_p.mean[name]), f"mean of {name}"
            assert same_words(acc.m2(ps, name), want_p.m2[name]), f"M2 of {name}"
    # (the shock-frame dN/dp is a sum in a fixed order per thread: it does repeat)
    assert bits_equal(plain.mean(ps, "dNdp_sf"), both.mean(ps, "dNdp_sf")) and bits_equal(plain.m2(ps, "dNdp_sf"), both.m2(ps, "dNdp_sf"))
    with pytest.raises(RuntimeError, match="mcs_ens_read"):
        plain._read(hs, 0, 0, 1)                  # (it has no layout either: the wrapper's named read would say so first)
    into = ens.HipEnsemble(hb, 1)
    into.merge(plain)
    assert into.count(hs) == 0 and into.photon_layout is None
    plain.destroy(); both.destroy(); into.destroy()


ME_MP = mcs.constants.ME / mcs.constants.MP


def test_driver_feeds_the_photons_slots():
    prob = make_problem(300, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(ME_MP, -1.0, 1e6, 1.0)], radiation_losses=True,
                        B_mag_upstream=3e-3, JETFR=(0.0, 20.0), num_iterations=4)
    hb = hip_backend(prob)
    setup = cons.PhotonSetup(3, 3, jet_dist_kpc=1.0e3)
    run = mcs.driver.run
    # the content of the samples: three iterations stepped through one run() each, so that every iteration's spectra come back
    # (RunResult.photons, the device's own words); the slot then holds the Welford statistics of exactly those, bit for bit
    e1 = ens.Ensemble.for_backend(hb, 2)
    h0, h1 = e1.photons_slot(0), e1.photons_slot(1)
    state, samples = None, {0: [], 1: []}
    for it in (1, 2, 3):
        r = run(prob, hb, n_itrs=1, first_iter=it, iter_state=state, max_pcuts=8, finalize=True, photons=setup, ensemble=e1)
        state = r.iter_state
        assert len(r.photons) == 2 and r.photons[0].processes == ("pion",) and r.photons[1].processes == ("synch", "ic")
        for s in (0, 1):
            samples[s].append(r.photons[s].sample())
    assert e1.photon_layout.args() == (6, 179, 139, 119, 0, 110, 130, 250)
    n = e1.photon_layout.offsets()["_total"]
    lit = 0
    for s, slot in ((0, h0), (1, h1)):
        mean, m2, k = np.zeros(n), np.zeros(n), 0
        for x in samples[s]:
            assert x.shape == (n,)
            k = ens.welford_update(mean, m2, k, x)
        assert e1.count(slot) == 3 and bits_equal(e1._read(slot, 0, 0, n), mean) and bits_equal(e1._read(slot, 1, 0, n), m2), s
        lit += int((mean > 1e-99).sum())
    lit_pion = int((e1.mean(h0, "pion")[6] > 1e-99).sum())
    print("lit words of the two means:", lit, "; of the mean pion-decay spectrum of all shells:", lit_pion)
    assert lit_pion > 0 and e1.m2(h0, "pion").max() > 0
    e1.destroy()
    # the stop rule on photons slots, both triggers on the protons' lit pion-decay spectrum of all shells.  Samples are not negative,
    # so a relative standard error is at most 1 (one sample lit, the others dark): 1.5 is met by whatever is selected; 1e-15 is not
    # met by Monte-Carlo spectra that differ from iteration to iteration
    e = ens.Ensemble.for_backend(hb, 2)
    met = ens.Trigger(h0, "total", "max", 1.5, zones=(6, 7))
    unmet = ens.Trigger(h0, "pion", "max", 1e-15, zones=(6, 7))
    with pytest.raises(ValueError, match="photons slot needs photons="):
        run(prob, hb, n_itrs=2, max_pcuts=1, finalize=True, ensemble=e, triggers=[met])
    res = run(prob, hb, n_itrs=3, max_pcuts=8, finalize=True, photons=setup, ensemble=e, triggers=[met, unmet])
    assert e.count(h0) == e.count(h1) == 3 and e.count(e.products_slot(1)) == 3 and e.count(0) == 3 and len(res.photons) == 2
    c = res.convergence
    assert c is not None and not c.satisfied and c.stopped_at == 3 and [it for it, _ in c.checks] == [2, 3]
    for (it, rows), n_samples in zip(c.checks, (2, 3)):
        assert rows[0].met and not rows[1].met and rows[0].summary.n == rows[1].summary.n == n_samples
        assert rows[0].summary.n_selected > 0 and rows[1].summary.n_selected > 0
    mean, m2 = e._read(h0, 0, 0, n), e._read(h0, 1, 0, n)
    for row in c.checks[-1][1]:
        t = row.trigger
        first, count = e.word_range(h0, t.name, t.zones, t.bins)
        want = restate(mean[first:first + count], m2[first:first + count], 3, t.floor_frac, 0.0)
        assert_exact(as_dict(row.summary), want, repr(t))
        assert_sums(as_dict(row.summary), want, repr(t))
    print("max_rel of the two triggers:", c.checks[-1][1][0].value, c.checks[-1][1][1].value)
    assert 1e-15 < c.checks[-1][1][1].value <= 1.5
    e.destroy(); hb.destroy()
