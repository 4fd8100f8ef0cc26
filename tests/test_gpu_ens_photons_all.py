"""The source slot of the ensemble statistics on the device -- the photon spectrum summed over species (csrc/mcs_ensemble.hip:
mcs_k_ens_add_photons_deposit, mcs_k_ens_add_vector, through ensemble.HipEnsemble) against ensemble.HostEnsemble fed the device's own
observation words and against the restatements in Python floats: the deposit and the take bit for bit, the summaries, the merged
summary and the comparison on its ranges, the refusals, the untouched accumulator, and the samples of driver.run and
driver.run_overlapped."""
import numpy as np
import pytest

from conftest import mcs, make_problem, hip_backend
from ensemble_common import crafted_buffers
from ens_summary_common import as_dict, assert_exact, assert_sums, restate, same_bits
import ens_compare_common as cmpc
from photons_all_common import LAYOUT, SPECIES_PROCESSES, bits_equal, deposit_restated, slot_words, welford_restated
from test_gpu_ens_photons import observe
from test_gpu_ens_products import consume

pytestmark = pytest.mark.gpu

cons, ens = mcs.consumers, mcs.ensemble
ALL = 1 << 28


def spectra_of(per):
    return cons.ObservedSpectra(tuple(per), per, {}, cons.photon_total(per, LAYOUT), None, LAYOUT, 0.1)


def feed(hb, dev, host, iterations, seed, plain=None):
    """Per iteration and species slot: mcs_photon_observe of seeded emission, the fused sample-and-deposit on `dev`, the same words
    into `host` (a HostEnsemble, or None); then the take.  plain: a second device accumulator that takes the same observation, made
    once more, by mcs_ens_add_photons."""
    for it in iterations:
        for s, processes in enumerate(SPECIES_PROCESSES):
            per = observe(hb, processes, seed + 10 * it + s)
            dev.add_photons(hb, s, deposit=True)
            assert dev.pending_photons == tuple(range(s + 1))
            if host is not None:
                host.add_photons(None, s, spectra_of(per), deposit=True)
            if plain is not None:
                again = observe(hb, processes, seed + 10 * it + s)
                assert all(bits_equal(again[p], per[p]) for p in per)
                plain.add_photons(hb, s)
        dev.add_photons_all()
        assert dev.pending_photons == ()
        if host is not None:
            host.add_photons_all()


def device_ensemble(hb, layout=LAYOUT):
    e = ens.HipEnsemble(hb, 3)
    if layout is not None:
        e.set_photon_layout(layout)
    return e


@pytest.fixture(scope="module")
def fed():
    prob = make_problem(64)
    hb = hip_backend(prob)
    dev, plain = device_ensemble(hb), device_ensemble(hb)
    host = ens.HostEnsemble(prob.params, 3)
    host.set_photon_layout(LAYOUT)
    feed(hb, dev, host, range(5), 0, plain)
    yield prob, hb, dev, plain, host
    dev.destroy(); plain.destroy(); hb.destroy()


def assert_same_slots(dev, host, what=""):
    off = LAYOUT.offsets()
    for slot in [dev.photons_slot(s) for s in range(3)] + [ALL]:
        assert dev.count(slot) == host.count(slot), (what, slot)
        if host.count(slot) == 0:
            continue
        a, b = slot_words(dev, slot), slot_words(host, slot)
        differ = {name: int((a[0] != b[0])[off[name][0]:off[name][0] + 4 * off[name][1]].sum()) for name in ens.PHOTON_NAMES}
        assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]), (what, slot, "words whose means differ, per section:", differ)


def test_deposit_and_take_are_bit_exact(fed):
    prob, hb, dev, plain, host = fed
    assert dev.count(ALL) == 5 and [dev.count(dev.photons_slot(s)) for s in range(3)] == [5, 5, 5] and dev.count(0) == 0 and dev.count(3) == 0
    assert_same_slots(dev, host)
    # the host ensemble is itself the rule: its source slot from its species' samples, by the restatement in Python floats
    mean, m2 = slot_words(dev, ALL)
    assert (mean > 1e-90).mean() > 0.3 and m2.max() > 0
    assert bits_equal(dev.mean(ALL, "total"), mean[LAYOUT.offsets()["total"][0]:].reshape(4, 31)) and dev.names(ALL) == ens.PHOTON_NAMES
    # the species' photons slots are what mcs_ens_add_photons gives
    assert plain.count(ALL) == 0 and plain.pending_photons == ()
    for s in range(3):
        a, b = slot_words(dev, dev.photons_slot(s)), slot_words(plain, plain.photons_slot(s))
        assert plain.count(plain.photons_slot(s)) == 5 and bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]), s
    # one iteration on its own, word by word in Python floats: first deposit, later deposits, take
    one = device_ensemble(hb)
    samples = []
    for s, processes in enumerate(SPECIES_PROCESSES):
        samples.append(spectra_of(observe(hb, processes, 300 + s)).sample())
        one.add_photons(hb, s, deposit=True)
    one.add_photons_all()
    got = slot_words(one, ALL)
    assert one.count(ALL) == 1 and bits_equal(got[0], deposit_restated(samples)) and not got[1].any()
    lit = sum((x > 1e-99).astype(int) for x in samples)
    assert (lit == 0).sum() > 0 and (lit == 1).sum() > 0 and (lit >= 2).sum() > 0
    one.destroy()


def test_summaries_and_comparison_of_the_source_slot(fed):
    prob, hb, dev, plain, host = fed
    mean, m2 = slot_words(dev, ALL)
    reqs = [ens.Request("total"), ens.Request("total", (3, 4), 1e-6, 0.5, (5, 25)), ens.Request("synch", (0, 2), 0.0, 0.3),
            ens.Request("pion", None, 1e-3, 0.1), ens.Request("ic", (1, 2), 0.5, 1.0, (0, 17)), ens.Request("total", (0, 1), 1.0, 0.0, (30, 31))]
    for q, s in zip(reqs, dev.summarize(ALL, reqs)):
        first, count = dev.word_range(ALL, q.name, q.zones, q.bins)
        want = restate(mean[first:first + count], m2[first:first + count], 5, q.floor_frac, q.tol)
        assert s.n == 5 and want["n_selected"] > 0
        assert_exact(as_dict(s), want, repr(q))
        assert_sums(as_dict(s), want, repr(q))
    # merged over two accumulators with 2 + 3 samples: what merging them into an empty one and summarising it gives; the merge is the
    # host ensemble's (Chan's)
    a, b, into = device_ensemble(hb), device_ensemble(hb), device_ensemble(hb, None)
    ha, hb_, hinto = (ens.HostEnsemble(prob.params, 3) for _ in range(3))
    ha.set_photon_layout(LAYOUT); hb_.set_photon_layout(LAYOUT)
    feed(hb, a, ha, range(2), 40)
    feed(hb, b, hb_, range(2, 5), 40)
    per = observe(hb, SPECIES_PROCESSES[1], 999)
    b.add_photons(hb, 1, deposit=True)                                   # a pending deposit is not merged and does not hinder
    hb_.add_photons(None, 1, spectra_of(per), deposit=True)
    merged = a.summarize_merged([b], ALL, reqs)
    assert into.count(ALL) == 0 and into.photon_layout is None
    into.merge(a); into.merge(b)                                         # (allocates in the destination, which takes the layout)
    hinto.merge(ha); hinto.merge(hb_)
    assert [x.count(ALL) for x in (a, b, into)] == [2, 3, 5] and into.photon_layout is LAYOUT and b.pending_photons == (1,) and into.pending_photons == ()
    assert_same_slots(into, hinto, "merged")
    for q, x, y in zip(reqs, merged, into.summarize(ALL, reqs)):
        dx, dy = as_dict(x), as_dict(y)
        assert x.n == y.n == 5
        for key in dx:
            assert same_bits(dx[key], dy[key]) if isinstance(dy[key], float) else dx[key] == dy[key], (q, key)
    # the comparison of two source slots
    mb, qb = slot_words(into, ALL)
    creqs = [ens.CompareRequest("total", None, 1e-9, 2.0), ens.CompareRequest("ic", (3, 4), 0.0, 1.0, (2, 15)), ens.CompareRequest("synch", (0, 3), 1e-3, 3.0)]
    for q, d in zip(creqs, dev.compare(into, ALL, creqs)):
        first, count = dev.word_range(ALL, q.name, q.zones, q.bins)
        sl = slice(first, first + count)
        w = cmpc.restate(mean[sl], m2[sl], 5, mb[sl], qb[sl], 5, q.floor_frac, q.zcut)
        assert w["n_selected"] > 0
        cmpc.assert_exact(cmpc.as_dict(d), w, repr(q))
        cmpc.assert_sums(cmpc.as_dict(d), w, repr(q))
    for x in (a, b, into):
        x.destroy()


def test_refusals_change_nothing_on_the_device(fed):
    prob, hb, fed_dev, plain, fed_host = fed
    dev, other = device_ensemble(hb), device_ensemble(hb)
    host = ens.HostEnsemble(prob.params, 3)
    host.set_photon_layout(LAYOUT)
    feed(hb, dev, host, range(2), 70)
    feed(hb, other, None, range(2), 80)
    # two deposits pending, on the device and in the mirror that sees no refused call
    for s in (0, 2):
        per = observe(hb, SPECIES_PROCESSES[s], 500 + s)
        dev.add_photons(hb, s, deposit=True)
        host.add_photons(None, s, spectra_of(per), deposit=True)
    before = {slot: slot_words(dev, slot) for slot in [ALL] + [dev.photons_slot(s) for s in range(3)]}
    hs = dev.photons_slot(0)
    odd = device_ensemble(hb, cons.PhotonLayout(3, LAYOUT.n, {"synch": 1, "ic": 9, "pion": 20}, 31))
    feed(hb, odd, None, range(2), 90)
    never = device_ensemble(hb)
    reqs, creqs = [ens.Request("total")], [ens.CompareRequest("total")]
    per1 = observe(hb, SPECIES_PROCESSES[1], 501)                          # the observation the refused deposits leave on the context
    refused = [
        ("mcs_ens_add_photons_deposit.*has been deposited", lambda: dev.add_photons(hb, 2, deposit=True)),      # a double deposit
        ("mcs_ens_add_photons_deposit", lambda: dev.add_photons(hb, 3, deposit=True)),                          # the iteration slot
        ("mcs_ens_add_photons_deposit", lambda: dev.add_photons(hb, ALL, deposit=True)),                        # no species slot
        ("mcs_ens_add_photons_all.*no deposit pending", lambda: never.add_photons_all()),
        ("mcs_ens_read.*source slot has never", lambda: never._read(ALL, 0, 0, 1)),
        ("mcs_ens_summarize", lambda: never._summarize(ALL, 0, [(0, 1, 0.0, 1.0)])),
        ("mcs_ens_load_mean", lambda: dev.load_mean(ALL, hb)),
        ("differ in kind", lambda: dev._compare(other, ALL, hs, 2, 2, [(0, 1, 0.0, 1.0)])),                     # (past the wrapper)
        ("differ in kind", lambda: dev._compare(other, hs, ALL, 2, 2, [(0, 1, 0.0, 1.0)])),
        ("mcs_ens_count", lambda: dev.count((1 << 29) | 3)),                                                    # still no species slot 3
        ("mcs_ens_set_photon_layout", lambda: ens.HipEnsemble._set_photon_layout(dev, LAYOUT)),                 # the layout is fixed
        ("photon layouts differ", lambda: dev.merge(odd)),
        ("photon layouts differ", lambda: odd.merge(dev)),
        ("photon layouts differ", lambda: dev.summarize_merged([odd], ALL, reqs)),
        ("photon layouts differ", lambda: dev.compare(odd, ALL, creqs)),
    ]
    for who, call in refused:
        with pytest.raises(RuntimeError, match=who):
            call()
    with pytest.raises(ValueError, match="source slot with a photons slot"):
        dev.compare(other, ALL, creqs, hs)
    assert never.count(ALL) == 0 and dev.pending_photons == (0, 2)
    for slot, (mean, m2) in before.items():
        after = slot_words(dev, slot)
        assert bits_equal(after[0], mean) and bits_equal(after[1], m2), slot
    # the refused deposits left the context's observation in place: species 1 deposits it now, without a new one; the pending vector
    # and the bookkeeping are what the mirror's are -- the take gives its bits
    dev.add_photons(hb, 1, deposit=True)
    host.add_photons(None, 1, spectra_of(per1), deposit=True)
    with pytest.raises(RuntimeError, match="mcs_ens_add_photons_deposit"):
        dev.add_photons(hb, 1, deposit=True)                               # (and that deposit took the observation)
    assert dev.pending_photons == host.pending_photons == (0, 2, 1)
    dev.add_photons_all(); host.add_photons_all()
    assert_same_slots(dev, host, "after the refusals")
    # dropping: the species deposits again, and the vector starts anew
    for s in (0, 1):
        per = observe(hb, SPECIES_PROCESSES[s], 600 + s)
        dev.add_photons(hb, s, deposit=True)
        host.add_photons(None, s, spectra_of(per), deposit=True)               # (the dropped ones are samples of their species too)
    dev.drop_pending_photons(); host.drop_pending_photons()
    assert dev.pending_photons == ()
    with pytest.raises(RuntimeError, match="no deposit pending"):
        dev.add_photons_all()
    per = observe(hb, SPECIES_PROCESSES[0], 700)
    dev.add_photons(hb, 0, deposit=True); dev.add_photons_all()
    host.add_photons(None, 0, spectra_of(per), deposit=True); host.add_photons_all()
    assert_same_slots(dev, host, "after the drop")
    for x in (dev, other, odd, never):
        x.destroy()


def test_an_accumulator_that_never_deposits_is_what_it_was(fed):
    prob, hb, fed_dev, plain, fed_host = fed
    L = mcs.capi.Layout(prob.params)
    tabs_c = cons.consumer_tables(prob, 1)
    x_log = ens.bin_centres_log10(prob)
    today, both = ens.HipEnsemble(hb, 1), ens.HipEnsemble(hb, 1)
    for acc in (today, both):
        acc.set_photon_layout(LAYOUT)
        acc.set_slope_window(10, 50, x_log)
    prev = np.zeros(L.total)
    for k, (f, i) in enumerate(crafted_buffers(L, 3)):
        hb.write_tallies(prev, i)
        today.begin_iteration(hb); both.begin_iteration(hb)
        hb.write_tallies(f, i)
        today.add_species(hb, 0); both.add_species(hb, 0)
        observe(hb, SPECIES_PROCESSES[k], 90 + k)
        today.add_photons(hb, 0)
        observe(hb, SPECIES_PROCESSES[k], 90 + k)
        both.add_photons(hb, 0, deposit=True); both.add_photons_all()
        consume(hb, tabs_c); today.add_products(hb, 0)
        consume(hb, tabs_c); both.add_products(hb, 0)
        today.add_iteration(hb); both.add_iteration(hb)
        prev = f
    hs, ps = today.photons_slot(0), today.products_slot(0)
    assert today.count(ALL) == 0 and both.count(ALL) == 3 and today.pending_photons == ()
    for slot in (0, 1, hs, ps):
        assert today.count(slot) == both.count(slot) == 3, slot
    for slot in (0, 1, hs):
        n = today._len(slot)
        for what in (0, 1):
            assert bits_equal(today._read(slot, what, 0, n), both._read(slot, what, 0, n)), (slot, what)
    # (the consumers add with atomics: of a products slot only the shock-frame dN/dp, a sum in a fixed order per thread, repeats)
    assert bits_equal(today.mean(ps, "dNdp_sf"), both.mean(ps, "dNdp_sf")) and bits_equal(today.m2(ps, "dNdp_sf"), both.m2(ps, "dNdp_sf"))
    with pytest.raises(RuntimeError, match="mcs_ens_read"):
        today._read(ALL, 0, 0, 1)
    into = ens.HipEnsemble(hb, 1)
    into.merge(today)
    assert into.count(ALL) == 0 and into.count(hs) == 3
    for x in (today, both, into):
        x.destroy()


ME_MP = mcs.constants.ME / mcs.constants.MP
SETUP = cons.PhotonSetup(3, 3, jet_dist_kpc=1.0e3)


def electron_problem():
    return make_problem(300, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(ME_MP, -1.0, 1e6, 1.0)], radiation_losses=True,
                        B_mag_upstream=3e-3, JETFR=(0.0, 20.0), num_iterations=4)


def test_run_takes_one_source_sample_per_iteration():
    prob = electron_problem()
    hb = hip_backend(prob)
    e = ens.Ensemble.for_backend(hb, 2)
    state, fed_samples = None, []
    for it in (1, 2, 3):
        r = mcs.driver.run(prob, hb, n_itrs=1, first_iter=it, iter_state=state, max_pcuts=8, finalize=True, photons=SETUP, ensemble=e)
        state = r.iter_state
        fed_samples.append([r.photons[s].sample() for s in (0, 1)])
        assert e.count(ALL) == it and e.pending_photons == ()
    n = e.photon_layout.offsets()["_total"]
    assert e.photon_layout.args() == (6, 179, 139, 119, 0, 110, 130, 250)
    mean, m2 = welford_restated([deposit_restated(samples) for samples in fed_samples])
    got = slot_words(e, ALL, n)
    assert bits_equal(got[0], mean) and bits_equal(got[1], m2)
    rows = e.photon_layout.rows
    all_shells, all_m2 = e.mean(ALL, "total")[rows - 1], e.m2(ALL, "total")[rows - 1]
    print("lit words of the mean all-shells total of the source:", int((all_shells > 1e-98).sum()), "; largest M2:", all_m2.max())
    assert (all_shells > 1e-98).sum() > 0 and all_m2.max() > 0
    assert [e.count(e.photons_slot(s)) for s in (0, 1)] == [3, 3] and e.count(e.products_slot(1)) == 3 and e.count(2) == 3
    e.destroy(); hb.destroy()


def test_run_overlapped_feeds_the_source_slot():
    prob = electron_problem()
    bes = [hip_backend(prob), hip_backend(prob)]
    ovl = mcs.driver.run_overlapped(prob, bes, n_itrs=4, max_pcuts=8, ensemble=True, photons=SETUP)
    e = ovl.ensemble
    h0, h1 = e.photons_slot(0), e.photons_slot(1)
    assert [e.count(s) for s in (h0, h1, ALL)] == [4, 4, 4] and e.count(e.products_slot(1)) == 4 and e.count(2) == 4 and e.finalize_count == 4
    assert len(ovl.photons) == 2 and ovl.photons[0].processes == ("pion",) and ovl.photons[1].processes == ("synch", "ic")
    assert len(ovl.iter_finals) == 4
    # Linearity.  Every term is non-negative; the rounding of the Welford means, the Chan merges and the species sum stays below
    # (n + n_species + 4) 2^-53 relative, the floors add at most 3e-99: 1e-12 is a derived bound with three orders of slack
    n = e.photon_layout.offsets()["_total"]
    mean_all = e._read(ALL, 0, 0, n)
    mean_sum = e._read(h0, 0, 0, n) + e._read(h1, 0, 0, n)
    sel = mean_all > 1e-80
    worst = float((np.abs(mean_all - mean_sum)[sel] / mean_all[sel]).max()) if sel.any() else float("nan")
    print("words of the source mean above 1e-80:", int(sel.sum()), "; largest relative distance from the sum of the species' means:", worst)
    assert sel.sum() > 0 and np.all(np.abs(mean_all - mean_sum)[sel] <= 1e-12 * mean_all[sel])
    e.destroy()
    # the stop rule on the source slot's total: 1.5 is met by whatever is selected (a relative standard error is at most 1), at the
    # first check -- the end of the first round
    rows = cons.stock_photon_layout(SETUP.n_shells).rows
    trig = ens.Trigger(ALL, "total", "max", 1.5, zones=(rows - 1, rows))
    with pytest.raises(ValueError, match="source slot needs photons="):
        mcs.driver.run_overlapped(prob, bes, n_itrs=4, max_pcuts=1, ensemble=True, triggers=[trig])
    with pytest.raises(ValueError, match="photons slot needs photons="):
        mcs.driver.run_overlapped(prob, bes, n_itrs=4, max_pcuts=1, ensemble=True, triggers=[ens.Trigger(h0, "total", "max", 1.5)])
    stop = mcs.driver.run_overlapped(prob, bes, n_itrs=4, max_pcuts=8, ensemble=True, photons=SETUP, triggers=[trig])
    c = stop.convergence
    assert c.satisfied and c.stopped_at == 2 and [it for it, _ in c.checks] == [2] and stop.ensemble.count(ALL) == 2
    assert c.checks[0][1][0].summary.n == 2 and c.checks[0][1][0].summary.n_selected > 0 and len(stop.photons) == 2
    stop.ensemble.destroy()
    # without photons= the run is what it is: no spectra, no photons sample, no layout
    plain = mcs.driver.run_overlapped(prob, bes, n_itrs=2, max_pcuts=8, ensemble=True)
    assert plain.photons is None and plain.ensemble.photon_layout is None and plain.ensemble.pending_photons == ()
    assert [plain.ensemble.count(s) for s in (h0, h1, ALL)] == [0, 0, 0] and plain.ensemble.count(2) == 2 and plain.ensemble.count(plain.ensemble.products_slot(1)) == 2
    assert len(plain.iter_finals) == 2 and plain.convergence is None
    plain.ensemble.destroy()
    for be in bes:
        be.destroy()
