"""The source slot of the ensemble statistics on the host -- the photon spectrum summed over species, sampled once per iteration
(include/mcs.h, "source sample"): the exported calls, ensemble.HostEnsemble against a restatement of the deposit rule and of the update in
Python floats, the refusals, the merge, and driver.run(photons=, ensemble=) on the CPU oracle.  Equal bits everywhere: the device
(tests/test_gpu_ens_photons_all.py) is held to the same."""
import numpy as np
import pytest

from conftest import mcs, make_problem, oracle_backend
from ensemble_common import crafted_buffers
from photons_all_common import LAYOUT, bits_equal, chan_restated, crafted_species, deposit_restated, slot_words, welford_restated

cons, ens = mcs.consumers, mcs.ensemble
ALL = 1 << 28


def test_library_exports_the_new_calls():
    lib = mcs.capi.load_library()
    for name in ("mcs_ens_add_photons_deposit", "mcs_ens_add_photons_all", "mcs_ens_drop_pending_photons"):
        assert hasattr(lib, name) and name in mcs.capi.EXPORTED_SYMBOLS, name
    for name, call in (("mcs_ens_add_photons_deposit", lambda: lib.mcs_ens_add_photons_deposit(None, None, 0)),
                       ("mcs_ens_add_photons_all", lambda: lib.mcs_ens_add_photons_all(None)),
                       ("mcs_ens_drop_pending_photons", lambda: lib.mcs_ens_drop_pending_photons(None))):
        assert call() != 0 and name.encode() in lib.mcs_last_error() and b"null argument" in lib.mcs_last_error(), name
    assert mcs.capi.ENS_PHOTONS_ALL == ALL == ens.Ensemble.photons_all_slot


def feed(e, iterations, seed=0, deposit=True, layout=LAYOUT):
    """Every species of every iteration sampled (and deposited), one take per iteration -> per iteration the species' sample vectors."""
    fed = []
    for it in iterations:
        obs = crafted_species(it, seed, layout)
        for s, o in enumerate(obs):
            e.add_photons(None, s, o, deposit=deposit)
            if deposit:
                assert e.pending_photons == tuple(range(s + 1))
        if deposit:
            e.add_photons_all()
            assert e.pending_photons == ()
        fed.append([o.sample() for o in obs])
    return fed


def fresh(prob, layout=LAYOUT):
    e = ens.HostEnsemble(prob.params, 3)
    if layout is not None:
        e.set_photon_layout(layout)
    return e


def state_of(e):
    """Everything a refused call must leave as it was."""
    vec = lambda a: None if a is None else a.copy()
    hs = {s: e._slots[e.photons_slot(s)] for s in range(e.n_species) if e.photons_slot(s) in e._slots}      # (absent: never allocated)
    src = e._slots.get(ALL)
    return dict(hmean={s: x.mean.copy() for s, x in hs.items()}, hm2={s: x.m2.copy() for s, x in hs.items()},
                hn=[e.count(e.photons_slot(s)) for s in range(e.n_species)], amean=vec(src and src.mean), am2=vec(src and src.m2), an=e.count(ALL),
                pending=vec(e._pending), deposited=e.pending_photons, layout=e.photon_layout)


def same_state(a, b):
    for key in ("hn", "an", "deposited"):
        if a[key] != b[key]:
            return False
    if a["layout"] is not b["layout"] or a["hmean"].keys() != b["hmean"].keys():
        return False
    pairs = [(a[k], b[k]) for k in ("amean", "am2", "pending")] + [(a[k][s], b[k][s]) for k in ("hmean", "hm2") for s in a[k]]
    return all((x is None and y is None) or (x is not None and y is not None and bits_equal(x, y)) for x, y in pairs)


def test_the_source_slot_is_the_deposit_rule_then_welford():
    prob = make_problem(64)
    e, plain = fresh(prob), fresh(prob)
    assert e.is_photons_all(ALL) and not e.is_photons(ALL) and not e.is_products(ALL) and not e.is_photons_all(e.photons_slot(0))
    assert e._kind(ALL) == "source" and e.names(ALL) == ens.PHOTON_NAMES and e.count(ALL) == 0 and e.pending_photons == ()
    fed = feed(e, range(5))
    feed(plain, range(5), deposit=False)
    # the crafted words: lit in no species, in one, in several; and values above the floor that the floor changes
    lit = sum((x > 1e-99).astype(int) for x in fed[0])
    tiny = np.concatenate([x[(x > 1e-99) & (x < 1e-98)] for x in fed[0]])
    assert (lit == 0).sum() > 10 and (lit == 1).sum() > 10 and (lit >= 2).sum() > 10 and tiny.size > 10 and np.all(1e-99 + tiny != tiny)
    mean, m2 = welford_restated([deposit_restated(samples) for samples in fed])
    got = slot_words(e, ALL)
    assert e.count(ALL) == 5 and bits_equal(got[0], mean) and bits_equal(got[1], m2) and m2.max() > 0
    # the species' photons slots are what add_photons without a deposit gives, and that is the update of their samples
    for s in range(3):
        hs = e.photons_slot(s)
        want = welford_restated([samples[s] for samples in fed])
        a, b = slot_words(e, hs), slot_words(plain, hs)
        assert e.count(hs) == plain.count(hs) == 5
        assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]) and bits_equal(a[0], want[0]) and bits_equal(a[1], want[1]), s
    assert plain.count(ALL) == 0 and plain._pending is None and ALL not in plain._slots
    # names, ranges, summaries and a trigger work on it as on a photons slot
    off = LAYOUT.offsets()
    assert e.word_range(ALL, "total", (3, 4), (5, 12)) == (off["total"][0] + 3 * 31 + 5, 7) == e.word_range(e.photons_slot(1), "total", (3, 4), (5, 12))
    assert bits_equal(e.mean(ALL, "ic"), mean[off["ic"][0]:off["pion"][0]].reshape(4, 17))
    assert bits_equal(e.stderr(ALL, "total"), np.sqrt(m2[off["total"][0]:] / 20.0).reshape(4, 31))
    reqs = [ens.Request("total", (3, 4), 1e-6, 0.5), ens.Request("synch", (0, 2), 0.0, 0.3), ens.Request("pion", (3, 4), 1e-3, 0.1, (2, 9))]
    for q, s in zip(reqs, e.summarize(ALL, reqs)):
        first, count = e.word_range(ALL, q.name, q.zones, q.bins)
        assert s == ens.summary_of(mean[first:first + count], m2[first:first + count], 5, q.floor_frac, q.tol) and s.n_selected > 0
    trig = ens.Trigger(ALL, "total", "max", 1.5, zones=(3, 4))
    e.check_trigger(trig)
    assert trig.met(e.summarize(ALL, [trig.request])[0])
    # the all-shells row of the source is the sum over species of their all-shells rows, not the sum of the source's shell rows
    row = off["total"][0] + 3 * 31
    assert bits_equal(got[0][row:row + 31], welford_restated([deposit_restated([x[row:row + 31] for x in samples]) for samples in fed])[0])


def test_refusals_leave_everything_as_it_was():
    prob = make_problem(64)
    e, other = fresh(prob), fresh(prob)
    feed(e, range(2))
    feed(other, range(2), seed=3)
    obs = crafted_species(7)
    e.add_photons(None, 0, obs[0], deposit=True)
    e.add_photons(None, 2, obs[2], deposit=True)
    assert e.pending_photons == (0, 2)
    before = state_of(e)
    with pytest.raises(ValueError, match="has been deposited since the last"):
        e.add_photons(None, 2, obs[2], deposit=True)                      # a double deposit of a species
    with pytest.raises(ValueError, match="no species slot"):
        e.add_photons(None, ALL, obs[1], deposit=True)
    with pytest.raises(ValueError, match="was observed as"):
        e.add_photons(None, 1, cons.ObservedSpectra(("pion",), {"pion": np.ones((3, 11))}, {}, None, None, LAYOUT, 0.1), deposit=True)
    with pytest.raises(ValueError, match="source slot is no species slot"):
        e.load_mean(ALL, None)
    hs = e.photons_slot(0)
    creqs = [ens.CompareRequest("total")]
    with pytest.raises(ValueError, match="source slot with a photons slot"):
        e.compare(other, ALL, creqs, hs)
    with pytest.raises(ValueError, match="photons slot with a source slot"):
        e.compare(other, hs, creqs, ALL)
    with pytest.raises(ValueError, match="comparison of slot"):
        e.compare(e, ALL, creqs)
    with pytest.raises(ValueError, match="stays as it is"):
        e.set_photon_layout(LAYOUT)
    # differing layouts: merge, merged summary, comparison
    odd_layout = cons.PhotonLayout(3, LAYOUT.n, {"synch": 1, "ic": 9, "pion": 20}, 31)
    odd = fresh(prob, odd_layout)
    feed(odd, range(2), layout=odd_layout)
    before_odd = state_of(odd)
    reqs = [ens.Request("total")]
    for call in (lambda: e.merge(odd), lambda: odd.merge(e), lambda: e.summarize_merged([odd], ALL, reqs), lambda: e.compare(odd, ALL, creqs)):
        with pytest.raises(ValueError, match="photon layouts differ"):
            call()
    assert same_state(state_of(e), before) and same_state(state_of(odd), before_odd)
    # a take with nothing pending; a read of a source slot that was never sampled
    never = fresh(prob)
    never.add_photons(None, 1, obs[1])
    before_never = state_of(never)
    with pytest.raises(ValueError, match="no deposit pending"):
        never.add_photons_all()
    with pytest.raises(ValueError, match="source slot has never taken a sample"):
        never.mean(ALL, "total")
    with pytest.raises(ValueError, match="at least two samples"):
        never.summarize(ALL, reqs)
    assert never.count(ALL) == 0 and same_state(state_of(never), before_never)
    e.add_photons_all()
    with pytest.raises(ValueError, match="no deposit pending"):
        e.add_photons_all()
    assert e.count(ALL) == 3 and e.pending_photons == ()
    # the comparison of two source slots is that of their words
    (d,) = e.compare(other, ALL, creqs)
    (ma, qa), (mb, qb) = slot_words(e, ALL), slot_words(other, ALL)
    o, w = LAYOUT.offsets()["total"]
    assert d == ens.difference_of(ma[o:o + 4 * w], qa[o:o + 4 * w], 3, mb[o:o + 4 * w], qb[o:o + 4 * w], 2, 1e-3, 3.0) and d.n_selected > 0


def test_drop_pending_lets_a_species_deposit_again():
    prob = make_problem(64)
    e = fresh(prob)
    assert e.drop_pending_photons() is None and e.pending_photons == ()          # (nothing pending: nothing happens)
    first, second = crafted_species(1), crafted_species(2)
    e.add_photons(None, 0, first[0], deposit=True)
    e.add_photons(None, 1, first[1], deposit=True)
    e.drop_pending_photons()
    assert e.pending_photons == () and e.count(ALL) == 0
    with pytest.raises(ValueError, match="no deposit pending"):
        e.add_photons_all()
    e.add_photons(None, 0, second[0], deposit=True)                              # starts the pending vector anew
    e.add_photons(None, 2, second[2], deposit=True)
    e.add_photons_all()
    mean, m2 = slot_words(e, ALL)
    assert e.count(ALL) == 1 and bits_equal(mean, deposit_restated([second[0].sample(), second[2].sample()])) and not m2.any()
    assert [e.count(e.photons_slot(s)) for s in range(3)] == [2, 1, 1]


def test_merge_is_chans_and_a_destination_without_a_layout_takes_it():
    prob = make_problem(64)
    a, b = fresh(prob), fresh(prob)
    fa, fb = feed(a, range(2)), feed(b, range(2, 5))
    b.add_photons(None, 1, crafted_species(9)[1], deposit=True)                  # pending deposits are not merged and do not hinder
    wa = welford_restated([deposit_restated(s) for s in fa])
    wb = welford_restated([deposit_restated(s) for s in fb])
    reqs = [ens.Request("total", (3, 4), 1e-6, 0.5), ens.Request("synch")]
    merged = a.summarize_merged([b], ALL, reqs)
    into = fresh(prob, None)
    assert into.photon_layout is None and into.count(ALL) == 0
    into.merge(a)
    assert into.photon_layout is LAYOUT and into.count(ALL) == 2 and bits_equal(slot_words(into, ALL)[0], wa[0])
    into.merge(b)
    want = chan_restated(wa, 2, wb, 3)
    got = slot_words(into, ALL)
    assert into.count(ALL) == 5 and bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])
    assert into.pending_photons == () and b.pending_photons == (1,) and [x.count(ALL) for x in (a, b)] == [2, 3]
    assert merged == into.summarize(ALL, reqs) and merged[0].n == 5 and merged[0].n_selected > 0
    for s in range(3):
        assert into.count(into.photons_slot(s)) == 5 + (s == 1)
    # a source slot alone carries the layout over, too
    only = fresh(prob)
    only._slots[ALL] = a._slots[ALL].copy()
    into2 = fresh(prob, None)
    into2.merge(only)
    assert into2.photon_layout is LAYOUT and into2.count(ALL) == 2


def test_an_ensemble_that_never_deposits_is_what_it_was():
    prob = make_problem(64)
    be = oracle_backend(prob)
    L = mcs.capi.Layout(prob.params)
    x_log = ens.bin_centres_log10(prob)
    today, both = ens.HostEnsemble(prob.params, 3), ens.HostEnsemble(prob.params, 3)
    for e in (today, both):
        e.set_photon_layout(LAYOUT)
        e.set_slope_window(10, 50, x_log)
    prev = np.zeros(L.total)
    for k, (f, i) in enumerate(crafted_buffers(L, 3)):
        obs = crafted_species(k)
        for e in (today, both):
            be.write_tallies(prev, i)
            e.begin_iteration(be)
            be.write_tallies(f, i)
            fin = cons.ion_finalize(prob, be, 1)
            for s in range(3):
                e.add_species(be, s)
                e.add_photons(be, s, obs[s], deposit=e is both)
            if e is both:
                e.add_photons_all()
            e.add_products(be, 2, fin)
            e.add_iteration(be)
        prev = f
    assert today.count(ALL) == 0 and ALL not in today._slots and today._pending is None and both.count(ALL) == 3
    slots = [0, 1, 2, 3, today.products_slot(2)] + [today.photons_slot(s) for s in range(3)]
    for slot in slots:
        n = today._len(slot)
        assert today.count(slot) == both.count(slot) == 3, slot
        for what in (0, 1):
            a, b = today._read(slot, what, 0, n), both._read(slot, what, 0, n)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (slot, what)
    be.destroy()


# ---- driver.run(photons=, ensemble=) on the oracle backend -----------------------------------------------------------------------------
ME_MP = mcs.constants.ME / mcs.constants.MP
SETUP = cons.PhotonSetup(3, 3, jet_dist_kpc=1.0e3)


def electron_problem(N=300):
    return make_problem(N, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(ME_MP, -1.0, 1e6, 1.0)], radiation_losses=True,
                        B_mag_upstream=3e-3, JETFR=(0.0, 20.0), num_iterations=4)


def test_driver_takes_one_source_sample_per_iteration():
    prob = electron_problem(300)
    be = oracle_backend(prob, nthreads=8)
    run = mcs.driver.run
    e = ens.Ensemble.for_backend(be, 2)
    state, fed = None, []
    for it in (1, 2, 3):
        r = run(prob, be, n_itrs=1, first_iter=it, iter_state=state, max_pcuts=8, finalize=True, photons=SETUP, ensemble=e)
        state = r.iter_state
        fed.append([r.photons[s].sample() for s in (0, 1)])
        assert e.pending_photons == () and e.count(ALL) == it
    n = e.photon_layout.offsets()["_total"]
    mean, m2 = welford_restated([deposit_restated(samples) for samples in fed])
    got = slot_words(e, ALL, n)
    assert bits_equal(got[0], mean) and bits_equal(got[1], m2)
    for s in (0, 1):
        want = welford_restated([samples[s] for samples in fed])
        a = slot_words(e, e.photons_slot(s), n)
        assert e.count(e.photons_slot(s)) == 3 and bits_equal(a[0], want[0]) and bits_equal(a[1], want[1]), s
    rows = e.photon_layout.rows
    all_shells = e.mean(ALL, "total")[rows - 1]
    print("lit words of the mean all-shells total of the source:", int((all_shells > 1e-98).sum()), "; largest M2:", e.m2(ALL, "total")[rows - 1].max())
    assert (all_shells > 1e-98).sum() > 0 and e.m2(ALL, "total")[rows - 1].max() > 0
    assert e.count(e.products_slot(1)) == 3 and e.count(2) == 3
    # the stop rule on the source slot.  Samples are not negative, so a relative standard error is at most 1: 1.5 is met by whatever is
    # selected; 1e-15 is not met by Monte-Carlo spectra that differ from iteration to iteration
    e2 = ens.Ensemble.for_backend(be, 2)
    met = ens.Trigger(ALL, "total", "max", 1.5, zones=(rows - 1, rows))
    unmet = ens.Trigger(ALL, "total", "max", 1e-15, zones=(rows - 1, rows))
    with pytest.raises(ValueError, match="source slot needs photons="):
        run(prob, be, n_itrs=2, max_pcuts=1, finalize=True, ensemble=e2, triggers=[met])
    assert e2.count(0) == 0 and e2.count(ALL) == 0
    res = run(prob, be, n_itrs=2, max_pcuts=8, finalize=True, photons=SETUP, ensemble=e2, triggers=[met, unmet])
    c = res.convergence
    assert e2.count(ALL) == 2 and not c.satisfied and c.stopped_at == 2 and [it for it, _ in c.checks] == [2]
    (row_met, row_unmet), = [rows_ for _, rows_ in c.checks]
    assert row_met.met and not row_unmet.met and row_met.summary.n == 2 and row_met.summary.n_selected > 0
    assert 1e-15 < row_unmet.value <= 1.5
    alone = run(prob, be, n_itrs=2, max_pcuts=8, finalize=True, photons=SETUP, ensemble=e2, triggers=[met])
    assert alone.convergence.satisfied and alone.convergence.stopped_at == 2 and e2.count(ALL) == 4
    be.destroy()
