"""The observed shell spectra on the host (consumers.shell_spectra_host, observed_spectra, the photons slot of ensemble.HostEnsemble and
driver.run(photons=)): the numpy statement of include/mcs.h "observed shell spectra" against `summed_emission`, which it restates per
process, and against a serial restatement in Python floats; the sample vector and its statistics against plain numpy.  Equal bits
everywhere: the device (tests/test_gpu_photon_observed.py) is held to the same."""
import math
import types

import numpy as np
import pytest

from conftest import mcs, make_problem, oracle_backend
from photon_observed_common import BETAS, bits_equal, crafted_emis, flux_classes, serial_restatement, tables

cons = mcs.consumers
ens = mcs.ensemble


def _fake_prob(n_grid, gam=None, beta=None):
    P = types.SimpleNamespace(n_grid=n_grid)
    g = np.ones(n_grid + 2) if gam is None else np.concatenate([[1.0], gam, [1.0]])
    b = np.zeros(n_grid + 2) if beta is None else np.concatenate([[0.0], beta, [0.0]])
    return types.SimpleNamespace(params=P, gam_ef=g, beta_ef=b)


def _summed_inputs(ng=12):
    """The inputs of test_summed_emission_layout_and_sums: lines of the three processes in zones 3, 5, 8 and 10 of 12."""
    n = {p: cons.photon_n_photon(p) for p in cons.PHOTON_PROCESSES}
    E = {p: cons.photon_e_min(p) * 10.0 ** (np.arange(n[p]) / 10) for p in cons.PHOTON_PROCESSES}
    f = {p: np.full((ng, n[p]), 1e-99) for p in cons.PHOTON_PROCESSES}
    f["pion"][2, 20] = 3e-7; f["pion"][7, 20] = 1e-7; f["pion"][7, 50] = 5e-9
    f["synch"][4, 100] = 2e-5
    f["ic"][9, 30] = 4e-8; f["ic"][9, 60] = 4e-10
    f["ic"][7, int(round((math.log10(E["pion"][20]) + 2) * 10))] = 2e-7            # an IC line at the pion line's energy, zone 8
    return E, f


@pytest.mark.parametrize("moving", [False, True])
def test_host_function_is_summed_emission(moving):
    ng = 12
    E, f = _summed_inputs(ng)
    ends = np.array([1, 4, 9, 13])
    rng = np.random.default_rng(1)
    beta = rng.choice(BETAS[1:], ng) if moving else np.zeros(ng)
    gam = 1.0 / np.sqrt(1.0 - beta * beta)
    prob = _fake_prob(ng, gam, beta)
    se = cons.summed_emission(prob, ends, pion=cons.PhotonPion(E["pion"], None, None, f["pion"], None, 1), synch=cons.PhotonSynch(E["synch"], None, None, f["synch"]),
                              ic=cons.PhotonIC(E["ic"], None, None, f["ic"], None))
    dlog = 0.1
    per = {}
    for p in cons.PHOTON_PROCESSES:
        sh = cons.shell_spectra_host(p, None, None, E[p], None, dlog, 10.0 ** dlog, np.linspace(-1.0, 1.0, 181), gam, beta, gam ** 3, ends, flux=f[p])
        assert sh.shape == (4, len(E[p]) - 1)
        want = se.per_process[p][1]
        got = np.where(sh[:3] > 1.0e-99, np.log10(np.maximum(sh[:3], 1e-300) / dlog), -99.0)
        assert bits_equal(got, want), p
        assert (want > -99).sum() >= (3 if p != "synch" else 1)
        per[p] = sh
    layout = cons.stock_photon_layout(3)
    assert layout.args() == (3, 179, 139, 119, 0, 110, 130, 250)
    tot = cons.photon_total(per, layout)
    back = lambda a: np.where(a > 1.0e-96, np.log10(np.maximum(a, 1e-300) / dlog), -99.0)
    assert bits_equal(back(tot[:3]), se.per_shell) and bits_equal(back(tot[3]), se.total)
    assert (se.per_shell > -99).sum() >= 6
    # the all-shell row of a process is the sum of its shells' lit words
    for p, sh in per.items():
        lit = np.where(sh[:3] > 1.0e-99, sh[:3], 0.0)
        assert bits_equal(sh[3], np.maximum((lit[0] + lit[1]) + lit[2], 1.0e-99)), p


@pytest.mark.parametrize("process", cons.PHOTON_PROCESSES)
def test_host_function_is_the_serial_restatement(process):
    ng, n_photon = 3, 25                     # 24 bins
    for betas, ends in (((0.0, 0.6, math.sqrt(24.0 / 25.0)), (1, 3, 4)), ((0.9, 0.3, 0.0), (0, 2, 2, 4)), ((0.6, 0.6, 0.9), (1, 4))):
        tabs = tables(process, ng, n_photon, betas, ends)
        emis = crafted_emis(process, 6, n_photon, tabs)[[2, 4, 5]]          # dense, sub-1e-90 beside a line, the lowest bins
        floor, low, lit = flux_classes(process, emis, tabs)
        assert floor > 0 and low == 1 and lit > 24
        got = cons.shell_spectra_host(process, emis, **tabs)
        want = serial_restatement(process, emis, **tabs)
        assert got.shape == (len(ends), 24) and bits_equal(got, want), (process, betas)
        assert (got[-1] > 1.0e-99).sum() >= 3               # (every layout has the two line zones in a shell)


# ---- the photons slot of the numpy ensemble -------------------------------------------------------------------------------------
def crafted_observations(layout, k, seed=0):
    """k ObservedSpectra on `layout`: positive words over forty decades, one word in five on the floor in all of them; the even ones
    observe synch + ic, the odd ones pion alone."""
    common = np.random.default_rng(seed + 100)
    out = []
    for i in range(k):
        rng = np.random.default_rng(seed + i)
        per = {}
        for p in (("synch", "ic") if i % 2 == 0 else ("pion",)):
            shape = (layout.rows, layout.n[p])
            a = rng.uniform(1, 10, shape) * 10.0 ** rng.integers(-30, 10, shape)
            a[np.random.default_rng(seed + 100 + len(p)).random(shape) < 0.2] = 1e-99
            per[p] = a
        out.append(cons.ObservedSpectra(tuple(per), per, {}, cons.photon_total(per, layout), None, layout, 0.1))
    return out


def total_restated(per, layout):
    """The total section from the statement in include/mcs.h, word by word in Python floats."""
    ns = layout.n_shells
    tot = np.empty((ns + 1, layout.n_pts))
    for t in range(layout.n_pts):
        col = 0.0
        for s in range(ns):
            x = 1.0e-99
            for p in ("pion", "synch", "ic"):
                if p in per and layout.start[p] <= t < layout.start[p] + layout.n[p]:
                    v = float(per[p][s, t - layout.start[p]])
                    x = x + (v if v > 1.0e-99 else 0.0)
            tot[s, t] = x
            col = col + x
        tot[ns, t] = col
    return tot


def small_layout():
    return cons.PhotonLayout(3, {"synch": 23, "ic": 17, "pion": 11}, {"synch": 0, "ic": 9, "pion": 20}, 31)


def test_host_ensemble_photons_slot():
    prob = make_problem(64)
    lay = small_layout()
    e = ens.HostEnsemble(prob.params, 2)
    hs = e.photons_slot(1)
    assert hs == 1 | (1 << 29) and e.is_photons(hs) and not e.is_products(hs) and not e.is_photons(e.products_slot(1)) and e._kind(hs) == "photons"
    assert e.names(hs) == ens.PHOTON_NAMES == ("synch", "ic", "pion", "total")
    with pytest.raises(ValueError, match="no photon layout"):
        e.add_photons(None, 1, crafted_observations(lay, 1)[0])
    with pytest.raises(ValueError, match="no layout yet"):
        e.word_range(hs, "total")
    with pytest.raises(ValueError, match="energy words inside the common grid"):
        e.set_photon_layout(cons.PhotonLayout(3, {"synch": 23, "ic": 17, "pion": 12}, {"synch": 0, "ic": 9, "pion": 20}, 31))
    e.set_photon_layout(cons.PhotonLayout(2, lay.n, lay.start, 40))      # (may be called again until the first sample)
    e.set_photon_layout(lay)
    obs = crafted_observations(lay, 5)
    for o in obs:
        e.add_photons(None, 1, o)
    assert e.count(hs) == 5 and e.count(e.photons_slot(0)) == 0 and e.count(1) == 0
    with pytest.raises(ValueError, match="stays as it is"):
        e.set_photon_layout(lay)
    # the update is welford_update's on the stated sample vector; an absent process reads 1e-99; the total is its restatement
    samples = []
    for o in obs:
        parts = [o.per_process[p] if p in o.per_process else np.full((lay.rows, lay.n[p]), 1e-99) for p in cons.PHOTON_PROCESSES]
        tot = total_restated(o.per_process, lay)
        assert bits_equal(tot, o.total)
        samples.append(np.concatenate([a.ravel() for a in parts] + [tot.ravel()]))
    mean, m2, n = np.zeros_like(samples[0]), np.zeros_like(samples[0]), 0
    for x in samples:
        n = ens.welford_update(mean, m2, n, x)
    off = lay.offsets()
    assert off["_total"] == mean.size == 4 * (23 + 17 + 11 + 31)
    for name in ens.PHOTON_NAMES:
        o, w = off[name]
        assert bits_equal(e.mean(hs, name), mean[o:o + 4 * w].reshape(4, w)) and bits_equal(e.m2(hs, name), m2[o:o + 4 * w].reshape(4, w)), name
    assert bits_equal(e.stderr(hs, "total"), np.sqrt(m2[off["total"][0]:] / 20.0).reshape(4, 31))
    # word ranges: zones = shell rows, bins = an energy window of one row
    assert e.word_range(hs, "synch") == (0, 4 * 23) and e.word_range(hs, "ic", (1, 3)) == (4 * 23 + 17, 2 * 17)
    assert e.word_range(hs, "total", (3, 4), (5, 12)) == (off["total"][0] + 3 * 31 + 5, 7)
    with pytest.raises(ValueError, match="outside"):
        e.word_range(hs, "pion", (0, 5))
    with pytest.raises(KeyError):
        e.word_range(hs, "psd")
    with pytest.raises(KeyError):
        e.word_range(0, "total")
    # a summary, a trigger and a comparison on the slot, against plain numpy
    reqs = [ens.Request("total", (3, 4), 1e-6, 0.5, (5, 25)), ens.Request("synch", (0, 2), 0.0, 0.3), ens.Request("pion")]
    for q, s in zip(reqs, e.summarize(hs, reqs)):
        first, count = e.word_range(hs, q.name, q.zones, q.bins)
        assert s == ens.summary_of(mean[first:first + count], m2[first:first + count], 5, q.floor_frac, q.tol) and s.n_selected > 0
    trig = ens.Trigger(hs, "total", "max", 10.0, zones=(3, 4), bins=(5, 25), floor_frac=1e-6)
    e.check_trigger(trig)
    (s,) = e.summarize(hs, [trig.request])
    first, count = e.word_range(hs, "total", (3, 4), (5, 25))
    a = np.abs(mean[first:first + count])
    rel = np.sqrt(m2[first:first + count] / 20.0) / a
    sel = a >= 1e-6 * a.max()
    assert trig.value(s) == rel[sel].max() and trig.met(s) and not ens.Trigger(hs, "total", "max", rel[sel].max() / 2, zones=(3, 4), bins=(5, 25), floor_frac=1e-6).met(s)
    other = ens.HostEnsemble(prob.params, 2)
    other.set_photon_layout(lay)
    for o in crafted_observations(lay, 4, seed=50):
        other.add_photons(None, 0, o)
    mb, qb = (other._read(other.photons_slot(0), what, 0, mean.size) for what in (0, 1))
    creqs = [ens.CompareRequest("total", (0, 3), 1e-9, 2.0), ens.CompareRequest("ic", (3, 4), 0.0, 1.0, (2, 15))]
    for q, d in zip(creqs, e.compare(other, hs, creqs, other.photons_slot(0))):
        first, count = e.word_range(hs, q.name, q.zones, q.bins)
        sl = slice(first, first + count)
        assert d == ens.difference_of(mean[sl], m2[sl], 5, mb[sl], qb[sl], 4, q.floor_frac, q.zcut) and d.n_selected > 0
    (row,) = ens.check_agreements(e, other, [ens.Agreement(hs, "total", "max_z", 1e6, other_slot=other.photons_slot(0))])
    assert row.met and row.difference.n_a == 5 and row.difference.n_b == 4
    with pytest.raises(ValueError, match="photons slot with a products slot|products slot with a photons slot"):
        e.compare(other, hs, creqs, other.products_slot(0))
    # merge: Chan's, allocating in the destination; other layouts are refused
    into = ens.HostEnsemble(prob.params, 2)
    into.merge(e)
    assert into.count(hs) == 5 and into.photon_layout is lay and bits_equal(into.mean(hs, "total"), e.mean(hs, "total"))
    more = ens.HostEnsemble(prob.params, 2)
    more.set_photon_layout(lay)
    for o in crafted_observations(lay, 3, seed=9):
        more.add_photons(None, 1, o)
    got = e.summarize_merged([more], hs, reqs)
    into.merge(more)
    assert into.count(hs) == 8 and got == into.summarize(hs, reqs)
    odd = ens.HostEnsemble(prob.params, 2)
    odd.set_photon_layout(cons.PhotonLayout(3, lay.n, lay.start, 32))
    for call in (lambda: e.merge(odd), lambda: e.summarize_merged([odd], hs, reqs), lambda: odd.merge(e)):
        with pytest.raises(ValueError, match="photon layouts differ"):
            call()
    with pytest.raises(ValueError, match="never taken a sample"):
        odd.mean(hs, "total")
    with pytest.raises(ValueError, match="was observed as"):
        odd.add_photons(None, 0, cons.ObservedSpectra(("pion",), {"pion": np.ones((3, 11))}, {}, None, None, lay, 0.1))


def test_library_exports_the_new_calls():
    lib = mcs.capi.load_library()
    for name in ("mcs_photon_observe", "mcs_ens_photons_get_layout", "mcs_ens_set_photon_layout", "mcs_ens_add_photons"):
        assert hasattr(lib, name) and name in mcs.capi.EXPORTED_SYMBOLS, name
    out = mcs.capi.McsEnsPhotonsLayout()
    lay = cons.stock_photon_layout(6)
    a = lay.args()
    assert lib.mcs_ens_photons_get_layout(a[0], a[1], a[2], a[3], a[7], out) == 0
    off = lay.offsets()
    assert (out.synch, out.ic, out.pion, out.total_section, out.total) == (off["synch"][0], off["ic"][0], off["pion"][0], off["total"][0], off["_total"])
    assert (out.n_synch, out.n_ic, out.n_pion, out.n_pts, out.rows) == (179, 139, 119, 250, 7)
    assert lib.mcs_ens_photons_get_layout(0, 179, 139, 119, 250, out) != 0 and b"n_shells" in lib.mcs_last_error()


# ---- driver.run(photons=) on the oracle backend --------------------------------------------------------------------------------------
ME_MP = mcs.constants.ME / mcs.constants.MP
N_PCUTS = 8


def electron_problem(N=300):
    return make_problem(N, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(ME_MP, -1.0, 1e6, 1.0)], radiation_losses=True,
                        B_mag_upstream=3e-3, JETFR=(0.0, 20.0), num_iterations=4)


SETUP = cons.PhotonSetup(3, 3, jet_dist_kpc=1.0e3)


def test_driver_refusals():
    prob = electron_problem(64)
    be, be2 = oracle_backend(prob), oracle_backend(prob)
    e = ens.Ensemble.for_backend(be, 2)
    trig = ens.Trigger(e.photons_slot(0), "total", "max", 1.0)
    run = mcs.driver.run
    with pytest.raises(ValueError, match="photons slot needs photons="):
        run(prob, be, n_itrs=2, max_pcuts=1, finalize=True, ensemble=e, triggers=[trig])
    with pytest.raises(ValueError, match="photons: not with species_backends"):
        run(prob, be, n_itrs=1, max_pcuts=1, finalize=True, photons=SETUP, species_backends=[be2])
    with pytest.raises(ValueError, match="photons: needs finalize"):
        run(prob, be, n_itrs=1, max_pcuts=1, photons=SETUP)
    comm = mcs.driver.Comm(False); comm.enabled = True
    with pytest.raises(ValueError, match="photons: one process without a communicator"):
        run(prob, be, comm=comm, n_itrs=1, max_pcuts=1, finalize=True, photons=SETUP)
    assert e.count(e.photons_slot(0)) == 0 and e.count(0) == 0
    be.destroy(); be2.destroy()


def test_driver_feeds_the_photons_slots():
    prob = electron_problem(300)
    be = oracle_backend(prob, nthreads=8)
    e = ens.Ensemble.for_backend(be, 2)
    res = mcs.driver.run(prob, be, n_itrs=2, max_pcuts=N_PCUTS, finalize=True, photons=SETUP, ensemble=e)
    assert e.photon_layout.args() == (6, 179, 139, 119, 0, 110, 130, 250)
    assert [e.count(e.photons_slot(s)) for s in (0, 1)] == [2, 2] and e.count(e.products_slot(1)) == 2 and e.count(e.products_slot(0)) == 0
    assert len(res.photons) == 2 and res.photons[0].processes == ("pion",) and res.photons[1].processes == ("synch", "ic")
    assert res.photons[1].per_process["synch"].shape == (7, 179) and res.photons[0].total.shape == (7, 250)
    assert bits_equal(res.photons[0].per_dlog().total, res.photons[0].total / 0.1)
    # by hand: every species end's tallies on a second context, ion_finalize, the folds, the host function, the sample; then the mean
    be2 = oracle_backend(prob, nthreads=8)
    by_hand = {0: [], 1: []}
    _, zones = cons.photon_shells(prob, 3, 3)
    kw = dict(jet_dist_kpc=SETUP.jet_dist_kpc, redshift=SETUP.redshift)
    back = lambda a: np.where(a > 1.0e-96, np.log10(np.maximum(a, 1e-300) / 0.1), -99.0)
    lit_chain = 0
    for i_iter, i_ion, f, i in res.per_species:
        be2.write_tallies(f, i)
        fin = cons.ion_finalize(prob, be2, i_ion)
        obs = cons.observed_spectra(prob, be2, i_ion, SETUP, fin)
        by_hand[i_ion - 1].append(obs)
        # the whole chain from the emission -- step 1, the flux at Earth, included -- against the existing host path: the conversions
        # of photon_pion / photon_synch / photon_ic and summed_emission on their photon fluxes
        folds = dict(pion=cons.photon_pion(prob, be2, fin, i_ion, **kw)) if i_ion == 1 else dict(
            synch=cons.photon_synch(prob, be2, fin, i_ion, **kw), ic=cons.photon_ic(prob, be2, i_ion, **kw))
        se = cons.summed_emission(prob, zones, **folds)
        for p, ph in folds.items():
            emis = ph.emis_erg if p == "ic" else ph.emis_erg_s
            tabs = cons.observe_tables(prob, SETUP, p, ph.energy_MeV)
            flux = cons.photon_flux_host(p, emis, ph.energy_erg if p == "pion" else tabs["energy_div"], tabs["area"])
            assert bits_equal(flux, ph.photon_flux), (i_ion, p)
            sh = obs.per_process[p]
            assert bits_equal(np.where(sh[:6] > 1.0e-99, np.log10(np.maximum(sh[:6], 1e-300) / 0.1), -99.0), se.per_process[p][1]), (i_ion, p)
            lit_chain += int((se.per_process[p][1] > -99).sum())
        assert bits_equal(back(obs.total[:6]), se.per_shell) and bits_equal(back(obs.total[6]), se.total), i_ion
    print("lit words of the chain against summed_emission:", lit_chain)
    assert lit_chain > 0
    lit = 0
    for s in (0, 1):
        assert bits_equal(by_hand[s][1].sample(), res.photons[s].sample())
        mean, m2, n = np.zeros(e.photon_layout.offsets()["_total"]), np.zeros(e.photon_layout.offsets()["_total"]), 0
        for obs in by_hand[s]:
            n = ens.welford_update(mean, m2, n, obs.sample())
        off = e.photon_layout.offsets()
        for name in ens.PHOTON_NAMES:
            o, w = off[name]
            assert bits_equal(e.mean(e.photons_slot(s), name), mean[o:o + 7 * w].reshape(7, w)), (s, name)
            assert bits_equal(e.m2(e.photons_slot(s), name), m2[o:o + 7 * w].reshape(7, w)), (s, name)
        lit += int((mean > 1e-99).sum())
    print("lit words of the two means:", lit)
    assert lit > 0
    # the last species' ion_finalize is the one finalize used
    assert bits_equal(res.iter_finals[-1][2].dNdp_cr, cons.ion_finalize(prob, be2, 2).dNdp_cr)
    be.destroy(); be2.destroy()
