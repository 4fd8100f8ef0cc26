"""Ensemble statistics without a GPU: the numpy accumulator (ensemble.HostEnsemble) against the restatement of
ensemble_common.py bit for bit, the layout of the sample vectors, the exported symbols, and driver.run(ensemble=...) through the
CPU oracle."""
import ctypes as ct
import types

import numpy as np
import pytest

from conftest import mcs, make_problem, oracle_backend
from ensemble_common import (AS_IS, HISTS, INCREMENTS, SPECIES_TALLIES, assert_tail_is_exercised, bits_equal, check_one_merge_of_every_kind,
                             crafted_buffers, iteration_parts, species_parts, stat_of)
from photons_all_common import SMALL_LAYOUT, SMALL_PROCESSES, crafted_species

ens = mcs.ensemble


class _Buffers:
    """The least a backend is to the host accumulator: the parameters and a tally buffer to read and write."""

    def __init__(self, prob):
        self.P = prob.params
        self.layout = mcs.capi.Layout(self.P)
        self.f, self.i = np.zeros(self.layout.total), np.zeros(self.layout.n_i64, dtype=np.int64)

    def read_tallies(self):
        return self.f.copy(), self.i.copy()

    def write_tallies(self, f, i):
        self.f, self.i = np.array(f, dtype=np.float64), np.array(i, dtype=np.int64)


@pytest.fixture(scope="module")
def crafted():
    prob = make_problem(64)
    L = mcs.capi.Layout(prob.params)
    bufs = crafted_buffers(L)
    return prob, L, bufs, [species_parts(L, f, i) for f, i in bufs]


def _assert_slot(e, slot, want, names, what=""):
    assert e.count(slot) == want.n, what
    for name in names:
        assert bits_equal(e.mean(slot, name), want.mean[name]), f"{what} mean of {name}"
        assert bits_equal(e.m2(slot, name), want.m2[name]), f"{what} M2 of {name}"


def test_host_ensemble_equals_the_restatement(crafted):
    prob, L, bufs, parts = crafted
    be = _Buffers(prob)
    e = ens.HostEnsemble(prob.params, 2)
    assert set(e.names(0)) == set(parts[0]) and e.names(2) == INCREMENTS + AS_IS
    for f, i in bufs:
        be.write_tallies(f, i)
        e.add_species(be, 1)
    want = stat_of(parts)
    _assert_slot(e, 1, want, parts[0])
    assert e.count(0) == 0 and e.count(2) == 0
    floor = np.arange(0, L.offsets["esc_flux"], 7)
    mean1 = np.concatenate([e.mean(1, n).ravel() for n in SPECIES_TALLIES])
    m21 = np.concatenate([e.m2(1, n).ravel() for n in SPECIES_TALLIES])
    assert np.all(mean1[floor] == 1e-99) and not np.any(m21[floor])
    for name in parts[0]:
        assert bits_equal(e.stderr(1, name), np.sqrt(want.m2[name] / 20.0)), name
    assert e.mean(1, "psd_mom").shape == (prob.params.n_grid, prob.params.num_psd_mom_bins + 2)
    assert e.mean(1, "therm_pf_tht").shape == (prob.params.n_grid, prob.params.num_psd_tht_bins + 2)
    # the iteration slot: the never-reset sections as growth since begin_iteration, the rest as it stands
    prev = np.zeros(L.total)
    it_parts = []
    for f, i in bufs:
        be.write_tallies(prev, i)
        e.begin_iteration(be)
        be.write_tallies(f, i)
        e.add_iteration(be)
        it_parts.append(iteration_parts(L, f, prev))
        prev = f
    _assert_slot(e, 2, stat_of(it_parts), INCREMENTS + AS_IS, "iteration slot:")
    # merge: samples 1-3 and 4-5 on two accumulators
    a, b = ens.HostEnsemble(prob.params, 2), ens.HostEnsemble(prob.params, 2)
    for k, (f, i) in enumerate(bufs):
        be.write_tallies(f, i)
        (a if k < 3 else b).add_species(be, 1)
    a.merge(b)
    _assert_slot(a, 1, stat_of(parts[:3]).merged_with(stat_of(parts[3:])), parts[0], "merged:")
    _assert_slot(b, 1, stat_of(parts[3:]), parts[0], "the source of a merge is unchanged:")
    empty = ens.HostEnsemble(prob.params, 2)
    empty.merge(b); b.merge(ens.HostEnsemble(prob.params, 2))
    _assert_slot(empty, 1, stat_of(parts[3:]), parts[0], "an empty slot takes the source as it is:")
    _assert_slot(b, 1, stat_of(parts[3:]), parts[0], "an empty source changes nothing:")
    # load_mean: parts 1 - 3 of the mean into the per-species sections, the rest of the buffers untouched
    be.write_tallies(*bufs[0])
    e.load_mean(1, be)
    f, i = be.read_tallies()
    for name in SPECIES_TALLIES + ("energy_recv_pool",):
        assert bits_equal(L.view(f, name), want.mean[name]), name
    assert np.array_equal(i[:L.n_grid], np.rint(want.mean["num_crossings"]).astype(np.int64))
    for name in mcs.capi.RUNNING_F64:
        assert bits_equal(L.view(f, name), L.view(bufs[0][0], name)), name
    assert np.array_equal(i[L.n_grid:], bufs[0][1][L.n_grid:])
    # refusals
    with pytest.raises(ValueError):
        e.add_species(be, 2)
    with pytest.raises(ValueError):
        e.add_iteration(be)                      # no begin_iteration since the last sample
    with pytest.raises(ValueError):
        ens.HostEnsemble(prob.params, 1).stderr(0, "psd")
    with pytest.raises(KeyError):
        e.mean(1, "spectra_sf")
    with pytest.raises(KeyError):
        e.mean(2, "px_esc_feb")                  # indexed by iteration: not exposed


def test_one_merge_sends_every_kind_through(crafted):
    """Two ensembles of two species slots with samples in slot 0, the iteration slot, products_slot(0), photons_slot(0) and the source
    slot -- two on one side, three on the other -- and in photons_slot(1) of the second alone: one merge call, every kind."""
    prob, L, bufs, parts = crafted
    be = oracle_backend(prob)
    x_log = ens.bin_centres_log10(prob)
    ng, nm = prob.params.n_grid, prob.params.num_psd_mom_bins + 2

    def products_of(k):      # (what add_products reads of an IonFinal; the merge does not care where a sample came from)
        rng = np.random.default_rng(500 + k)
        dndp = np.where(rng.random((3, ng, nm)) < 0.8, 10.0 ** rng.uniform(-30, 5, (3, ng, nm)), 1e-99)
        return types.SimpleNamespace(dNdp_cr=dndp, P_psd_par=rng.uniform(1, 2, ng), P_psd_perp=rng.uniform(1, 2, ng), energy_density_psd=rng.uniform(1, 2, ng))

    a, b = ens.HostEnsemble(prob.params, 2), ens.HostEnsemble(prob.params, 2)
    for e, ks in ((a, (1, 2)), (b, (3, 4, 0))):
        e.set_slope_window(0, prob.params.num_psd_mom_bins + 1, x_log)
        e.set_photon_layout(SMALL_LAYOUT)
        for k in ks:
            f, i = bufs[k]
            obs = crafted_species(k, 0, SMALL_LAYOUT, SMALL_PROCESSES)
            be.write_tallies(bufs[k - 1][0], i)
            e.begin_iteration(be)
            be.write_tallies(f, i)
            e.add_species(be, 0)
            e.add_products(be, 0, products_of(k))
            e.add_photons(None, 0, obs[0], deposit=True)
            if e is b:
                e.add_photons(None, 1, obs[1])
            e.add_photons_all()
            e.add_iteration(be)
    slots = [0, a.iteration_slot, a.products_slot(0), a.photons_slot(0), a.photons_slot(1), a.photons_all_slot]
    assert [a._kind(s) for s in slots] == ["species", "iteration", "products", "photons", "photons", "source"]
    check_one_merge_of_every_kind(a, b, {s: b._len(s) for s in slots}, only_b=[b.photons_slot(1)])
    assert a.count(1) == 0 and a.count(a.products_slot(1)) == 0 and a.pending_photons == () and b.pending_photons == ()
    be.destroy()


def test_layout_agrees_with_the_library_and_the_tally_layout():
    lib = mcs.capi.load_library()
    for kw in ({}, dict(num_iterations=3, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(4.0, 2.0, 1e6, 0.1)])):
        prob = make_problem(64, **kw)
        P = prob.params
        E = mcs.capi.McsEnsLayout()
        assert lib.mcs_ens_get_layout(ct.byref(P), ct.byref(E)) == 0
        got = {name: int(getattr(E, name)) for name, _ in E._fields_}
        mirror = ens.EnsLayout(P)
        assert got == mirror.fields
        raw = (ct.c_int64 * 24)()
        assert lib.mcs_get_layout(ct.byref(P), raw) == 0
        psd, esc_flux, recv, scalars, total = raw[0], raw[8], raw[18], raw[19], raw[20]
        ng, nm, nt = P.n_grid, P.num_psd_mom_bins + 2, P.num_psd_tht_bins + 2
        assert (got["tally_sp_first"], got["tally_it_first"], got["tally_recv_pool"], got["tally_scalars"]) == (psd, esc_flux, recv, scalars)
        assert got["sp_tallies_n"] == esc_flux - psd and got["it_sums_n"] == recv - esc_flux and got["it_scalars_n"] == total - scalars == 4
        assert got["sp_total"] == (esc_flux - psd) + 2 * ng + 3 * ng * (nm + nt) and got["it_total"] == (recv - esc_flux) + 4
        assert (got["sp_marg_mom_n"], got["sp_marg_tht_n"]) == (ng * nm, ng * nt)
        order = ["sp_tallies", "sp_recv_pool", "sp_num_crossings", "sp_psd_mom", "sp_psd_tht", "sp_therm_sf_mom", "sp_therm_sf_tht",
                 "sp_therm_pf_mom", "sp_therm_pf_tht", "sp_total"]
        sizes = [esc_flux - psd, ng, ng, ng * nm, ng * nt, ng * nm, ng * nt, ng * nm, ng * nt]
        assert [got[b] - got[a] for a, b in zip(order, order[1:])] == sizes and got["sp_tallies"] == 0
        L = mcs.capi.Layout(P)
        for name in SPECIES_TALLIES:
            assert mirror.species[name] == (L.offsets[name] - psd, L.shapes[name])
        for h in HISTS:
            assert mirror.species[h + "_mom"] == (got[f"sp_{h}_mom"], (ng, nm)) and mirror.species[h + "_tht"] == (got[f"sp_{h}_tht"], (ng, nt))
        for name in INCREMENTS + AS_IS[:2]:
            assert mirror.iteration[name] == (L.offsets[name] - esc_flux, L.shapes[name])
        assert mirror.iteration["scalars"] == (got["it_scalars"], (4,))
    assert_tail_is_exercised(got)
    assert lib.mcs_ens_get_layout(None, ct.byref(E)) != 0 and b"mcs_ens_get_layout" in lib.mcs_last_error()


def test_symbols_are_exported_and_create_needs_a_context():
    lib = mcs.capi.load_library()
    names = ["mcs_ens_get_layout", "mcs_ens_create", "mcs_ens_destroy", "mcs_ens_begin_iteration", "mcs_ens_add_species",
             "mcs_ens_add_iteration", "mcs_ens_merge", "mcs_ens_count", "mcs_ens_read", "mcs_ens_load_mean"]
    for name in names:
        assert hasattr(lib, name) and name in mcs.capi.EXPORTED_SYMBOLS, name
    h = ct.c_void_p(None)
    assert lib.mcs_ens_create(None, 1, ct.byref(h)) != 0 and not h.value
    assert b"mcs_ens_create" in lib.mcs_last_error()
    for call in (lambda: lib.mcs_ens_add_species(None, None, 0), lambda: lib.mcs_ens_merge(None, None),
                 lambda: lib.mcs_ens_read(None, 0, 0, 0, 0, None), lambda: lib.mcs_ens_count(None, 0, None)):
        assert call() != 0 and b"null argument" in lib.mcs_last_error()
    assert lib.mcs_ens_destroy(None) == 0


# max_pcuts = 4: nothing ends within four pcuts, so the never-reset sections stay empty; with every pcut they grow
@pytest.fixture(scope="module", params=[4, None], ids=["4pcuts", "all_pcuts"])
def oracle_run(request):
    n_itrs = 3
    prob = make_problem(300, num_iterations=n_itrs)
    be = oracle_backend(prob, nthreads=8)
    L = be.layout
    e = ens.Ensemble.for_backend(be, 1)
    assert isinstance(e, ens.HostEnsemble)
    ends, iters = [], [be.read_tallies()[0]]
    res = mcs.driver.run(prob, be, n_itrs=n_itrs, max_pcuts=request.param, ensemble=e,
                         on_species_end=lambda it, ion, f, i: ends.append((f.copy(), i.copy())),
                         on_iteration_end=lambda it: iters.append(be.read_tallies()[0]))
    yield prob, be, L, e, res, ends, iters, request.param
    be.destroy()


def test_driver_run_feeds_the_ensemble(oracle_run):
    prob, be, L, e, res, ends, iters, max_pcuts = oracle_run
    assert res.ensemble is e and len(ends) == 3 and len(iters) == 4
    assert e.count(0) == 3 and e.count(1) == 3
    sp = [species_parts(L, f, i) for f, i in ends]
    want = stat_of(sp)
    assert want.mean["therm_sf"].max() > 0 and want.m2["therm_sf"].max() > 0      # (the runs differ: the keys carry the iteration)
    _assert_slot(e, 0, want, sp[0], "species slot:")
    it = [iteration_parts(L, iters[k + 1], iters[k]) for k in range(3)]
    want_it = stat_of(it)
    if max_pcuts is None:
        assert want_it.m2["spectra_coupled"].max() > 0 and want_it.m2["esc_num_eff"].max() > 0 and want_it.m2["scalars"].max() > 0
    _assert_slot(e, 1, want_it, INCREMENTS + AS_IS, "iteration slot:")
    # what accumulates over the iterations is the sum of its increments
    total = L.view(iters[3], "spectra_coupled") - L.view(iters[0], "spectra_coupled")
    assert np.allclose(want_it.mean["spectra_coupled"] * 3, total, rtol=1e-12, atol=1e-12 * total.max())


def test_driver_refuses_what_breaks_the_premise(oracle_run):
    prob, be, L, e, res, ends, iters, max_pcuts = oracle_run
    n0 = [e.count(0), e.count(1)]
    sm = mcs.iter_finalize.SmoothingConfig(smooth_shocks=True)
    comm = mcs.driver.Comm(False)
    comm.enabled = True
    for kw in (dict(tcut_print=True), dict(smoothing=sm), dict(comm=comm)):
        with pytest.raises(ValueError, match="ensemble"):
            mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, ensemble=e, **kw)
    with pytest.raises(ValueError, match="species slots"):
        mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, ensemble=ens.HostEnsemble(prob.params, 0))
    assert [e.count(0), e.count(1)] == n0


def test_run_overlapped_merges_the_contexts_ensembles():
    """Two oracle contexts, three iterations: context 0 takes iterations 1 and 3, context 1 iteration 2; the merged ensemble is
    Chan's merge of the two, and the host statistics of ion_finalize are those of the per-iteration results."""
    n_itrs = 3
    prob = make_problem(300, num_iterations=n_itrs)
    bes = [oracle_backend(prob), oracle_backend(prob)]
    L = bes[0].layout
    ends = {}
    res = mcs.driver.run_overlapped(prob, bes, n_itrs=n_itrs, max_pcuts=4, ensemble=True)
    assert mcs.driver.run_overlapped(prob, bes[:1], n_itrs=1, max_pcuts=1, first_iter=1).ensemble is None
    e = res.ensemble
    assert e.count(0) == 3 and e.count(1) == 3
    for it, ion, f, i in res.per_species:
        ends[it] = (f, i)
    # (the oracle has no light read: every species end hands over the whole buffer)
    sp = {it: species_parts(L, f, i) for it, (f, i) in ends.items()}
    assert sp[1]["therm_sf"].max() > 0
    want = stat_of([sp[1], sp[3]]).merged_with(stat_of([sp[2]]))
    _assert_slot(e, 0, want, sp[1], "merged over the contexts:")
    assert e.finalize_count == 3 and set(e.finalize_mean) == set(ens.FINALIZE_NAMES)
    for name in ens.FINALIZE_NAMES:
        s = stat_of([{name: np.asarray(getattr(fin, name), dtype=np.float64)} for _, _, fin in res.iter_finals])
        assert bits_equal(e.finalize_mean[name], s.mean[name]) and bits_equal(e.finalize_stderr[name], np.sqrt(s.m2[name] / 6.0)), name
    for be in bes:
        be.destroy()
