"""The device accumulator of the ensemble statistics (csrc/mcs_ensemble.hip through ensemble.HipEnsemble) against the plain-numpy
restatement of ensemble_common.py: update, iteration sample and merge bit for bit, the refusals, the driver's calls, and the
tally consumers on the ensemble-mean histograms."""
import numpy as np
import pytest

from conftest import mcs, make_problem, hip_backend, oracle_backend
from ensemble_common import (AS_IS, INCREMENTS, SPECIES_TALLIES, assert_tail_is_exercised, bits_equal, check_one_merge_of_every_kind,
                             crafted_buffers, iteration_parts, species_parts, stat_of)
from photons_all_common import SMALL_ENDS, SMALL_LAYOUT, SMALL_N_PHOTON, SMALL_PROCESSES
from test_gpu_ens_photons import observe
from test_gpu_ens_products import consume

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
TALLY_RTOL = 1e-11          # of each array's maximum: two GPU runs differ by the order of their atomic adds (test_gpu_parity.py)
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def crafted():
    """Five crafted buffers on the stock binning, their species samples, and what one accumulator fed all five must hold."""
    prob = make_problem(64)
    L = mcs.capi.Layout(prob.params)
    assert_tail_is_exercised(ens.EnsLayout(prob.params).fields)
    bufs = crafted_buffers(L)
    parts = [species_parts(L, f, i) for f, i in bufs]
    return prob, L, bufs, parts, stat_of(parts)


def _assert_slot(e, slot, want, names, what=""):
    assert e.count(slot) == want.n, what
    for name in names:
        assert bits_equal(e.mean(slot, name), want.mean[name]), f"{what} mean of {name}"
        assert bits_equal(e.m2(slot, name), want.m2[name]), f"{what} M2 of {name}"


def test_update_is_bit_exact(crafted):
    prob, L, bufs, parts, want = crafted
    hb = hip_backend(prob)
    e = ens.Ensemble.for_backend(hb, 2)
    assert isinstance(e, ens.HipEnsemble)
    for f, i in bufs:
        hb.write_tallies(f, i)
        e.add_species(hb, 1)
    assert e.count(1) == 5 and e.count(0) == 0 and e.count(2) == 0
    _assert_slot(e, 1, want, parts[0])
    assert float(want.mean["num_crossings"][0]) == 2.0 ** 50
    floor = np.arange(0, L.offsets["esc_flux"], 7)
    mean1 = np.concatenate([e.mean(1, n).ravel() for n in SPECIES_TALLIES])
    m21 = np.concatenate([e.m2(1, n).ravel() for n in SPECIES_TALLIES])
    assert np.all(mean1[floor] == 1e-99) and not np.any(m21[floor])
    same = np.flatnonzero(bufs[0][0][:mean1.size] == bufs[1][0][:mean1.size])
    assert same.size > mean1.size // 30 and np.array_equal(mean1[same], bufs[0][0][same]) and not np.any(m21[same])
    for name in parts[0]:
        assert bits_equal(e.stderr(1, name), np.sqrt(want.m2[name] / 20.0)), name
    # the untouched slot is still empty, and the samples left the context as it was
    assert not np.any(e.mean(0, "psd")) and not np.any(e.m2(0, "therm_pf_tht"))
    f, i = hb.read_tallies()
    assert bits_equal(f, bufs[-1][0]) and np.array_equal(i, bufs[-1][1])
    e.destroy(); hb.destroy()


def test_iteration_sample_is_bit_exact(crafted):
    prob, L, bufs, parts, want = crafted
    hb = hip_backend(prob)
    e = ens.HipEnsemble(hb, 1)
    prev = np.zeros(L.total)
    it_parts = []
    for f, i in bufs:
        hb.write_tallies(prev, i)
        e.begin_iteration(hb)
        hb.write_tallies(f, i)              # (every section changes between the snapshot and the sample)
        e.add_iteration(hb)
        it_parts.append(iteration_parts(L, f, prev))
        prev = f
    want_it = stat_of(it_parts)
    assert e.count(1) == 5 and e.count(0) == 0
    _assert_slot(e, 1, want_it, INCREMENTS + AS_IS)
    assert want_it.mean["spectra_sf"].min() < 0 < want_it.mean["spectra_sf"].max()       # growth, not the section itself
    for name in INCREMENTS + AS_IS:
        assert bits_equal(e.stderr(1, name), np.sqrt(want_it.m2[name] / 20.0)), name
    e.destroy(); hb.destroy()


def test_merge_is_chans_and_close_to_one_accumulator(crafted):
    prob, L, bufs, parts, want = crafted
    ha, hb = hip_backend(prob), hip_backend(prob)
    a, b = ens.HipEnsemble(ha, 1), ens.HipEnsemble(hb, 1)
    for k, (f, i) in enumerate(bufs):
        be, e = (ha, a) if k < 3 else (hb, b)
        be.write_tallies(f, i)
        e.add_species(be, 0)
    a.merge(b)
    wa, wb = stat_of(parts[:3]), stat_of(parts[3:])
    merged = wa.merged_with(wb)
    _assert_slot(a, 0, merged, parts[0], "merged:")
    _assert_slot(b, 0, wb, parts[0], "the source of a merge is unchanged:")
    assert a.count(1) == 0 and b.count(1) == 0
    # against one accumulator fed all five (the restatement `want`; test_update_is_bit_exact pins the device to it): every one of
    # the n steps contributes a few roundings of the size of the result
    n = 5
    worst = [0.0, 0.0]
    for name in parts[0]:
        mean, m2 = a.mean(0, name), a.m2(0, name)
        sum_x2 = np.zeros_like(mean)
        for p in parts:
            sum_x2 = sum_x2 + p[name] * p[name]
        d_mean, d_m2 = np.abs(mean - want.mean[name]), np.abs(m2 - want.m2[name])
        with np.errstate(divide="ignore", invalid="ignore"):
            worst[0] = max(worst[0], float(np.nanmax(np.where(want.mean[name] != 0, d_mean / np.abs(want.mean[name]), 0.0))))
            worst[1] = max(worst[1], float(np.nanmax(np.where(sum_x2 != 0, d_m2 / sum_x2, 0.0))))
        assert np.all(d_mean <= 16 * n * EPS * np.abs(want.mean[name])), name
        assert np.all(d_m2 <= 16 * n * EPS * sum_x2), name
    print(f"merge against one accumulator: worst |dmean|/|mean| = {worst[0]:.2e}, worst |dM2|/sum x^2 = {worst[1]:.2e}; bound {16 * n * EPS:.2e}")
    # an empty slot takes the source as it is, an empty source changes nothing
    c = ens.HipEnsemble(ha, 1)
    c.merge(b)
    _assert_slot(c, 0, wb, parts[0], "an empty slot takes the source as it is:")
    d = ens.HipEnsemble(hb, 1)
    b.merge(d)
    _assert_slot(b, 0, wb, parts[0], "an empty source changes nothing:")
    for e in (a, b, c, d):
        e.destroy()
    ha.destroy(); hb.destroy()


def test_one_merge_sends_every_kind_through(crafted):
    """Two accumulators of two species slots with samples in slot 0, the iteration slot, products_slot(0), photons_slot(0) and the
    source slot -- two on one side, three on the other -- and in photons_slot(1) of the second alone: one mcs_ens_merge, every kind."""
    prob, L, bufs, parts, want = crafted
    ha, hb = hip_backend(prob), hip_backend(prob)
    tabs = mcs.consumers.consumer_tables(prob, 1)
    x_log = ens.bin_centres_log10(prob)
    a, b = ens.HipEnsemble(ha, 2), ens.HipEnsemble(hb, 2)
    for be, e, ks in ((ha, a, (1, 2)), (hb, b, (3, 4, 0))):
        e.set_slope_window(0, prob.params.num_psd_mom_bins + 1, x_log)
        e.set_photon_layout(SMALL_LAYOUT)
        for k in ks:
            f, i = bufs[k]
            be.write_tallies(bufs[k - 1][0], i)
            e.begin_iteration(be)
            be.write_tallies(f, i)
            e.add_species(be, 0)
            consume(be, tabs)
            e.add_products(be, 0)
            observe(be, SMALL_PROCESSES[0], k, SMALL_N_PHOTON, SMALL_ENDS)
            e.add_photons(be, 0, deposit=True)
            if e is b:
                observe(be, SMALL_PROCESSES[1], 50 + k, SMALL_N_PHOTON, SMALL_ENDS)
                e.add_photons(be, 1)
            e.add_photons_all()
            e.add_iteration(be)
    slots = [0, a.iteration_slot, a.products_slot(0), a.photons_slot(0), a.photons_slot(1), a.photons_all_slot]
    assert [a._kind(s) for s in slots] == ["species", "iteration", "products", "photons", "photons", "source"]
    check_one_merge_of_every_kind(a, b, {s: b._len(s) for s in slots}, only_b=[b.photons_slot(1)])
    assert a.count(1) == 0 and a.count(a.products_slot(1)) == 0 and a.pending_photons == () and b.pending_photons == ()
    a.destroy(); b.destroy()
    ha.destroy(); hb.destroy()


def test_refusals_change_nothing(crafted):
    prob, L, bufs, parts, want = crafted
    hb = hip_backend(prob)
    other = hip_backend(make_problem(64, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(4.0, 2.0, 1e6, 0.1)]))
    e, e_other, e_wide = ens.HipEnsemble(hb, 1), ens.HipEnsemble(other, 1), ens.HipEnsemble(hb, 2)
    hb.write_tallies(*bufs[0])
    e.add_species(hb, 0)
    one = stat_of(parts[:1])
    refused = [
        ("mcs_ens_add_species", lambda: e.add_species(hb, 1)),               # the iteration slot
        ("mcs_ens_add_species", lambda: e.add_species(hb, 2)),               # out of range
        ("mcs_ens_add_species", lambda: e.add_species(hb, -1)),
        ("mcs_ens_add_species", lambda: e.add_species(other, 0)),            # another layout
        ("mcs_ens_begin_iteration", lambda: e.begin_iteration(other)),
        ("mcs_ens_add_iteration", lambda: e.add_iteration(hb)),              # no begin_iteration
        ("mcs_ens_read", lambda: e.stderr(0, "psd")),                        # n = 1
        ("mcs_ens_merge", lambda: e.merge(e)),
        ("mcs_ens_merge", lambda: e.merge(e_other)),
        ("mcs_ens_merge", lambda: e.merge(e_wide)),                          # other slots
        ("mcs_ens_load_mean", lambda: e.load_mean(1, hb)),
        ("mcs_ens_load_mean", lambda: e.load_mean(0, other)),
        ("mcs_ens_count", lambda: e.count(5)),
    ]
    for who, call in refused:
        with pytest.raises(RuntimeError, match=who):
            call()
    e.begin_iteration(hb); e.add_iteration(hb)
    with pytest.raises(RuntimeError, match="mcs_ens_add_iteration"):
        e.add_iteration(hb)                                                   # the snapshot serves one sample
    assert e.count(0) == 1 and e.count(1) == 1 and e_other.count(0) == 0 and e_other.count(1) == 0
    _assert_slot(e, 0, one, parts[0], "after the refusals:")
    f, i = hb.read_tallies()
    assert bits_equal(f, bufs[0][0]) and np.array_equal(i, bufs[0][1])
    for x in (e, e_other, e_wide, hb, other):
        x.destroy()


N_ITRS, N_PCUTS = 4, 6


@pytest.fixture(scope="module")
def driver_run():
    """driver.run on one HIP context with an ensemble, the buffers of every species end and iteration end collected in the hooks."""
    prob = make_problem(2000, num_iterations=N_ITRS)
    hb = hip_backend(prob)
    e = ens.Ensemble.for_backend(hb, 1)
    ends, iters = [], [hb.read_tallies()[0]]
    res = mcs.driver.run(prob, hb, n_itrs=N_ITRS, max_pcuts=N_PCUTS, species_tallies="full", ensemble=e,
                         on_species_end=lambda it, ion, f, i: ends.append((f.copy(), i.copy())),
                         on_iteration_end=lambda it: iters.append(hb.read_tallies()[0]))
    yield prob, hb, e, res, ends, iters
    e.destroy(); hb.destroy()


def test_driver_samples_are_the_hooks_buffers(driver_run):
    prob, hb, e, res, ends, iters = driver_run
    L = hb.layout
    assert res.ensemble is e and len(ends) == N_ITRS and len(iters) == N_ITRS + 1
    sp = [species_parts(L, f, i) for f, i in ends]
    want = stat_of(sp)
    assert want.m2["therm_sf"].max() > 0 and want.m2["therm_sf_mom"].max() > 0
    _assert_slot(e, 0, want, sp[0], "species slot:")
    want_it = stat_of([iteration_parts(L, iters[k + 1], iters[k]) for k in range(N_ITRS)])
    _assert_slot(e, 1, want_it, INCREMENTS + AS_IS, "iteration slot:")
    # the same run on two contexts, every context with an accumulator of its own, merged at the end
    bes = [hip_backend(prob), hip_backend(prob)]
    ovl = mcs.driver.run_overlapped(prob, bes, n_itrs=N_ITRS, max_pcuts=N_PCUTS, ensemble=True)
    eo = ovl.ensemble
    assert eo.count(0) == N_ITRS and eo.count(1) == N_ITRS
    for slot, names in ((0, sp[0]), (1, INCREMENTS + AS_IS)):
        for name in names:
            a, b = eo.mean(slot, name), e.mean(slot, name)
            scale = float(np.max(np.abs(b)))
            assert float(np.max(np.abs(a - b))) <= TALLY_RTOL * scale, (slot, name)
    assert eo.finalize_count == N_ITRS and set(eo.finalize_mean) == set(ens.FINALIZE_NAMES)
    for name in ens.FINALIZE_NAMES:
        s = stat_of([{name: np.asarray(getattr(fin, name), dtype=np.float64)} for _, _, fin in ovl.iter_finals])
        assert bits_equal(eo.finalize_mean[name], s.mean[name])
        assert bits_equal(eo.finalize_stderr[name], np.sqrt(s.m2[name] / float(N_ITRS * (N_ITRS - 1)))), name
    eo.destroy()
    for be in bes:
        be.destroy()


def relerr(a, b):
    s = float(np.max(np.abs(b)))
    return float(np.max(np.abs(a - b))) / s if s > 0 else float(np.max(np.abs(a)))


def test_consumers_run_on_the_ensemble_mean(driver_run):
    prob, hb, e, res, ends, iters = driver_run
    L = hb.layout
    f0, i0 = hb.read_tallies()
    e.load_mean(0, hb)
    f, i = hb.read_tallies()
    for name in SPECIES_TALLIES + ("energy_recv_pool",):
        assert bits_equal(L.view(f, name), e.mean(0, name)), name
    assert np.array_equal(i[:L.n_grid], np.rint(e.mean(0, "num_crossings")).astype(np.int64))
    for name in mcs.capi.RUNNING_F64:
        assert bits_equal(L.view(f, name), L.view(f0, name)), name
    assert np.array_equal(i[L.n_grid:], i0[L.n_grid:])
    assert not bits_equal(L.view(f, "therm_sf"), L.view(f0, "therm_sf"))          # (the mean is not the last realisation)
    ob = oracle_backend(prob)
    for hist in (True, False):
        t = mcs.consumers.consumer_tables(prob, 1, therm_from_hist=hist)
        d_g, g_g = hb.dndp_cr(t)
        d_o, g_o = ob.dndp_cr(t, tallies=(f, i))
        assert np.array_equal(g_o, g_g)
        for m in range(3):
            assert relerr(d_g[m], d_o[m]) < 1e-12, m
        for a, b in zip(hb.thermo_calcs(t), ob.thermo_calcs(t, tallies=(f, i))):
            assert relerr(a, b) < 1e-9
    ob.destroy()
