"""The detector spectra without a GPU: the entry points and layouts (include/mcs.h, mcs_detector_spectra and "detectors sample"), the
numpy path of consumers.detector_spectra against the restatement of tests/detectors_common.py word for word on every crafted
scenario, the detectors slots of HostEnsemble, the refusals of the ensembles and of driver.run / run_overlapped, and one run on the
oracle backend with a row of detectors."""
import ctypes as ct
import os

import numpy as np
import pytest

import consumers_common as cc
import detectors_common as dc
from conftest import ROOT, mcs, make_problem, oracle_backend

ens = mcs.ensemble
BINNINGS = {"stock": {}, "largest": cc.LARGE_BINNING}
XSPEC_RG = dc.XSPEC_RG


def xspec_problem(n, **kw):
    return dc.xspec_problem(make_problem, n, **kw)


# ---- (a) the ABI and the layouts -----------------------------------------------------------------------------------------------------
def test_entry_points_and_layouts():
    lib = mcs.capi.load_library()
    for name in ("mcs_detector_spectra", "mcs_detector_get_layout", "mcs_ens_detectors_get_layout", "mcs_ens_add_detectors"):
        assert hasattr(lib, name) and name in mcs.capi.EXPORTED_SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "mcs.h")).read()
    assert "#define MCS_ENS_DETECTORS(s) ((s) | (1 << 23))" in header and mcs.capi.ENS_DETECTORS_BIT == 1 << 23
    for kw in (cc.SMALL_BINNING, cc.LARGE_BINNING, {}):
        P = make_problem(64, **kw).params
        NM = P.num_psd_mom_bins + 2
        for nd in (1, 3, 5, P.n_grid):
            # hand-counted: 2 nd rows of NM twice, then number, mean_log_p, three quantile rows, slope of 2 nd each, then NM
            r = 2 * nd
            want = dict(spectrum=0, dndp=r * NM, number=2 * r * NM, mean_log_p=2 * r * NM + r, quantile=2 * r * NM + 2 * r,
                        slope=2 * r * NM + 5 * r, gradient=2 * r * NM + 6 * r, row_n=NM, n_det=nd, total=2 * r * NM + 6 * r + NM)
            for fn in (lib.mcs_detector_get_layout, lib.mcs_ens_detectors_get_layout):
                X = mcs.capi.McsDetectorLayout()
                assert fn(ct.byref(P), nd, ct.byref(X)) == 0
                assert {name: int(getattr(X, name)) for name, _ in X._fields_} == want, (fn, nd)
            mirror = ens.EnsLayout(P)
            assert mirror.detectors_fields(nd) == want
            assert mirror.detectors(nd) == {"spectrum": (0, (r, NM)), "dndp": (r * NM, (r, NM)), "number": (2 * r * NM, (r,)),
                                            "mean_log_p": (2 * r * NM + r, (r,)), "quantile": (2 * r * NM + 2 * r, (3, r)),
                                            "slope": (2 * r * NM + 5 * r, (r,)), "gradient": (2 * r * NM + 6 * r, (NM,))}
    assert NM == 157
    X = mcs.capi.McsDetectorLayout()
    for bad in (0, -1, P.n_grid + 1):
        assert lib.mcs_detector_get_layout(ct.byref(P), bad, ct.byref(X)) != 0 and b"n_det outside 1..n_grid" in lib.mcs_last_error()
        with pytest.raises(ValueError, match="n_det outside"):
            mcs.capi.detector_layout(P, bad)
    assert lib.mcs_ens_detectors_get_layout(None, 3, ct.byref(X)) != 0 and b"mcs_ens_detectors_get_layout" in lib.mcs_last_error()
    assert lib.mcs_detector_get_layout(ct.byref(P), 3, None) != 0


def test_no_context_no_spectra():
    lib = mcs.capi.load_library()
    prob = make_problem(64)
    s = mcs.consumers.consumer_tables(prob, 1).as_struct()
    out = np.zeros(mcs.capi.detector_layout(prob.params, 3).total)
    assert lib.mcs_detector_spectra(None, ct.byref(s), 0, 10, 1.0, out.ctypes.data_as(mcs.capi.c_double_p), None) != 0 and not out.any()
    assert lib.mcs_ens_add_detectors(None, None, 0) != 0 and b"mcs_ens_add_detectors" in lib.mcs_last_error()


# ---- (b) the numpy path against the restatement ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(BINNINGS))
def oracle_ctx(request):
    prob = dc.two_ion_problem(make_problem, **BINNINGS[request.param])
    assert prob.params.n_ions == 2 and prob.params.num_psd_mom_bins == (199 if request.param == "largest" else 155)
    prob.rg0 = dc.X_UNIT                  # (the unit of the gradient's x that consumers.detector_spectra passes)
    return prob, oracle_backend(prob)


def spectra_of(prob, be, sc, block=None):
    return mcs.consumers.detector_spectra(prob, be, 2, window=sc.window, base=block)


def test_numpy_path_equals_the_restatement(oracle_ctx):
    """Every crafted scenario (nd = 1, 3, 5, n_grid; the species is the second of two), word for word."""
    prob, ob = oracle_ctx
    nm = prob.params.num_psd_mom_bins
    log10 = ens._det_log10(ob)
    tabs = mcs.consumers.consumer_tables(prob, 2)
    seen = set()
    for name, sc in dc.scenarios(nm, prob.params.n_grid).items():
        now, base, block = dc.load_rows(ob, prob, 2, sc)
        ref = dc.reference(now, base, tabs.mom_log_cgs, tabs.mom_edge_cgs, prob.x_spec, nm, sc.window, dc.X_UNIT, log10)
        dc.check_claims(name, sc, ref, nm)
        got = spectra_of(prob, ob, sc, block)
        dc.assert_same(got, ref, name)
        assert dc.same_words(got.words(), ref.words()) and got.words().size == mcs.capi.detector_layout(prob.params, len(sc.x)).total
        assert np.all(np.isfinite(got.spectrum)) and np.all(np.isfinite(got.dndp)) and got.window == sc.window and got.x_unit == dc.X_UNIT
        seen.add(len(sc.x))
    assert seen == {1, 3, 5, prob.params.n_grid}


def test_host_refusals(oracle_ctx):
    prob, ob = oracle_ctx
    nm = prob.params.num_psd_mom_bins
    sc = dc.scenarios(nm, prob.params.n_grid)["three_upstream_dense"]
    now, base, block = dc.load_rows(ob, prob, 2, sc)
    with pytest.raises(ValueError, match="needs the base"):
        mcs.consumers.detector_spectra(prob, ob, 2)
    for bad in ((-1, 5), (0, nm + 2), (4, 6), (7, 3)):
        with pytest.raises(ValueError, match="window"):
            mcs.consumers.detector_spectra(prob, ob, 2, window=bad, base=block)
    tabs = mcs.consumers.consumer_tables(prob, 2)
    args = (now, base, tabs.mom_log_cgs, tabs.mom_edge_cgs, prob.x_spec, nm, (0, nm + 1))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="x_unit"):
            mcs.consumers.detector_spectra_host(*args, bad, ens._det_log10(ob))
    E = tabs.mom_edge_cgs.copy(); E[5] = E[4]
    with pytest.raises(ValueError, match="strictly ascending"):
        mcs.consumers.detector_spectra_host(now, base, tabs.mom_log_cgs, E, prob.x_spec, nm, (0, nm + 1), dc.X_UNIT, ens._det_log10(ob))
    none = make_problem(64)
    assert len(none.x_spec) == 0
    with pytest.raises(ValueError, match="no detector"):
        mcs.consumers.detector_spectra(none, oracle_backend(none), 1, base=np.zeros((2, 1, 201)))


# ---- (c) the detectors slots of the numpy ensemble ------------------------------------------------------------------------------------
def crafted_spectra(prob, ob, names):
    out = []
    S = dc.scenarios(prob.params.num_psd_mom_bins, prob.params.n_grid)
    for name in names:
        _, _, block = dc.load_rows(ob, prob, 2, S[name])
        out.append(spectra_of(prob, ob, S[name], block))
    return out


SAME_SETTINGS = ("three_upstream_dense", "three_small_sums")           # (the same positions and window)


def test_host_ensemble_detectors_slot(oracle_ctx):
    prob, ob = oracle_ctx
    NM = prob.params.num_psd_mom_bins + 2
    samples = crafted_spectra(prob, ob, SAME_SETTINGS + ("three_upstream_dense",))
    e = ens.HostEnsemble(prob.params, 2)
    s = e.detectors_slot(1)
    assert s == 1 | (1 << 23) and e.is_detectors(s) and not e.is_detectors(e.tcuts_slot(1)) and not e.is_tcuts(s) and not e.is_angles(s)
    assert not e.is_detectors(e.photons_all_slot) and not e.is_detectors(e.profile_slot) and not e.is_detectors(1) and e.count(s) == 0
    assert not e.is_profile(s) and not e.is_escape(s) and not e.is_products(s)
    with pytest.raises(ValueError, match="no sample yet"):
        e.word_range(s, "number")
    with pytest.raises(ValueError, match="no settings yet"):
        e.detectors_row(0, 0)
    for x in samples:
        e.add_detectors(ob, 1, x)
    assert e.count(s) == 3 and e.count(e.detectors_slot(0)) == 0 and e.detectors_settings[0] == 3 and e.names(s) == ens.DETECTORS_NAMES
    assert e.detectors_row(1, 2) == (5, 6)
    with np.errstate(invalid="ignore"):
        mean, err, n = ens.stats_over([x.words() for x in samples])
    lay = ens.EnsLayout(prob.params).detectors(3)
    for name in ens.DETECTORS_NAMES:
        off, shape = lay[name]
        cnt = int(np.prod(shape))
        assert dc.same_words(e.mean(s, name).ravel(), mean[off:off + cnt]), name
        assert dc.same_words(e.stderr(s, name).ravel(), err[off:off + cnt]), name
    assert e.word_range(s, "dndp", zones=e.detectors_row(1, 0), bins=(3, 20)) == (6 * NM + 3 * NM + 3, 17)
    assert e.word_range(s, "quantile", zones=(1, 2), bins=e.detectors_row(0, 2)) == (12 * NM + 12 + 6 + 2, 1)
    assert e.word_range(s, "gradient", zones=(4, 9)) == (12 * NM + 36 + 4, 5)
    # row (0, 2) is live in every sample; row (0, 0) was dead in one: it stays non-finite and no trigger on it is met
    got = e.summarize(s, [ens.Request("number", zones=e.detectors_row(0, 2)), ens.Request("mean_log_p", zones=e.detectors_row(0, 0)),
                          ens.Request("gradient", zones=(0, NM))])
    assert got[0].n_nonfinite == 0 and got[0].n_selected == 1 and got[1].n_nonfinite == 1 and got[2].n_nonfinite >= 1
    dead, alive = (ens.Trigger(s, "mean_log_p", "max", 1e30, zones=e.detectors_row(0, d)) for d in (0, 2))
    e.check_trigger(dead); e.check_trigger(alive)
    assert not dead.met(e.summarize(s, [dead.request])[0]) and alive.met(e.summarize(s, [alive.request])[0])


def test_ensemble_refusals(oracle_ctx):
    prob, ob = oracle_ctx
    three, window, unsorted5, at_zero = crafted_spectra(prob, ob, ("three_upstream_dense", "three_window_two_valid", "five_unsorted", "three_one_at_zero"))
    a, b = ens.HostEnsemble(prob.params, 2), ens.HostEnsemble(prob.params, 2)
    with pytest.raises(ValueError, match="only a species slot"):
        a.detectors_slot(2)
    with pytest.raises(ValueError, match="a detectors slot"):
        a.add_detectors(ob, 2, three)
    with pytest.raises(ValueError, match="from a DetectorSpectra"):
        a.add_detectors(ob, 0, None)
    for _ in range(2):
        a.add_detectors(ob, 0, three)
        b.add_detectors(ob, 0, unsorted5)
    for other in (window, unsorted5, at_zero):       # another window, another nd, another x_spec
        with pytest.raises(ValueError, match="differ from those of the ensemble's detectors samples"):
            a.add_detectors(ob, 1, other)
    import dataclasses
    with pytest.raises(ValueError, match="differ from those"):
        a.add_detectors(ob, 1, dataclasses.replace(three, x_unit=dc.up(three.x_unit)))
    with pytest.raises(ValueError, match="differ from those"):
        a.expect_detectors(unsorted5.settings())
    a.expect_detectors(three.settings())
    with pytest.raises(ValueError, match="detectors samples differ in their settings"):
        a.merge(b)
    with pytest.raises(ValueError, match="detectors samples differ in their settings"):
        a.summarize_merged([b], a.detectors_slot(0), [ens.Request("number")])
    with pytest.raises(ValueError, match="detectors samples differ in their settings"):
        a.compare(b, a.detectors_slot(0), [ens.CompareRequest("number")])
    with pytest.raises(ValueError, match="frames 0, 1 and detectors 0..2"):
        a.detectors_row(0, 3)
    with pytest.raises(ValueError, match="frames 0, 1"):
        a.detectors_row(2, 0)
    # ... and what is allowed: a merge into an ensemble that has none takes the source's settings
    c = ens.HostEnsemble(prob.params, 2)
    c.merge(a)
    assert c.detectors_settings == three.settings() and c.count(c.detectors_slot(0)) == 2
    d = a.compare(c, a.detectors_slot(0), [ens.CompareRequest("number"), ens.CompareRequest("gradient")])
    assert d[0].max_abs_z == 0.0


def test_driver_refusals():
    prob = xspec_problem(64)
    ob = oracle_backend(prob)
    run = mcs.driver.run
    with pytest.raises(ValueError, match="detectors: needs finalize=True"):
        run(prob, ob, n_itrs=1, max_pcuts=1, detectors=True)
    with pytest.raises(ValueError, match="window"):
        run(prob, ob, n_itrs=1, max_pcuts=1, finalize=True, detectors=(5, 6))
    e = ens.HostEnsemble(prob.params, 1)
    with pytest.raises(ValueError, match="a trigger on a detectors slot needs detectors=True"):
        run(prob, ob, n_itrs=2, max_pcuts=1, finalize=True, ensemble=e, triggers=[ens.Trigger(e.detectors_slot(0), "number", "max", 0.1)])

    class FakeComm:
        enabled, rank, world = True, 0, 1
    with pytest.raises(ValueError, match="communicator"):
        run(prob, ob, comm=FakeComm(), n_itrs=1, max_pcuts=1, finalize=True, detectors=True)
    with pytest.raises(ValueError, match="detectors: one context only.*shared by all species.*accumulate_tallies"):
        run(prob, ob, n_itrs=1, max_pcuts=1, finalize=True, detectors=True, species_backends=[oracle_backend(prob)])
    with pytest.raises(ValueError, match="detectors: the overlapped run leaves the detector spectra out"):
        mcs.driver.run_overlapped(prob, [ob], n_itrs=1, detectors=True)
    with pytest.raises(ValueError, match="detectors: the overlapped run leaves the detector spectra out"):
        mcs.driver.run_overlapped(prob, [ob], n_itrs=2, ensemble=True, triggers=[ens.Trigger(e.detectors_slot(0), "number", "max", 0.1)])
    none = make_problem(64)
    with pytest.raises(ValueError, match="detectors: the problem has no detector"):
        run(none, oracle_backend(none), n_itrs=1, max_pcuts=1, finalize=True, detectors=True)
    fields = [f.name for f in __import__("dataclasses").fields(mcs.driver.RunResult)]
    assert fields[-1] == "angles" and "detectors" in fields


# ---- (d) one run on the oracle backend ------------------------------------------------------------------------------------------------
def test_one_run_on_the_oracle_backend():
    """driver.run(finalize=True, detectors=True) with the numpy path: 4000 protons, 12 pcuts, two iterations, detectors at
    (-0.5, -0.3, -0.1, 0.05, 2.0) rg0.  All ten rows are live in iteration 1, some gradient word is finite, and iteration 2's numbers
    are a growth, not the running sum: below 1.5 x iteration 1's in every row live in both."""
    prob = xspec_problem(4000, num_iterations=2)
    assert np.allclose(prob.x_spec / prob.rg0, XSPEC_RG, rtol=1e-15)
    ob = oracle_backend(prob)
    e = ens.HostEnsemble(prob.params, 1)
    res = mcs.driver.run(prob, ob, n_itrs=2, max_pcuts=12, finalize=True, detectors=True, ensemble=e)
    assert [(it, ion) for it, ion, _ in res.detectors] == [(1, 1), (2, 1)] and e.count(e.detectors_slot(0)) == 2
    (_, _, first), (_, _, second) = res.detectors
    nm = prob.params.num_psd_mom_bins
    print("iteration 1 number", first.number.tolist()); print("iteration 2 number", second.number.tolist())
    print("gradient", first.gradient[np.isfinite(first.gradient)].tolist(), "diag", first.diag.tolist(), second.diag.tolist())
    assert first.window == (0, nm + 1) and first.x_unit == prob.rg0
    assert np.all(first.number > 1e-99) and first.diag[0] == 10
    # (spectra_pf takes positive deposits only; those of spectra_sf are signed, so its rows may hold bins with now < base: diag[1])
    now_pf, base_pf = ob.layout.view(res.per_species[1][2], "spectra_pf")[:5], ob.layout.view(res.per_species[0][2], "spectra_pf")[:5]
    assert np.all(now_pf >= base_pf) and np.all(first.dndp[1] > 0) and np.all(second.dndp[1] > 0)
    assert first.diag[2] >= 1 and np.isfinite(first.gradient).sum() == first.diag[2]
    both = (first.number > 1e-99) & (second.number > 1e-99)
    assert both.sum() >= 8 and np.all(second.number[both] < 1.5 * first.number[both])
    sf2 = ob.layout.view(res.per_species[1][2], "spectra_sf")
    assert sf2[0, :nm + 1].sum() > 1.5 * first.number[0, 0]             # (while the tally itself holds both iterations)
    assert np.all(np.diff(first.quantile, axis=0) >= 0)                 # the 50, 90, 99 % momenta are ordered
    assert dc.same_words(e.mean(e.detectors_slot(0), "number").ravel(), ens.stats_over([first.number.ravel(), second.number.ravel()])[0])
    assert e.summarize(e.detectors_slot(0), [ens.Request("gradient", zones=(0, nm + 2))])[0].n_nonfinite >= 1
