"""K14, mcs_detector_spectra (csrc/mcs_consumers.hip: mcs_k_detector_rows, mcs_k_detector_join) on crafted rows of spectra_sf and
spectra_pf against the restatement of tests/detectors_common.py: every output word bit for bit, at the stock binning of make_problem
and at the largest the library accepts, for the second of two species, with nd = 1, 3, 5 and n_grid and NaN in everything the call
must not read; the reproducibility of the bits, the quiet NaNs, an overwritten tally, the refusals, and one real species against the
numpy path on the tallies and the base of the same context."""
import ctypes as ct

import numpy as np
import pytest

import consumers_common as cc
import detectors_common as dc
from conftest import mcs, make_problem, hip_backend

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
BINNINGS = {"stock": {}, "largest": cc.LARGE_BINNING}
QUIET_NAN = 0x7FF8000000000000


@pytest.fixture(scope="module", params=list(BINNINGS))
def ctx(request):
    prob = dc.two_ion_problem(make_problem, **BINNINGS[request.param])
    assert prob.params.n_ions == 2 and prob.params.num_psd_mom_bins == (199 if request.param == "largest" else 155)
    prob.rg0 = dc.X_UNIT                  # (the unit of the gradient's x that consumers.detector_spectra passes)
    hb = hip_backend(prob)
    yield prob, hb
    hb.destroy()


def quiet_nans(a):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return np.all(a[np.isnan(a)].view(np.uint64) & np.uint64(QUIET_NAN) == np.uint64(QUIET_NAN))


@pytest.mark.parametrize("scenario", list(dc.scenarios(8, 7)))
def test_crafted_rows(ctx, scenario):
    """Every output word equals the restatement's; a second call on the same buffers gives the same bits."""
    prob, hb = ctx
    nm = prob.params.num_psd_mom_bins
    sc = dc.scenarios(nm, prob.params.n_grid)[scenario]
    now, base, _ = dc.load_rows(hb, prob, 2, sc)
    tabs = mcs.consumers.consumer_tables(prob, 2)
    ref = dc.reference(now, base, tabs.mom_log_cgs, tabs.mom_edge_cgs, prob.x_spec, nm, sc.window, dc.X_UNIT, lambda a: hb.eval_fn("log10", a))
    dc.check_claims(scenario, sc, ref, nm)
    got = mcs.consumers.detector_spectra(prob, hb, 2, window=sc.window)
    dc.assert_same(got, ref, scenario)
    nd = len(sc.x)
    assert got.number.shape == (2, nd) and got.spectrum.shape == (2, nd, nm + 2) and got.gradient.shape == (nm + 2,)
    assert quiet_nans(got.words()) and np.all(np.isfinite(got.spectrum)) and np.all(np.isfinite(got.dndp)) and got.diag[1] == 0
    again = mcs.consumers.detector_spectra(prob, hb, 2, window=sc.window)
    assert dc.bits_equal(again.words(), got.words()) and np.array_equal(again.diag, got.diag)
    print(f"{scenario}: {nd} detectors, diag {got.diag.tolist()}")


def test_an_overwritten_tally_shows_in_diag(ctx):
    """now < base in three words (a caller overwrote the tallies): diag[1] counts them, and the words are what the rules give."""
    prob, hb = ctx
    nm = prob.params.num_psd_mom_bins
    R = dc.crafted_rows(nm)
    b, n = R["dense_1"]
    n = n.copy(); n[3] = b[3] - 0.25; n[nm] = b[nm] - 1.0e-3
    b2, n2 = R["full_1"]
    n2 = n2.copy(); n2[7] = b2[7] - 0.125
    sc = dc.Scenario([R["dense_2"], (b, n), R["one_bin_first"]], [R["full_0"], (b2, n2), R["full_2"]], [-0.5, -0.3, -0.1], (0, nm + 1))
    now, base, _ = dc.load_rows(hb, prob, 2, sc)
    tabs = mcs.consumers.consumer_tables(prob, 2)
    ref = dc.reference(now, base, tabs.mom_log_cgs, tabs.mom_edge_cgs, prob.x_spec, nm, sc.window, dc.X_UNIT, lambda a: hb.eval_fn("log10", a))
    got = mcs.consumers.detector_spectra(prob, hb, 2, window=sc.window)
    dc.assert_same(got, ref, "overwritten")
    assert got.diag[:2].tolist() == [6, 3] and got.dndp[0, 1, 3] < 0 and got.spectrum[0, 1, 3] == 1e-99


def test_refusals(ctx):
    prob, hb = ctx
    lib = hb.lib
    nm = prob.params.num_psd_mom_bins
    dp = mcs.capi.c_double_p
    tabs = mcs.consumers.consumer_tables(prob, 2)
    sc = dc.scenarios(nm, prob.params.n_grid)["three_upstream_dense"]
    dc.load_rows(hb, prob, 2, sc)
    good = mcs.consumers.detector_spectra(prob, hb, 2)
    out = np.zeros(good.words().size)
    s = tabs.as_struct()
    call = lambda h, l_lo, l_hi, xu, st=s: lib.mcs_detector_spectra(h, ct.byref(st), l_lo, l_hi, xu, out.ctypes.data_as(dp), None)
    for l_lo, l_hi in ((-1, 5), (0, nm + 2), (4, 6), (7, 3)):
        assert call(hb.h, l_lo, l_hi, 1.0) != 0 and b"mcs_detector_spectra: window" in lib.mcs_last_error() and not out.any()
    for xu in (0.0, -1.0, float("inf"), float("nan")):
        assert call(hb.h, 0, nm + 1, xu) != 0 and b"mcs_detector_spectra: x_unit must be finite and positive" in lib.mcs_last_error() and not out.any()
    assert lib.mcs_detector_spectra(hb.h, None, 0, nm + 1, 1.0, out.ctypes.data_as(dp), None) != 0 and b"null argument" in lib.mcs_last_error()
    assert lib.mcs_detector_spectra(hb.h, ct.byref(s), 0, nm + 1, 1.0, None, None) != 0 and b"null argument" in lib.mcs_last_error()
    flat = mcs.consumers.consumer_tables(prob, 2)
    flat.mom_edge_cgs = flat.mom_edge_cgs.copy(); flat.mom_edge_cgs[5] = flat.mom_edge_cgs[4]
    assert call(hb.h, 0, nm + 1, 1.0, flat.as_struct()) != 0 and b"not strictly ascending" in lib.mcs_last_error() and not out.any()
    # the refused calls left the result of the good one alone: a sample can still be taken from it
    e = ens.HipEnsemble(hb, 2)
    e.add_detectors(hb, 1, good)
    assert dc.same_words(e.mean(e.detectors_slot(1), "gradient"), good.gradient)
    e.destroy()
    # cuts set after the species began: the base is gone
    hb.set_cuts(prob)
    with pytest.raises(RuntimeError, match="mcs_detector_spectra: no base"):
        hb.detector_spectra(tabs, 0, nm + 1, 1.0)
    # no species begun; no detector set
    fresh = hip_backend(prob)
    try:
        with pytest.raises(RuntimeError, match="mcs_detector_spectra: no species has begun"):
            fresh.detector_spectra(tabs, 0, nm + 1, 1.0)
    finally:
        fresh.destroy()
    none = make_problem(64)
    hn = hip_backend(none)
    try:
        hn.begin_species(1, 1, 1.0, 1.0, none.pmax, 1.0, 1.0)
        assert call(hn.h, 0, nm + 1, 1.0) != 0 and b"mcs_detector_spectra: no detector is set" in lib.mcs_last_error() and not out.any()
        with pytest.raises(ValueError, match="no detector"):
            mcs.consumers.detector_spectra(none, hn, 1)
    finally:
        hn.destroy()
    # a context whose cuts were never set
    h = ct.c_void_p(None)
    assert lib.mcs_create(ct.byref(prob.params), 0, None, ct.byref(h)) == 0
    try:
        assert call(h, 0, nm + 1, 1.0) != 0 and b"mcs_detector_spectra: cuts not set" in lib.mcs_last_error() and not out.any()
    finally:
        lib.mcs_destroy(h)


def test_a_real_species_equals_the_numpy_path():
    """4000 protons through 12 pcuts with detectors at (-0.5, -0.3, -0.1, 0.05, 2.0) rg0, two iterations of one context: the device
    result of each equals the numpy statement of the same rules on the tallies downloaded after the species and on the base
    downloaded before it -- the second iteration's base is the first's tallies.  The tallies come from atomic adds, so the run is
    compared with itself, never with another run."""
    prob = dc.xspec_problem(make_problem, 4000, num_iterations=2)
    nm, nd = prob.params.num_psd_mom_bins, len(prob.x_spec)
    hb = hip_backend(prob)
    try:
        log10 = lambda a: hb.eval_fn("log10", a)
        tabs = mcs.consumers.consumer_tables(prob, 1)
        state, before = None, mcs.consumers.detector_base(hb, nd)
        numbers, diags = [], []
        for it in (1, 2):
            res = mcs.driver.run(prob, hb, n_itrs=1, first_iter=it, iter_state=state, max_pcuts=12, finalize=True, detectors=True)
            state = res.iter_state
            (i_iter, i_ion, got), = res.detectors
            after = mcs.consumers.detector_base(hb, nd)
            args = (after, before, tabs.mom_log_cgs, tabs.mom_edge_cgs, prob.x_spec, nm, (0, nm + 1), prob.rg0, log10)
            want = mcs.consumers.detector_spectra_host(*args)
            assert (i_iter, i_ion) == (it, 1)
            dc.assert_same(got, want, f"iteration {it}")
            dc.assert_same(got, dc.reference(*args), f"iteration {it}, the restatement")
            assert np.all(after[1] >= before[1]) and quiet_nans(got.words())
            numbers.append(got.number); diags.append(got.diag)
            print(f"iteration {it}: diag {got.diag.tolist()}, number {got.number.tolist()}, slope {got.slope.tolist()}, "
                  f"gradient {got.gradient[np.isfinite(got.gradient)].tolist()}")
            before = after
        assert np.all(numbers[0] > 1e-99) and diags[0][0] == 10 and diags[0][2] >= 1
        live = (numbers[0] > 0) & (numbers[1] > 0)
        assert np.all(numbers[1][live] < 1.5 * numbers[0][live])          # a growth, not the running sum
    finally:
        hb.destroy()
