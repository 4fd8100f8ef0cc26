"""K12, mcs_tcut_spectra (csrc/mcs_consumers.hip: mcs_k_tcut_rows, mcs_k_tcut_index) on crafted rows of spectra_coupled against the
restatement of tests/tcuts_common.py: every output word bit for bit, at the stock binning of make_problem and at the largest the
library accepts, for the second of two species, with n_tcuts = 1, 3 and 99 and NaN in everything the call must not read; the
reproducibility of the bits, the refusals, and one real species against the numpy path on the tallies and the base of the same
context."""
import ctypes as ct

import numpy as np
import pytest

import consumers_common as cc
import tcuts_common as tc
from conftest import mcs, make_problem, hip_backend

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
BINNINGS = {"stock": {}, "largest": cc.LARGE_BINNING}
QUIET_NAN = 0x7FF8000000000000


@pytest.fixture(scope="module", params=list(BINNINGS))
def ctx(request):
    prob = tc.two_ion_problem(make_problem, **BINNINGS[request.param])
    assert prob.params.n_ions == 2 and prob.params.num_psd_mom_bins == (199 if request.param == "largest" else 155)
    hb = hip_backend(prob)
    yield prob, hb
    hb.destroy()


def quiet_nans(a):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return np.all(a[np.isnan(a)].view(np.uint64) & np.uint64(QUIET_NAN) == np.uint64(QUIET_NAN))


@pytest.mark.parametrize("scenario", list(tc.scenarios(8)))
def test_crafted_rows(ctx, scenario):
    """Every output word equals the restatement's; a second call on the same buffers gives the same bits."""
    prob, hb = ctx
    nm = prob.params.num_psd_mom_bins
    rows = tc.scenarios(nm)[scenario]
    now, base, weight, _ = tc.load_rows(hb, prob, 2, rows)
    tabs = mcs.consumers.consumer_tables(prob, 2)
    ref = tc.reference(now, base, weight, tabs.mom_log_cgs, prob.tcuts, nm, lambda a: hb.eval_fn("log10", a))
    got = mcs.consumers.tcut_spectra(prob, hb, 2)
    tc.assert_same(got, ref, scenario)
    assert len(got.number) == len(rows) and got.spectrum.shape == (len(rows), nm + 2)
    assert quiet_nans(got.words()) and np.all(np.isfinite(got.spectrum)) and np.all(np.isfinite(got.weight)) and got.diag[1] == 0
    again = mcs.consumers.tcut_spectra(prob, hb, 2)
    assert tc.bits_equal(again.words(), got.words()) and np.array_equal(again.diag, got.diag)
    live = int((ref.number > 0).sum())
    if "two_live" in scenario:
        assert live == 2 and np.all(np.isnan(got.index))
    if "three_live" in scenario:
        assert live == 3 and np.all(np.isfinite(got.index))
    print(f"{scenario}: {len(rows)} cuts, {live} live, index {got.index.tolist()}")


def test_an_overwritten_tally_shows_in_diag(ctx):
    """now < base in two words (a caller overwrote the tallies): diag[1] counts them, and the words are what the rules give."""
    prob, hb = ctx
    nm = prob.params.num_psd_mom_bins
    R = tc.crafted_rows(nm)
    b, n, w = R["dense_1"]
    n = n.copy(); n[3] = b[3] - 0.25; n[nm] = b[nm] - 1.0e-3
    now, base, weight, _ = tc.load_rows(hb, prob, 2, [R["dense_2"], (b, n, w), R["one_bin_first"]])
    tabs = mcs.consumers.consumer_tables(prob, 2)
    ref = tc.reference(now, base, weight, tabs.mom_log_cgs, prob.tcuts, nm, lambda a: hb.eval_fn("log10", a))
    got = mcs.consumers.tcut_spectra(prob, hb, 2)
    tc.assert_same(got, ref, "overwritten")
    assert got.diag.tolist() == [3, 2]


def test_refusals(ctx):
    prob, hb = ctx
    lib = hb.lib
    tabs = mcs.consumers.consumer_tables(prob, 2)
    fresh = hip_backend(prob)
    try:
        with pytest.raises(RuntimeError, match="mcs_tcut_spectra: no species has begun"):
            fresh.tcut_spectra(tabs)
    finally:
        fresh.destroy()
    none = make_problem(64, TCUTS=None)
    hn = hip_backend(none)
    try:
        hn.begin_species(1, 1, 1.0, 1.0, none.pmax, 1.0, 1.0)
        s = tabs.as_struct()
        out = np.zeros(16)
        assert lib.mcs_tcut_spectra(hn.h, ct.byref(s), out.ctypes.data_as(mcs.capi.c_double_p), None) != 0
        assert b"mcs_tcut_spectra: the context tracks no time cuts" in lib.mcs_last_error() and not out.any()
        with pytest.raises(ValueError, match="tracks no time cuts"):
            mcs.consumers.tcut_spectra(none, hn, 1)
    finally:
        hn.destroy()
    # a context whose cuts were never set
    h = ct.c_void_p(None)
    assert lib.mcs_create(ct.byref(prob.params), 0, None, ct.byref(h)) == 0
    try:
        s = tabs.as_struct()
        out = np.zeros(mcs.capi.tcut_layout(prob.params, 3).total)
        assert lib.mcs_tcut_spectra(h, ct.byref(s), out.ctypes.data_as(mcs.capi.c_double_p), None) != 0
        assert b"mcs_tcut_spectra: cuts not set" in lib.mcs_last_error() and not out.any()
    finally:
        lib.mcs_destroy(h)


def test_a_real_species_equals_the_numpy_path():
    """4000 protons through 12 pcuts, two iterations of one context: the device result of each equals the numpy statement of the
    same rules on the tallies downloaded after the species and on the base downloaded before it -- the second iteration's base is
    the first's tallies.  The tallies come from atomic adds, so the run is compared with itself, never with another run."""
    prob = make_problem(4000, num_iterations=2)
    nm, nt = prob.params.num_psd_mom_bins, len(prob.tcuts)
    hb = hip_backend(prob)
    try:
        L = hb.layout
        log10 = lambda a: hb.eval_fn("log10", a)
        tabs = mcs.consumers.consumer_tables(prob, 1)
        state, before = None, hb.read_tallies()[0]
        numbers = []
        for it in (1, 2):
            res = mcs.driver.run(prob, hb, n_itrs=1, first_iter=it, iter_state=state, max_pcuts=12, finalize=True, tcuts=True)
            state = res.iter_state
            (i_iter, i_ion, got), = res.tcuts
            after = hb.read_tallies()[0]
            want = mcs.consumers.tcut_spectra_host(L.view(after, "spectra_coupled")[0], L.view(before, "spectra_coupled")[0],
                                                   L.view(after, "weight_coupled")[0], tabs.mom_log_cgs, prob.tcuts, nm, log10)
            assert (i_iter, i_ion) == (it, 1)
            tc.assert_same(got, want, f"iteration {it}")
            assert got.diag[1] == 0 and got.diag[0] >= 3 and got.number[nt - 1] == 0.0
            ref = tc.reference(L.view(after, "spectra_coupled")[0], L.view(before, "spectra_coupled")[0], L.view(after, "weight_coupled")[0],
                               tabs.mom_log_cgs, prob.tcuts, nm, log10)
            tc.assert_same(got, ref, f"iteration {it}, the restatement")
            numbers.append(got.number)
            print(f"iteration {it}: live {int(got.diag[0])}, number {got.number.tolist()}, q50 {got.quantile[0].tolist()}, index {got.index.tolist()}")
            before = after
        assert np.any(L.view(before, "spectra_coupled")[0] > 0)
        live = (numbers[0] > 0) & (numbers[1] > 0)
        assert np.all(numbers[1][live] < 1.5 * numbers[0][live])          # a growth, not the running sum
    finally:
        hb.destroy()
