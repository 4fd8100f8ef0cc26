"""The products sample of the ensemble statistics without a GPU (include/mcs.h, "products sample"): the layout against the library,
the numpy accumulator (ensemble.HostEnsemble.add_products) fed by driver.run(finalize=True, ensemble=...) through the CPU oracle
against the restatement of ensemble_common.py and a slope written out again here in Python floats, the momentum window of a summary
range (bins=), and the stop rule on a products slot."""
import ctypes as ct
import math

import numpy as np
import pytest

from conftest import mcs, make_problem, oracle_backend
from ensemble_common import stat_of
from ens_summary_common import as_dict, assert_exact, assert_sums, restate

ens = mcs.ensemble
N_ITRS = 5
WINDOW = (60, 110)          # momentum bins of the slope fit: inside the accelerated tail of the downstream zones of this problem
DNDP = ("dNdp_sf", "dNdp_pf", "dNdp_isf")
SCALARS = ("P_psd_par", "P_psd_perp", "energy_density_psd")
SLOPES = ("slope_sf", "slope_pf", "slope_isf")
NAMES = DNDP + SCALARS + SLOPES


def same_words(a, b):
    """Bit-equal, where a NaN equals a NaN (the bits of a NaN that went through an update are nobody's promise)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def oracle_log10(be, values):
    a = np.ascontiguousarray(values, dtype=np.float64)
    out = np.zeros_like(a)
    dp = ct.POINTER(ct.c_double)
    assert be.lib.orc_eval_fn(mcs.capi.FN["log10"], a.size, a.ctypes.data_as(dp), a.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    return out


def slope_restated(row, l_lo, l_hi, x_log, log10):
    """The slope definition of include/mcs.h for one row of dN/dp, in plain Python floats and serial sums."""
    ls = [l for l in range(l_lo, l_hi) if float(row[l]) > 1.0e-99]
    k = len(ls)
    if k < 3:
        return float("nan")
    xs = [float(x_log[l]) for l in ls]
    ys = [float(v) for v in log10(np.array([row[l] for l in ls]))]
    sx = sy = 0.0
    for x, y in zip(xs, ys):
        sx = sx + x
        sy = sy + y
    xbar, ybar = sx / k, sy / k
    sxx = sxy = 0.0
    for x, y in zip(xs, ys):
        dx = x - xbar
        sxx = sxx + dx * dx
        sxy = sxy + dx * (y - ybar)
    return sxy / sxx


def parts_of(fin, slopes):
    """name -> array of the products sample of an IonFinal; slopes [3][n_grid]."""
    out = {name: np.asarray(fin.dNdp_cr[m], dtype=np.float64) for m, name in enumerate(DNDP)}
    out.update({name: np.asarray(getattr(fin, name), dtype=np.float64) for name in SCALARS})
    out.update({name: slopes[m] for m, name in enumerate(SLOPES)})
    return out


def test_layout_agrees_with_the_library():
    lib = mcs.capi.load_library()
    for name in ("mcs_ens_products_get_layout", "mcs_ens_set_slope_window", "mcs_ens_add_products"):
        assert hasattr(lib, name) and name in mcs.capi.EXPORTED_SYMBOLS, name
    for kw in ({}, dict(num_iterations=3, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(4.0, 2.0, 1e6, 0.1)])):
        P = make_problem(64, **kw).params
        E = mcs.capi.McsEnsProductsLayout()
        assert lib.mcs_ens_products_get_layout(ct.byref(P), ct.byref(E)) == 0
        got = {name: int(getattr(E, name)) for name, _ in E._fields_}
        mirror = ens.EnsLayout(P)
        assert got == mirror.products_fields
        ng, NM = P.n_grid, P.num_psd_mom_bins + 2
        assert got["total"] == mirror.products_total == 3 * ng * NM + 6 * ng and (got["dNdp_n"], got["zone_n"]) == (ng * NM, ng)
        sizes = [ng * NM] * 3 + [ng] * 6
        assert [got[n] for n in NAMES] == [sum(sizes[:k]) for k in range(9)]
        assert ens.PRODUCT_NAMES == NAMES
        for name, size in zip(NAMES, sizes):
            off, shape = mirror.products[name]
            assert off == got[name] and int(np.prod(shape)) == size and shape[0] == ng
        assert got["total"] % 256 != 0
    assert lib.mcs_ens_products_get_layout(None, ct.byref(E)) != 0 and b"mcs_ens_products_get_layout" in lib.mcs_last_error()
    assert lib.mcs_ens_add_products(None, None, 0) != 0 and b"null argument" in lib.mcs_last_error()
    assert lib.mcs_ens_set_slope_window(None, 0, 3, None) != 0 and b"null argument" in lib.mcs_last_error()


@pytest.fixture(scope="module")
def oracle_run():
    """N_ITRS iterations on the oracle with finalize and an ensemble whose slope window is WINDOW."""
    prob = make_problem(300, num_iterations=N_ITRS)
    be = oracle_backend(prob)
    e = ens.Ensemble.for_backend(be, 1)
    assert isinstance(e, ens.HostEnsemble)
    x_log = ens.bin_centres_log10(prob)
    e.set_slope_window(*WINDOW, x_log)
    res = mcs.driver.run(prob, be, n_itrs=N_ITRS, finalize=True, ensemble=e)
    fins = [fin for _, _, fin in res.iter_finals]
    log10 = lambda a: oracle_log10(be, a)
    slopes = [np.array([[slope_restated(fin.dNdp_cr[m][z], *WINDOW, x_log, log10) for z in range(prob.params.n_grid)] for m in range(3)])
              for fin in fins]
    yield prob, be, e, res, fins, [parts_of(fin, s) for fin, s in zip(fins, slopes)], x_log
    be.destroy()


def test_products_are_the_statistics_of_the_ion_finals(oracle_run):
    prob, be, e, res, fins, parts, x_log = oracle_run
    ps = e.products_slot(0)
    assert ps == 1 << 30 and e.names(ps) == NAMES and e.count(ps) == N_ITRS and e.count(0) == N_ITRS and len(fins) == N_ITRS
    want = stat_of(parts)
    denom = float(N_ITRS) * float(N_ITRS - 1)
    for name in NAMES:
        assert same_words(e.mean(ps, name), want.mean[name]), f"mean of {name}"
        assert same_words(e.m2(ps, name), want.m2[name]), f"M2 of {name}"
        with np.errstate(invalid="ignore"):
            assert same_words(e.stderr(ps, name), np.sqrt(want.m2[name] / denom)), f"stderr of {name}"
    # the package's own statistics of the IonFinals (what run_overlapped reports as finalize_mean / finalize_stderr)
    for name, of in (("dNdp_sf", lambda f: f.dNdp_cr[0]), ("dNdp_pf", lambda f: f.dNdp_cr[1]), ("dNdp_isf", lambda f: f.dNdp_cr[2]),
                     ("P_psd_par", lambda f: f.P_psd_par), ("P_psd_perp", lambda f: f.P_psd_perp), ("energy_density_psd", lambda f: f.energy_density_psd)):
        mean, err, n = ens.stats_over([of(f) for f in fins])
        assert n == N_ITRS and same_words(e.mean(ps, name), mean) and same_words(e.stderr(ps, name), err), name
    # the slopes: a strong shock's downstream spectrum, with an error bar
    z = prob.params.n_grid - 1
    slope, err = e.mean(ps, "slope_pf")[z], e.stderr(ps, "slope_pf")[z]
    print(f"slope of dN/dp in the plasma frame, last zone: {slope:.3f} +- {err:.3f}")
    assert -3.5 < slope < -1.5 and 0 < err < 0.5
    assert e.mean(ps, "dNdp_pf").shape == (prob.params.n_grid, prob.params.num_psd_mom_bins + 2) and e.mean(ps, "slope_isf").shape == (prob.params.n_grid,)


def test_too_few_bins_give_nan_which_no_trigger_meets(oracle_run):
    prob, be, e, res, fins, parts, x_log = oracle_run
    ps = e.products_slot(0)
    valid = np.array([(p["dNdp_pf"][:, WINDOW[0]:WINDOW[1]] > 1e-99).sum(axis=1) for p in parts])       # [iteration][zone]
    few = np.flatnonzero((valid < 3).any(axis=0))
    full = np.flatnonzero((valid >= 3).all(axis=0))
    assert few.size > 0 and full.size > 0          # (far upstream the accelerated population does not reach)
    slope = e.mean(ps, "slope_pf")
    assert np.all(np.isnan(slope[few])) and np.all(np.isfinite(slope[full]))
    # exactly three valid bins fit; two do not
    row = np.full(prob.params.num_psd_mom_bins + 2, 1e-99)
    row[[61, 70, 90]] = [1e-3, 1e-5, 1e-9]
    log10 = lambda a: oracle_log10(be, a)
    three = ens.slopes_of(row[None, :], *WINDOW, x_log, log10)
    assert np.isfinite(three[0]) and same_words(three, [slope_restated(row, *WINDOW, x_log, log10)])
    row[70] = 1e-99
    assert np.isnan(ens.slopes_of(row[None, :], *WINDOW, x_log, log10)[0]) and math.isnan(slope_restated(row, *WINDOW, x_log, log10))
    z = int(few[0])
    (s,) = e.summarize(ps, [ens.Request("slope_pf", (z, z + 1), 0.0)])
    assert s.n_nonfinite == 1 and s.n_selected == 0
    (s_all,) = e.summarize(ps, [ens.Request("slope_pf", None, 0.0)])
    assert s_all.n_nonfinite == few.size and s_all.n_selected == prob.params.n_grid - few.size
    t = ens.Trigger(ps, "slope_pf", "max", 1e9, zones=(z, z + 1), floor_frac=0.0)
    assert not t.met(s) and not ens.Trigger(ps, "slope_pf", "max", 1e9, floor_frac=0.0).met(s_all)
    zf = int(full[-1])
    (s_ok,) = e.summarize(ps, [ens.Request("slope_pf", (zf, zf + 1), 0.0)])
    assert s_ok.n_nonfinite == 0 and ens.Trigger(ps, "slope_pf", "max", 1e9, zones=(zf, zf + 1), floor_frac=0.0).met(s_ok)


def test_bins_is_a_word_range_of_one_zone(oracle_run):
    prob, be, e, res, fins, parts, x_log = oracle_run
    ps = e.products_slot(0)
    ng, NM, NT = prob.params.n_grid, prob.params.num_psd_mom_bins + 2, prob.params.num_psd_tht_bins + 2
    off_pf = e.layout.products["dNdp_pf"][0]
    assert off_pf == ng * NM
    assert e.word_range(ps, "dNdp_pf", (7, 8), (60, 110)) == (off_pf + 7 * NM + 60, 50)
    assert e.word_range(ps, "dNdp_pf", (ng - 1, ng), (0, NM)) == (off_pf + (ng - 1) * NM, NM)
    assert e.word_range(ps, "dNdp_pf", (3, 4), (5, 5)) == (off_pf + 3 * NM + 5, 0)
    assert e.word_range(ps, "dNdp_pf", (3, 5)) == (off_pf + 3 * NM, 2 * NM) and e.word_range(ps, "slope_sf", (3, 5)) == (3 * ng * NM + 3 * ng + 3, 2)
    off_mom, off_tht = e.layout.species["psd_mom"][0], e.layout.species["psd_tht"][0]
    assert e.word_range(0, "psd_mom", (2, 3), (10, 20)) == (off_mom + 2 * NM + 10, 10)
    assert e.word_range(0, "psd_tht", (2, 3), (1, NT)) == (off_tht + 2 * NT + 1, NT - 1)
    # Request's field order stands, bins appended
    assert ens.Request("psd", (0, 1), 0.5, 0.25) == ens.Request(name="psd", zones=(0, 1), floor_frac=0.5, tol=0.25, bins=None)
    assert ens.Request("dNdp_pf", (1, 2), 1e-3, 0.0, (3, 9)).bins == (3, 9)
    t = ens.Trigger(ps, "dNdp_pf", "max", 0.1, zones=(7, 8), bins=(60, 110))
    assert t.bins == (60, 110) and t.request.bins == (60, 110) and "bins=(60, 110)" in repr(t)
    e.check_trigger(t)
    # the summary of such a range is that of its words
    z = ng - 1
    mean, m2 = e.mean(ps, "dNdp_pf")[z, 70:100], e.m2(ps, "dNdp_pf")[z, 70:100]
    (s,) = e.summarize(ps, [ens.Request("dNdp_pf", (z, z + 1), 1e-3, 0.2, (70, 100))])
    want = restate(mean, m2, N_ITRS, 1e-3, 0.2)
    assert want["n_selected"] > 0
    assert_exact(as_dict(s), want, "bins 70..100")
    assert_sums(as_dict(s), want, "bins 70..100")
    # refused: bins without a single-zone slice, on a part with one word per zone (or no zone axis), bounds outside the axis
    for bad in (lambda: ens.Request("dNdp_pf", None, bins=(1, 5)), lambda: ens.Request("dNdp_pf", (1, 3), bins=(1, 5)),
                lambda: ens.Request("dNdp_pf", (1, 1), bins=(1, 5)), lambda: ens.Request("slope_pf", (1, 2), bins=(0, 1)),
                lambda: ens.Request("P_psd_par", (1, 2), bins=(0, 1)), lambda: ens.Request("pxx_flux", (1, 2), bins=(0, 1)),
                lambda: ens.Request("psd", (1, 2), bins=(0, 1)), lambda: ens.Request("esc_flux", None, bins=(0, 1)),
                lambda: ens.Request("dNdp_pf", (1, 2), bins=(1, 2, 3)), lambda: ens.Request("dNdp_pf", (1, 2), bins=(1.5, 3)),
                lambda: ens.Trigger(ps, "dNdp_pf", "max", 0.1, bins=(1, 5)), lambda: ens.Trigger(ps, "slope_sf", "max", 0.1, zones=(1, 2), bins=(0, 1)),
                lambda: e.word_range(ps, "dNdp_pf", (1, 2), (-1, 5)), lambda: e.word_range(ps, "dNdp_pf", (1, 2), (5, NM + 1)),
                lambda: e.word_range(ps, "dNdp_pf", (1, 2), (9, 5)), lambda: e.word_range(0, "psd_tht", (1, 2), (0, NT + 1)),
                lambda: e.word_range(ps, "dNdp_pf", (ng, ng + 1), (1, 5)),
                lambda: e.check_trigger(ens.Trigger(ps, "dNdp_pf", "max", 0.1, zones=(1, 2), bins=(0, NM + 1)))):
        with pytest.raises(ValueError):
            bad()
    # a products part is no part of a species slot, and the reverse; only a species slot has a products slot
    with pytest.raises(KeyError):
        e.word_range(0, "dNdp_pf")
    with pytest.raises(KeyError):
        e.word_range(ps, "psd_mom")
    for bad in (lambda: e.products_slot(1), lambda: e.products_slot(-1), lambda: e.count(e.products_slot(0) + 1), lambda: e.names((1 << 30) | 5)):
        with pytest.raises(ValueError):
            bad()


def _run(prob, window, **kw):
    be = oracle_backend(prob)
    e = ens.Ensemble.for_backend(be, 1)
    if window is not None:
        e.set_slope_window(*window, ens.bin_centres_log10(prob))
    try:
        return mcs.driver.run(prob, be, ensemble=e, **kw), e
    finally:
        be.destroy()


def test_driver_stops_on_a_products_trigger(oracle_run):
    prob, be, e_ref, res_ref, fins, parts, x_log = oracle_run
    z = prob.params.n_grid - 1
    ps = e_ref.products_slot(0)
    bins = (70, 100)
    # the trigger's value after every iteration, from the restated samples
    values = {}
    for n in range(2, N_ITRS + 1):
        st = stat_of([{"d": p["dNdp_pf"][z, bins[0]:bins[1]]} for p in parts[:n]])
        values[n] = restate(st.mean["d"], st.m2["d"], n, 1e-3, 0.0)["max_rel"]
    print("max relative error of dNdp_pf, last zone, bins 70..100, by iteration:", values)
    loose = ens.Trigger(ps, "dNdp_pf", "max", 10.0, zones=(z, z + 1), bins=bins)
    res, e = _run(prob, WINDOW, n_itrs=N_ITRS, finalize=True, triggers=[loose])
    c = res.convergence
    assert c.satisfied and c.stopped_at == 2 and [it for it, _ in c.checks] == [2] and e.count(ps) == 2 and len(res.iter_finals) == 2
    (row,) = c.checks[0][1]
    assert row.trigger is loose and row.met and row.summary.n == 2 and row.value == values[2]
    tight = ens.Trigger(ps, "dNdp_pf", "max", 1e-6, zones=(z, z + 1), bins=bins)
    res, e = _run(prob, WINDOW, n_itrs=N_ITRS, finalize=True, triggers=[tight])
    c = res.convergence
    assert not c.satisfied and c.stopped_at == N_ITRS and [it for it, _ in c.checks] == list(range(2, N_ITRS + 1)) and e.count(ps) == N_ITRS
    for it, (row,) in c.checks:
        assert not row.met and row.summary.n == it and row.value == values[it] and row.predicted_samples > N_ITRS
    # this run is the fixture's run again: the same products, bit for bit
    for name in NAMES:
        assert same_words(e.mean(ps, name), e_ref.mean(ps, name)) and same_words(e.m2(ps, name), e_ref.m2(ps, name)), name
    # without finalize no sample would ever arrive: refused before any iteration; a species-slot trigger needs no finalize
    ran = []
    with pytest.raises(ValueError, match="finalize"):
        _run(prob, WINDOW, n_itrs=2, finalize=False, triggers=[loose], on_iteration_end=ran.append)
    assert ran == []
    # an ensemble without a window gets one over all bins
    res, e = _run(prob, None, n_itrs=1, finalize=True)
    assert e.window[:2] == (0, prob.params.num_psd_mom_bins + 1) and np.array_equal(e.window[2], x_log) and e.count(ps) == 1
    # without finalize the products slot stays empty and unreadable
    res, e = _run(prob, None, n_itrs=1, max_pcuts=1)
    assert e.count(ps) == 0 and e.window is None
    with pytest.raises(ValueError, match="never taken a sample"):
        e.mean(ps, "dNdp_pf")


def _fed(prob, be, fins, x_log, window=WINDOW):
    e = ens.HostEnsemble(prob.params, 1)
    if window is not None:
        e.set_slope_window(*window, x_log)
    for fin in fins:
        e.add_products(be, 0, fin)
    return e


def test_merge_is_chans_on_the_products_slots(oracle_run):
    prob, be, e_ref, res, fins, parts, x_log = oracle_run
    ps = e_ref.products_slot(0)
    a, b = _fed(prob, be, fins[:3], x_log), _fed(prob, be, fins[3:], x_log)
    wa, wb = stat_of(parts[:3]), stat_of(parts[3:])
    with np.errstate(invalid="ignore"):
        merged = wa.merged_with(wb)
    # the merged summary, before the merge changes a
    reqs = [ens.Request("dNdp_pf", (98, 99), 1e-3, 0.1, (70, 100)), ens.Request("P_psd_par"), ens.Request("slope_pf", (90, 99), 0.0)]
    got = a.summarize_merged([b], ps, reqs)
    a.merge(b)
    assert a.count(ps) == 5 and b.count(ps) == 2 and a.count(0) == 0
    for name in NAMES:
        assert same_words(a.mean(ps, name), merged.mean[name]) and same_words(a.m2(ps, name), merged.m2[name]), name
        assert same_words(b.mean(ps, name), wb.mean[name]) and same_words(b.m2(ps, name), wb.m2[name]), name
    assert got == a.summarize(ps, reqs)
    # an empty ensemble takes the source, and its window, as it is; an empty source changes nothing
    empty = ens.HostEnsemble(prob.params, 1)
    empty.merge(b)
    b.merge(ens.HostEnsemble(prob.params, 1))
    assert empty.count(ps) == 2 and b.count(ps) == 2 and empty.window[:2] == WINDOW
    for name in NAMES:
        assert same_words(empty.mean(ps, name), wb.mean[name]) and same_words(b.m2(ps, name), wb.m2[name]), name


def test_slope_windows_must_agree_and_stay(oracle_run):
    prob, be, e_ref, res, fins, parts, x_log = oracle_run
    ps = e_ref.products_slot(0)
    a = _fed(prob, be, fins[:2], x_log)
    other_bounds = _fed(prob, be, fins[2:4], x_log, (61, 110))
    x2 = x_log.copy()
    x2[3] = np.nextafter(x2[3], 1.0)
    other_word = _fed(prob, be, fins[2:4], x2)
    for o in (other_bounds, other_word):
        with pytest.raises(ValueError, match="slope windows differ"):
            a.merge(o)
        with pytest.raises(ValueError, match="slope windows differ"):
            a.summarize_merged([o], ps, [ens.Request("P_psd_par")])
    assert a.count(ps) == 2 and same_words(a.mean(ps, "dNdp_pf"), stat_of(parts[:2]).mean["dNdp_pf"])
    with pytest.raises(ValueError, match="window"):
        a.set_slope_window(*WINDOW, x_log)                 # after the first sample
    with pytest.raises(ValueError, match="window"):
        ens.HostEnsemble(prob.params, 1).add_products(be, 0, fins[0])      # without one
    fresh = ens.HostEnsemble(prob.params, 1)
    for bad in ((-1, 5), (0, prob.params.num_psd_mom_bins + 2), (5, 7)):
        with pytest.raises(ValueError, match="window"):
            fresh.set_slope_window(*bad, x_log)
    with pytest.raises(ValueError):
        fresh.set_slope_window(0, 5, x_log[:-1])
    with pytest.raises(ValueError):
        fresh.add_products(be, 1, fins[0])                  # the iteration slot
    # slope_window: the bins whose centre lies between two momenta
    l_lo, l_hi, x = ens.slope_window(prob, 10.0 ** x_log[60] * 0.9999, 10.0 ** x_log[109] * 1.0001)
    assert (l_lo, l_hi) == WINDOW and np.array_equal(x, x_log)
    mb = np.asarray(prob.psd_mom_bounds)
    assert np.allclose(10.0 ** x_log[1:], 10.0 ** (0.5 * (mb[1:-1] + mb[2:])) * mcs.constants.MP * mcs.constants.C, rtol=1e-13)
    with pytest.raises(ValueError):
        ens.slope_window(prob, 10.0 ** x_log[60], 10.0 ** x_log[61])
