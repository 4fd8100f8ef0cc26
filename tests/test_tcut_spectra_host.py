"""The time-cut spectra without a GPU: the entry points and layouts (include/mcs.h, mcs_tcut_spectra and "tcuts sample"), the numpy
path of consumers.tcut_spectra against the restatement of tests/tcuts_common.py word for word on every crafted case, the tcuts slots of
HostEnsemble, every refusal of the ensembles and of driver.run / run_overlapped, and one run on the oracle backend."""
import ctypes as ct
import os

import numpy as np
import pytest

import consumers_common as cc
import tcuts_common as tc
from conftest import ROOT, mcs, make_problem, oracle_backend

ens = mcs.ensemble
BINNINGS = {"stock": {}, "largest": cc.LARGE_BINNING}


# ---- (a) the ABI and the layouts -----------------------------------------------------------------------------------------------------
def test_entry_points_and_layouts():
    lib = mcs.capi.load_library()
    for name in ("mcs_tcut_spectra", "mcs_tcut_get_layout", "mcs_ens_tcuts_get_layout", "mcs_ens_add_tcuts"):
        assert hasattr(lib, name) and name in mcs.capi.EXPORTED_SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "mcs.h")).read()
    assert "#define MCS_ENS_TCUTS(s) ((s) | (1 << 25))" in header and mcs.capi.ENS_TCUTS_BIT == 1 << 25
    assert "#define MCS_TCUT_Q {0.5, 0.9, 0.99}" in header and mcs.capi.TCUT_Q == tc.Q == mcs.consumers.TCUT_Q
    for kw in (cc.SMALL_BINNING, cc.LARGE_BINNING, {}):
        P = make_problem(64, **kw).params
        NM = P.num_psd_mom_bins + 2
        for nt in (1, 3, 10, 99):
            # hand-counted: nt rows of NM, then three vectors of nt, three quantile rows of nt, three indices
            want = dict(spectrum=0, weight=nt * NM, number=nt * NM + nt, mean_log_p=nt * NM + 2 * nt, quantile=nt * NM + 3 * nt,
                        index=nt * NM + 6 * nt, row_n=NM, n_tcuts=nt, total=nt * (NM + 6) + 3)
            for fn in (lib.mcs_tcut_get_layout, lib.mcs_ens_tcuts_get_layout):
                X = mcs.capi.McsTcutLayout()
                assert fn(ct.byref(P), nt, ct.byref(X)) == 0
                assert {name: int(getattr(X, name)) for name, _ in X._fields_} == want, (fn, nt)
            mirror = ens.EnsLayout(P)
            assert mirror.tcuts_fields(nt) == want
            assert mirror.tcuts(nt) == {"spectrum": (0, (nt, NM)), "weight": (nt * NM, (nt,)), "number": (nt * NM + nt, (nt,)),
                                        "mean_log_p": (nt * NM + 2 * nt, (nt,)), "quantile": (nt * NM + 3 * nt, (3, nt)),
                                        "index": (nt * NM + 6 * nt, (3,))}
    assert NM == 157
    X = mcs.capi.McsTcutLayout()
    for bad in (0, -1, 100):
        assert lib.mcs_tcut_get_layout(ct.byref(P), bad, ct.byref(X)) != 0 and b"n_tcuts outside 1..99" in lib.mcs_last_error()
        with pytest.raises(ValueError, match="n_tcuts outside"):
            mcs.capi.tcut_layout(P, bad)
    assert lib.mcs_ens_tcuts_get_layout(None, 3, ct.byref(X)) != 0 and b"mcs_ens_tcuts_get_layout" in lib.mcs_last_error()
    assert lib.mcs_tcut_get_layout(ct.byref(P), 3, None) != 0


def test_no_context_no_spectra():
    lib = mcs.capi.load_library()
    prob = make_problem(64)
    s = mcs.consumers.consumer_tables(prob, 1).as_struct()
    out = np.zeros(mcs.capi.tcut_layout(prob.params, len(prob.tcuts)).total)
    assert lib.mcs_tcut_spectra(None, ct.byref(s), out.ctypes.data_as(mcs.capi.c_double_p), None) != 0 and not out.any()
    assert lib.mcs_ens_add_tcuts(None, None, 0) != 0 and b"mcs_ens_add_tcuts" in lib.mcs_last_error()


# ---- (b) the numpy path against the restatement ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(BINNINGS))
def oracle_ctx(request):
    prob = tc.two_ion_problem(make_problem, **BINNINGS[request.param])
    assert prob.params.n_ions == 2 and prob.params.do_tcuts
    if request.param == "largest":
        assert prob.params.num_psd_mom_bins == 199
    return prob, oracle_backend(prob)


def test_numpy_path_equals_the_restatement(oracle_ctx):
    """Every crafted scenario (n_tcuts 1, 3, 99; the species is the second of two), word for word."""
    prob, ob = oracle_ctx
    nm = prob.params.num_psd_mom_bins
    log10 = ens._det_log10(ob)
    tabs = mcs.consumers.consumer_tables(prob, 2)
    seen_dead = seen_nan_index = seen_index = 0
    for name, rows in tc.scenarios(nm).items():
        now, base, weight, block = tc.load_rows(ob, prob, 2, rows)
        ref = tc.reference(now, base, weight, tabs.mom_log_cgs, prob.tcuts, nm, log10)
        got = mcs.consumers.tcut_spectra(prob, ob, 2, base=block)
        tc.assert_same(got, ref, name)
        assert tc.same_words(got.words(), ref.words()) and not ref.f_is_one
        assert ref.diag[1] == 0 and np.all(np.isfinite(got.spectrum)) and np.all(np.isfinite(got.weight))
        seen_dead += int((ref.number == 0.0).sum())
        seen_nan_index += int(np.isnan(ref.index).all())
        seen_index += int(np.isfinite(ref.index).all())
    assert seen_dead > 100 and seen_nan_index >= 5 and seen_index >= 3


def test_the_crafted_rows_are_what_they_claim(oracle_ctx):
    """The properties the crafted rows exist for, read off the restatement (so that a change of a builder cannot empty a case)."""
    prob, ob = oracle_ctx
    nm = prob.params.num_psd_mom_bins
    e = mcs.consumers.consumer_tables(prob, 2).mom_log_cgs
    R = tc.crafted_rows(nm)
    one = lambda name: tc.reference([R[name][1]], [R[name][0]], [R[name][2]], e, tc.tcuts_for(prob, 1), nm, ens._det_log10(ob))
    for name, l in (("one_bin_first", 0), ("one_bin_last", nm), ("one_bin_middle", nm // 2)):
        r = one(name)
        assert r.number[0] > 0 and r.spectrum[0, l] == 1.0 and (r.spectrum[0] > 1e-99).sum() == 1
        assert np.all((r.quantile[:, 0] > e[l]) & (r.quantile[:, 0] < e[l + 1])) and np.all(np.diff(r.quantile[:, 0]) > 0)
    for j in range(3):                       # the tie: the quantile is the upper edge of the first lit bin, f = 1 exactly
        r = one(f"tie_q{j}")
        assert r.quantile[j, 0] == e[2] + 1.0 * (e[3] - e[2])
    r = one("now_equals_base")
    assert r.number[0] == 0.0 and np.all(r.spectrum == 1e-99) and np.isnan(r.mean_log_p[0]) and np.all(np.isnan(r.quantile)) and r.diag[0] == 0
    assert r.weight[0] == 1e-99 and one("one_bin_middle").weight[0] == 1e-60 and one("one_bin_last").weight[0] == tc.up(1e-60)
    r = one("one_ulp_of_base")
    assert r.number[0] == 2.0 ** -52 and r.spectrum[0, nm // 2 + 1] == 1.0
    assert one("floor_base_real_deposits").diag.tolist() == [1, 0]
    r = one("around_1e-60")
    assert r.number[0] == 1.0 and r.spectrum[0, 4] == 1e-60 and r.spectrum[0, 5] == 1e-99 and r.spectrum[0, 6] == tc.up(1e-60) and r.spectrum[0, nm - 1] == 1e-99
    assert one("number_at_1e-99").number[0] == 0.0 and one("number_below_1e-99").number[0] == 0.0 and one("number_above_1e-99").number[0] == tc.up(1e-99)


def test_the_f_is_one_rule_is_never_met():
    """The header's fall-back for a row where the last lit bin's C falls short of T through rounding (l* that bin, f = 1.0) has no
    row to be tested on.  There is none: C after the last bin is the same serial sum as number, and T = fl(q * number) <= number for
    q < 1, so the bin that completes the sum always meets T.  The search below (random rows over 30 decades, sparse and dense, with
    every q) finds none either; the rule stays in the kernel and in the restatement as the answer to a row that cannot occur."""
    rng = np.random.default_rng(5)
    nm = 40
    e = np.linspace(-20.0, -10.0, nm + 2)
    for trial in range(3000):
        g = rng.uniform(0.5, 1.5, nm + 1) * 10.0 ** rng.uniform(-15, 15, nm + 1) * (rng.random(nm + 1) < rng.uniform(0.05, 1.0))
        num = 0.0
        for v in g:
            num = num + float(v)
        if not num > 1e-99:
            continue
        for q in tc.Q:
            assert not tc.quantile_of([float(v) for v in g], e, nm, q * num)[1]


# ---- (c) the tcuts slots of the numpy ensemble -------------------------------------------------------------------------------------------
def crafted_spectra(prob, ob, names=("99_cuts_every_row", "99_cuts_three_live_apart", "99_cuts_two_live_apart")):
    out = []
    for name in names:
        _, _, _, block = tc.load_rows(ob, prob, 2, tc.scenarios(prob.params.num_psd_mom_bins)[name])
        out.append(mcs.consumers.tcut_spectra(prob, ob, 2, base=block))
    return out


def test_host_ensemble_tcuts_slot(oracle_ctx):
    prob, ob = oracle_ctx
    NM = prob.params.num_psd_mom_bins + 2
    samples = crafted_spectra(prob, ob)
    e = ens.HostEnsemble(prob.params, 2)
    s = e.tcuts_slot(1)
    assert s == 1 | (1 << 25) and e.is_tcuts(s) and not e.is_tcuts(e.angles_slot(1)) and not e.is_angles(s) and not e.is_escape(s)
    assert not e.is_tcuts(e.photons_all_slot) and not e.is_tcuts(1) and e.count(s) == 0
    assert e.tcuts_row(4) == (4, 5)
    with pytest.raises(ValueError, match="no sample yet"):
        e.word_range(s, "number")
    for x in samples:
        e.add_tcuts(ob, 1, x)
    assert e.count(s) == 3 and e.count(e.tcuts_slot(0)) == 0 and e.tcuts_n == 99 and e.names(s) == ens.TCUTS_NAMES
    with np.errstate(invalid="ignore"):
        mean, err, n = ens.stats_over([x.words() for x in samples])
    lay = ens.EnsLayout(prob.params).tcuts(99)
    for name in ens.TCUTS_NAMES:
        off, shape = lay[name]
        cnt = int(np.prod(shape))
        assert tc.same_words(e.mean(s, name).ravel(), mean[off:off + cnt]), name
        assert tc.same_words(e.stderr(s, name).ravel(), err[off:off + cnt]), name
    assert e.word_range(s, "spectrum", zones=e.tcuts_row(7), bins=(3, 20)) == (7 * NM + 3, 17)
    assert e.word_range(s, "quantile", zones=(1, 2), bins=e.tcuts_row(50)) == (99 * NM + 3 * 99 + 99 + 50, 1)
    assert e.word_range(s, "mean_log_p", zones=e.tcuts_row(98)) == (99 * NM + 2 * 99 + 98, 1)
    # a live row in every sample has error bars; a row that was dead in one sample stays non-finite and no trigger on it is met
    got = e.summarize(s, [ens.Request("quantile", zones=(0, 1), bins=e.tcuts_row(0)), ens.Request("quantile", zones=(0, 1), bins=e.tcuts_row(50))])
    assert got[0].n_nonfinite == 0 and got[0].n_selected == 1 and got[1].n_nonfinite == 1
    dead, alive = (ens.Trigger(s, "quantile", "max", 1e30, zones=(0, 1), bins=e.tcuts_row(k)) for k in (50, 0))
    e.check_trigger(dead); e.check_trigger(alive)
    assert not dead.met(e.summarize(s, [dead.request])[0]) and alive.met(e.summarize(s, [alive.request])[0])


def test_ensemble_refusals(oracle_ctx):
    prob, ob = oracle_ctx
    three, = crafted_spectra(prob, ob, ("three_cuts_three_live",))
    many, = crafted_spectra(prob, ob, ("99_cuts_every_row",))
    a, b = ens.HostEnsemble(prob.params, 2), ens.HostEnsemble(prob.params, 2)
    with pytest.raises(ValueError, match="only a species slot"):
        a.tcuts_slot(2)
    with pytest.raises(ValueError, match="a tcuts slot"):
        a.add_tcuts(ob, 2, three)
    with pytest.raises(ValueError, match="from a TcutSpectra"):
        a.add_tcuts(ob, 0, None)
    for _ in range(2):
        a.add_tcuts(ob, 0, three)
        b.add_tcuts(ob, 0, many)
    with pytest.raises(ValueError, match="99 time cuts, the ensemble's tcuts samples have 3"):
        a.add_tcuts(ob, 1, many)
    with pytest.raises(ValueError, match="99 time cuts"):
        a.expect_tcuts(99)
    a.expect_tcuts(3)
    with pytest.raises(ValueError, match="differ in the number of time cuts"):
        a.merge(b)
    req = ens.Request("number")
    with pytest.raises(ValueError, match="differ in the number of time cuts"):
        a.summarize_merged([b], a.tcuts_slot(0), [req])
    with pytest.raises(ValueError, match="differ in the number of time cuts"):
        a.compare(b, a.tcuts_slot(0), [ens.CompareRequest("number")])
    with pytest.raises((ValueError, KeyError)):
        a.word_range(a.tcuts_slot(0), "dNdp")
    with pytest.raises(ValueError, match="outside"):
        a.word_range(a.tcuts_slot(0), "number", zones=a.tcuts_row(3))
    # ... and what is allowed: a merge into an ensemble that has none takes the source's number of cuts
    c = ens.HostEnsemble(prob.params, 2)
    c.merge(a)
    assert c.tcuts_n == 3 and c.count(c.tcuts_slot(0)) == 2
    d = a.compare(c, a.tcuts_slot(0), [ens.CompareRequest("number")])[0]
    assert d.max_abs_z == 0.0


def test_driver_refusals():
    prob = make_problem(64)
    ob = oracle_backend(prob)
    run = mcs.driver.run
    with pytest.raises(ValueError, match="tcuts: needs finalize=True"):
        run(prob, ob, n_itrs=1, max_pcuts=1, tcuts=True)
    with pytest.raises(ValueError, match="tcuts: not with tcut_print"):
        run(prob, ob, n_itrs=1, max_pcuts=1, finalize=True, tcuts=True, tcut_print=True)
    e = ens.HostEnsemble(prob.params, 1)
    with pytest.raises(ValueError, match="a trigger on a tcuts slot needs tcuts=True"):
        run(prob, ob, n_itrs=2, max_pcuts=1, finalize=True, ensemble=e, triggers=[ens.Trigger(e.tcuts_slot(0), "number", "max", 0.1)])

    class FakeComm:
        enabled, rank, world = True, 0, 1
    with pytest.raises(ValueError, match="communicator"):
        run(prob, ob, comm=FakeComm(), n_itrs=1, max_pcuts=1, finalize=True, tcuts=True)
    with pytest.raises(ValueError, match="tcuts: the overlapped run leaves the time-cut spectra out"):
        mcs.driver.run_overlapped(prob, [ob], n_itrs=1, tcuts=True)
    with pytest.raises(ValueError, match="tcuts: the overlapped run leaves the time-cut spectra out"):
        mcs.driver.run_overlapped(prob, [ob], n_itrs=2, ensemble=True, triggers=[ens.Trigger(e.tcuts_slot(0), "number", "max", 0.1)])
    with pytest.raises(ValueError, match="needs the base"):
        mcs.consumers.tcut_spectra(prob, ob, 1)
    none = make_problem(64, TCUTS=None)
    assert not none.params.do_tcuts
    nb = oracle_backend(none)
    with pytest.raises(ValueError, match="tcuts: the problem tracks no time cuts"):
        run(none, nb, n_itrs=1, max_pcuts=1, finalize=True, tcuts=True)
    with pytest.raises(ValueError, match="tracks no time cuts"):
        mcs.consumers.tcut_spectra(none, nb, 1, base=np.zeros((100, 201)))


# ---- (d) one run on the oracle backend ---------------------------------------------------------------------------------------------------
def test_one_run_on_the_oracle_backend():
    """driver.run(finalize=True, tcuts=True) with the numpy path: in iteration 1, for every live row, number[k] agrees with
    weight_coupled[k] -- the same positive deposits summed in another order -- within (deposits + NM + 1) * 2^-53 relative, the
    deposits bounded by the run's helix-step counter (tcut_track runs once per step; the counter, 2e7 here, exceeds particles x cuts
    a hundredfold).  The second iteration's spectra are again a growth: their numbers are those of one iteration, not of two."""
    prob = make_problem(4000, num_iterations=2)
    ob = oracle_backend(prob)
    e = ens.HostEnsemble(prob.params, 1)
    res = mcs.driver.run(prob, ob, n_itrs=2, max_pcuts=12, finalize=True, tcuts=True, ensemble=e)
    assert [(it, ion) for it, ion, _ in res.tcuts] == [(1, 1), (2, 1)] and e.count(e.tcuts_slot(0)) == 2
    L = ob.layout
    NM = prob.params.num_psd_mom_bins + 2
    (_, _, first), (_, _, second) = res.tcuts
    (it, ion, f1, i1) = res.per_species[0]
    assert (it, ion) == (1, 1)
    steps = int(i1[prob.params.n_grid + mcs.capi.IC["STEPS_HELIX"]])
    wc = L.view(f1, "weight_coupled")[0][:len(prob.tcuts)]
    live = first.number > 1e-99
    bound = (steps + NM + 1) * 2.0 ** -53
    rel = np.abs(first.number[live] - wc[live]) / wc[live]
    print(f"steps {steps}, live rows {int(live.sum())} of {len(live)}, bound {bound:.3e}, largest relative difference {rel.max():.3e}")
    print("number", first.number.tolist()); print("weight_coupled", wc.tolist())
    assert live.sum() >= 3 and not live[-1] and first.diag.tolist() == [int(live.sum()), 0] and second.diag[1] == 0
    assert np.all(rel <= bound)
    assert tc.bits_equal(first.weight, np.where(wc < 1e-60, 1e-99, wc))
    # growth, not the running sum: iteration 2's numbers are of the size of iteration 1's
    both = (first.number > 1e-99) & (second.number > 1e-99)
    assert both.sum() >= 3 and np.all(second.number[both] < 1.5 * first.number[both])
    sc2 = L.view(res.per_species[1][2], "spectra_coupled")[0]
    assert sc2[0, :NM - 1].sum() > 1.5 * first.number[0]            # (while the tally itself holds both iterations)
    assert np.all(np.diff(first.quantile[:, live], axis=0) >= 0)      # the 50, 90, 99 % momenta are ordered
    assert np.isfinite(first.index).all()
    assert tc.same_words(e.mean(e.tcuts_slot(0), "number"), ens.stats_over([first.number, second.number])[0])
