"""The shock-profile update (K13; include/mcs.h, mcs_profile_update) on the CPU: the numpy statement consumers.profile_update_host
against the plain-Python restatement of the header (tests/profile_common.py) on crafted inputs, against the host's iter_finalize and
its C++ twin on a real iteration, the profile slot of the numpy ensemble, the refusals, and driver.run(profile=True)."""
import copy
import ctypes as ct

import numpy as np
import pytest

from conftest import mcs, orc, make_problem, oracle_backend
import profile_common as pc

ens = mcs.ensemble
cons = mcs.consumers
itf = mcs.iter_finalize
dp = ct.POINTER(ct.c_double)


def pin_of(c):
    return cons.ProfileIn(**{k: c[k] for k in cons.PROFILE_SETTINGS}, hist_q_px=c["hist_q_px"], hist_q_en=c["hist_q_en"],
                          pxx_EM=c["pxx_EM"], en_EM=c["en_EM"], atan_x=c["atan_x"])


def host_update(prob, c):
    return cons.profile_update_host(pin_of(c), prob.params, c["ux"], c["gam_sf"], c["x_grid_cm"], c["pxx_flux"], c["energy_flux"], c["scalars"],
                                    c["P_par"], c["P_perp"], c["e_dens"])


@pytest.fixture(scope="module")
def branches():
    """{branch: (prob, [(name, case, restatement)])}, made once."""
    out = {}
    for branch, prob in (("rel", make_problem(64)), ("cls", pc.classical_problem())):
        out[branch] = (prob, [(name, c, pc.restate(c)) for name, c in pc.make_cases(prob)])
    return out


def test_entry_points_and_layout():
    lib = mcs.capi.load_library()
    for name in ("mcs_profile_update", "mcs_profile_get_layout", "mcs_ens_profile_get_layout", "mcs_ens_add_profile"):
        assert hasattr(lib, name) and name in mcs.capi.EXPORTED_SYMBOLS, name
    prob = make_problem(64)
    n = prob.n_grid
    L = mcs.capi.profile_layout(prob.params)       # needs no GPU
    assert [getattr(L, k) for k in pc.ROWS] == [k * n for k in range(10)] and L.scalars == 10 * n
    assert (L.row_n, L.n_scalars, L.total) == (n, 8, 10 * n + 8)
    E = mcs.capi.McsProfileLayout()
    assert lib.mcs_ens_profile_get_layout(ct.byref(prob.params), ct.byref(E)) == 0 and bytes(E) == bytes(L)
    assert ens.EnsLayout(prob.params).profile_fields() == {k: getattr(L, k) for k, _ in L._fields_}
    assert lib.mcs_profile_get_layout(None, ct.byref(E)) != 0 and b"mcs_profile_get_layout" in lib.mcs_last_error()
    assert cons.PROFILE_ROWS == pc.ROWS == ens.PROFILE_ROW_NAMES and cons.PROFILE_SCALARS == pc.SCALARS == ens.PROFILE_SCALAR_NAMES
    assert ens.PROFILE_SLOT == 1 << 24


@pytest.mark.parametrize("branch", ["rel", "cls"])
def test_numpy_statement_equals_the_restatement(branches, branch):
    """Every crafted case, every output word and the three counts; a NaN matches a NaN."""
    prob, cases = branches[branch]
    assert len(cases) >= 9
    for name, c, ref in cases:
        got = host_update(prob, c)
        assert pc.same_words(got.words(), ref.words()), (name, pc.first_difference(got.words(), ref.words(), c["n_grid"]))
        assert np.array_equal(got.diag, ref.diag), (name, got.diag, ref.diag)
        assert pc.same_words(got.ux_next, ref.row("ux_next")) and (got.shift_rms == ref.scalars[7] or ref.scalars[7] != ref.scalars[7])


def test_the_crafted_cases_are_what_they_claim(branches):
    """The properties the cases exist for, read off the restatement (so that a change of a builder cannot empty a case)."""
    for branch in ("rel", "cls"):
        prob, cases = branches[branch]
        by = {name[4:]: (c, ref) for name, c, ref in cases}
        n = prob.n_grid
        c, ref = by["base"]
        assert ref.diag[0] == 0 and np.all(np.diff(ref.row("ux_pred")) <= 0) and ref.scalars[0] == 1.4
        assert (ref.diag[2] == 0) == (branch == "rel")
        c, ref = by["ties"]
        fp = ref.row("flux_px") * c["F_px_upstream"]
        assert fp[3] == 2.0e-13 / c["F_px_upstream"] * c["F_px_upstream"] and abs(fp[4] - 4.0e-13) < 1e-27 and fp[5] < 0 and fp[6] == 0.0 and fp[7] == 0.0
        assert abs(fp[8] + 4.0e-13) < 1e-27 and fp[9] == 0.0          # 2.5 -> 2, 3.5 -> 4, -4.5 -> -4, 0.5 -> 0: ties to even
        assert ref.scalars[5] != ref.scalars[3] and len(c["hist_q_px"]) == 1
        c, ref = by["edens"]
        assert ref.row("gamma_ad")[2] == 1.0e-99 and np.isinf(ref.row("gamma_ad")[3]) and np.isnan(ref.row("p_flux")[3]) and ref.diag[0] > 0
        assert c["i_trans"] == 2 and c["w"] == 10.35
        c, ref = by["last_ten"]
        assert c["i_trans"] == 0
        c, ref = by["K_sign"]
        assert ref.scalars[3] == 0.0 and ref.scalars[4] == 0.0
        assert by["increasing"][0]["i_trans"] == prob.params.i_shock and len(by["monotone"][0]["hist_q_px"]) == 3
        assert {by[k][0]["SMMOE"] for k in by} >= {0.0, 0.4, 1.0} and {by[k][0]["SMPFP"] for k in by} >= {0.0, 0.3, 1.0}
        assert {by[k][0]["w"] for k in by} >= {0.0, 1.0, 10.35}
    by = {name[4:]: (c, ref) for name, c, ref in branches["rel"][1]}
    c, ref = by["first_equals_avg"]
    up = np.asarray(c["x_grid_cm"])[1:c["n_grid"] + 1] < 0
    assert np.all(np.isnan(ref.row("ux_px")[up])) and np.all(ref.row("ux_px")[~up] == c["u2"])      # (u0 - u2) / 0: every zone that is not pinned
    assert ref.diag[0] >= 4 * int(up.sum())          # ux_px, ux_pred, ux_next and shift of those zones at least
    c, ref = by["K_sign"]
    # before smoothing and rescale the K < 0 zone has a negative root, the K == 0 zone the root 0: seen in the final row as the step
    assert ref.diag[0] == 0
    c, ref = by["increasing"]       # the raw momentum row rises towards the shock: the descending pass flattens all of it
    up = np.asarray(c["x_grid_cm"])[1:c["n_grid"] + 1] < 0
    assert np.ptp(ref.row("ux_px")[up][:-2]) <= 1e-6 * c["u0"]
    by = {name[4:]: (c, ref) for name, c, ref in branches["cls"][1]}
    c, ref = by["newton_runs_out"]
    assert tuple(ref.diag[1:]) == (1, pc.NEWTON_MAX) and np.isnan(ref.row("ux_px")[7]) and ref.row("ux_en")[7] == ref.row("ux_en")[7]
    assert by["base"][1].diag[1] == 0 and 3 <= by["base"][1].diag[2] < 100


def test_last_ten_sum_depends_on_the_order(branches):
    """The last-ten case: summed descending, the average differs in some bit, so a kernel that reduced it in another order would show."""
    for branch in ("rel", "cls"):
        (c, ref), = [(c, ref) for name, c, ref in branches[branch][1] if name.endswith("last_ten")]
        d = copy.deepcopy(c)
        for k in ("pxx_EM", "en_EM"):
            d[k][-10:] = c[k][-10:][::-1].copy()        # the same ten values, the other way round
        other = pc.restate(d)
        up = np.asarray(c["x_grid_cm"])[1:c["n_grid"] + 1] < 0
        a, b = ref.row("ux_px")[up], other.row("ux_px")[up]
        e, f = ref.row("ux_en")[up], other.row("ux_en")[up]
        assert not (np.array_equal(a, b) and np.array_equal(e, f))


# ---- a real iteration ---------------------------------------------------------------------------------------------------------------
def _p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(dp)


def _twin_ux(lib, prob, st, sm, w, pxx, en, q_px, q_en, P_tot):
    """oracle/mcs_iter.cpp:orc_smooth_grid_par on copies of the tables -> the new ux table"""
    P, cfg = prob.params, prob.cfg
    t = {k: np.ascontiguousarray(getattr(prob, k)).copy() for k in ("ux", "gam_sf", "utot", "beta_ef", "gam_ef", "btot")}
    n0_aa = float(sum(s.density * s.aa for s in cfg.species))
    ux_new = np.zeros(P.n_grid)
    rc = lib.orc_smooth_grid_par(P.n_grid, P.i_shock, _p(np.ascontiguousarray(prob.x_grid_rg)), _p(t["ux"]), _p(t["gam_sf"]), _p(t["utot"]),
                                 _p(t["beta_ef"]), _p(t["gam_ef"]), _p(t["btot"]), _p(np.ascontiguousarray(prob.theta)),
                                 _p(np.ascontiguousarray(st.Gamma_grid[:, 1])), _p(np.ascontiguousarray(pxx)), _p(np.ascontiguousarray(en)),
                                 _p(np.ascontiguousarray(P_tot)), q_px, q_en, st.F_px_upstream, st.F_energy_upstream, n0_aa,
                                 P.u0, P.beta0, P.gam0, P.u2, sm.SMMOE, sm.SMPFP, w,
                                 sm.artificial_smoothing_start_rg, cfg.B_mag_upstream, cfg.b_field_turbulence, cfg.b_field_amplify, _p(ux_new))
    assert rc == 0
    return t["ux"]


@pytest.fixture(scope="module")
def one_iteration():
    prob = make_problem(2500)
    be = oracle_backend(prob, nthreads=8)
    res = mcs.driver.run(prob, be, None, n_itrs=1, finalize=True)
    (_, fin, ion), = res.iter_finals
    return prob, be, res, ion


SEEN = {}


@pytest.mark.parametrize("variant", ["momentum", "energy-mix", "artificial", "damped"])
def test_ux_next_agrees_with_iter_finalize_and_the_twin(one_iteration, variant):
    """On a real oracle-backend iteration (2500 protons) ux_next is what iter_finalize -> smooth_grid_par writes into a copy of prob,
    and what the C++ twin writes, within the twin tolerance of tests/test_iter_finalize.py: rtol 1e-11.  The statement here is not
    bit-equal to the host file (products for powers); the largest relative difference seen is printed (run with -s)."""
    prob, be, res, ion = one_iteration
    sm = {"momentum": itf.SmoothingConfig(), "energy-mix": itf.SmoothingConfig(SMMOE=0.4),
          "artificial": itf.SmoothingConfig(artificial_smoothing_start_rg=-3.0),
          "damped": itf.SmoothingConfig(old_profile_weight=2.5, increase_old_profile_weighting=True)}[variant]
    i_iter = 2 if variant == "damped" else 1
    n = prob.n_grid
    pres = (ion.P_psd_par, ion.P_psd_perp, ion.energy_density_psd)
    st = itf.IterState.create(prob, sm, 3)
    history = [(0.0, 0.0)] if i_iter == 2 else None             # (what a fresh state's iteration 1 left: iter_finalize averages it in)
    before = (prob.ux.copy(), be.read_tallies()[0].copy())
    upd = cons.profile_update(prob, be, st, sm, i_iter, history=history, pressures=pres)
    assert np.array_equal(prob.ux, before[0]) and pc.same_words(be.read_tallies()[0], before[1])      # nothing is applied
    mine, st2 = copy.deepcopy(prob), copy.deepcopy(st)
    fin = itf.iter_finalize(mine, st2, sm, i_iter, res.tallies_f64, be.layout, *pres)
    assert fin.profile_changed
    host = mine.ux[1:n + 1]
    L = be.layout
    pxx = np.round(L.view(res.tallies_f64, "pxx_flux"), 13); en = np.round(L.view(res.tallies_f64, "energy_flux"), 13)
    twin = _twin_ux(be.lib, prob, st2, sm, st2.prof_weight_fac, pxx, en, upd.q_px_avg, upd.q_en_avg, pres[0] + pres[1])[1:n + 1]
    d_host, d_twin = float(np.max(np.abs(upd.ux_next / host - 1))), float(np.max(np.abs(upd.ux_next / twin - 1)))
    SEEN[variant] = (d_host, d_twin)
    print(f"profile_update vs iter_finalize [{variant}]: max rel diff {d_host:.3e}; vs the twin {d_twin:.3e}")
    assert np.allclose(upd.ux_next, host, rtol=1e-11, atol=0), d_host
    assert np.allclose(upd.ux_next, twin, rtol=1e-11, atol=0), d_twin
    assert upd.q_px == fin.q_esc_cal_px and upd.q_en == fin.q_esc_cal_energy or np.allclose([upd.q_px, upd.q_en], [fin.q_esc_cal_px, fin.q_esc_cal_energy], rtol=1e-12)
    assert np.isclose(upd.gamma_down, fin.Gamma_downstream, rtol=1e-15) and upd.px_esc_up == fin.px_esc_flux_upstream
    assert upd.diag[0] == 0 and not np.array_equal(upd.ux_pred, prob.ux[1:n + 1]) and upd.shift_rms > 0
    if variant == "damped":
        assert pin_w(prob, st, sm, i_iter) == 10.0


def pin_w(prob, st, sm, i_iter):
    return cons.profile_in(prob, st, sm, i_iter).w


def test_classical_branch_agrees_with_the_host_and_the_twin():
    """The non-relativistic equations as tests/test_iter_finalize.py sets them up (1500 km/s, r = 4, by hand): rtol 1e-10 there, and here."""
    prob = make_problem(64)
    P = prob.params
    n = P.n_grid
    sm = itf.SmoothingConfig(SMMOE=0.3)
    st = itf.IterState.create(prob, sm, 2)                      # (before the speed is replaced: calc_rRH refuses a low beta0, quirk G2)
    pc.to_classical(prob)
    st.F_px_upstream, _, st.F_energy_upstream = itf.upstream_fluxes(prob)
    st.Gamma_grid[:, 1] = 1 + 2.0 / 3.0
    x = prob.x_grid_rg[1:n + 1]
    ramp = 1 + 0.2 * np.exp(-np.abs(x) / 30.0)
    pxx = pc.MP * P.u0 * prob.ux[1:n + 1] * ramp
    en = 0.5 * pc.MP * P.u0 ** 3 * np.ones(n)
    pin = cons.profile_in(prob, st, sm, 1)
    pin.r_RH = pin.r_comp                                       # no escape: q = 0, as the twin test passes it
    ones = np.ones(n)
    upd = cons.profile_update_host(pin, P, prob.ux, prob.gam_sf, prob.x_grid_cm, pxx, en, np.array([1.0, 2.5, 0.0, 0.0]), ones, ones, 3.0 * ones)
    assert upd.q_px_avg == 0.0 and upd.q_en_avg == 0.0 and upd.diag[1] == 0 and upd.diag[2] > 2
    mine = copy.deepcopy(prob)
    assert itf.smooth_grid_par(mine, copy.deepcopy(st), sm, 1, np.round(pxx, 13), np.round(en, 13), 0.0, 0.0, ones, ones)
    twin = _twin_ux(orc.load("det", mcs.capi), prob, st, sm, sm.old_profile_weight, np.round(pxx, 13), np.round(en, 13), 0.0, 0.0, 2 * ones)[1:n + 1]
    d_host, d_twin = float(np.max(np.abs(upd.ux_next / mine.ux[1:n + 1] - 1))), float(np.max(np.abs(upd.ux_next / twin - 1)))
    print(f"profile_update vs smooth_grid_par [classical]: max rel diff {d_host:.3e}; vs the twin {d_twin:.3e}")
    assert np.allclose(upd.ux_next, mine.ux[1:n + 1], rtol=1e-10, atol=0), d_host
    assert np.allclose(upd.ux_next, twin, rtol=1e-10, atol=0), d_twin
    assert not np.array_equal(upd.ux_next, prob.ux[1:n + 1])


# ---- the profile slot of the numpy ensemble -------------------------------------------------------------------------------------------
def _samples(branches, k=4):
    """k updates of one setting: the base case with other fluxes."""
    prob, cases = branches["rel"]
    c0 = cases[0][1]
    out = []
    for s in range(k):
        c = copy.deepcopy(c0)
        rng = np.random.default_rng(100 + s)
        c["pxx_flux"] = c["pxx_flux"] * (1 + 1e-3 * rng.standard_normal(c["n_grid"]))
        c["energy_flux"] = c["energy_flux"] * (1 + 1e-3 * rng.standard_normal(c["n_grid"]))
        out.append(host_update(prob, c))
    return prob, out


def test_host_ensemble_profile_slot(branches):
    prob, samples = _samples(branches)
    n = prob.n_grid
    e = ens.HostEnsemble(prob.params, 1)
    s = e.profile_slot
    assert s == 1 << 24 and e.is_profile(s) and not e.is_tcuts(s) and not e.is_photons_all(s) and not e.is_profile(e.tcuts_slot(0))
    assert e.names(s) == ens.PROFILE_NAMES and e.count(s) == 0
    for x in samples:
        e.add_profile(None, x)
    assert e.count(s) == 4
    mean, err, k = ens.stats_over([x.words() for x in samples])
    lay = ens.EnsLayout(prob.params).profile()
    for name in ens.PROFILE_NAMES:
        off, shape = lay[name]
        cnt = int(np.prod(shape))
        assert pc.same_words(e.mean(s, name), mean[off:off + cnt]), name
        assert pc.same_words(e.stderr(s, name), err[off:off + cnt]), name
    assert e.word_range(s, "ux_next", zones=(3, 7)) == (8 * n + 3, 4) and e.word_range(s, "scalars") == (10 * n, 8)
    got = e.summarize(s, [ens.Request("shift", zones=(0, prob.params.i_shock)), ens.Request("scalars")])
    assert 0 < got[0].n_selected <= prob.params.i_shock and got[0].n_nonfinite == 0 and 0 < got[1].n_selected <= 8
    t = ens.Trigger(s, "ux_next", "max", 1e30, zones=(0, 10))
    e.check_trigger(t)
    assert t.met(e.summarize(s, [t.request])[0])
    # merge, the merged summary and the comparison go through the slot like any other
    a, b = ens.HostEnsemble(prob.params, 1), ens.HostEnsemble(prob.params, 1)
    for x in samples[:2]:
        a.add_profile(None, x)
    for x in samples[2:]:
        b.add_profile(None, x)
    req = [ens.Request("ux_next"), ens.Request("shift", zones=(0, 20))]
    merged = a.summarize_merged([b], s, req)
    a2 = copy.deepcopy(a)
    a2.merge(b)
    assert a2.count(s) == 4 and [m.max_rel for m in merged] == [m.max_rel for m in a2.summarize(s, req)]
    assert np.allclose(a2.mean(s, "ux_next"), e.mean(s, "ux_next"), rtol=1e-14)
    assert a.compare(b, s, [ens.CompareRequest("ux_next")])[0].n_selected == n
    c = ens.HostEnsemble(prob.params, 1)
    c.merge(a)                                                    # an ensemble without settings takes those of its source
    assert c.count(s) == 2 and c.profile_settings is not None and c.profile_settings.tobytes() == a.profile_settings.tobytes()


def test_ensemble_refusals(branches):
    prob, samples = _samples(branches, 2)
    prob, cases = branches["rel"]
    other = copy.deepcopy(cases[0][1])
    other["w"] = float(np.nextafter(other["w"], 2.0))             # one bit of one setting
    odd = host_update(prob, other)
    a, b = ens.HostEnsemble(prob.params, 1), ens.HostEnsemble(prob.params, 1)
    s = a.profile_slot
    with pytest.raises(ValueError, match="from a ProfileUpdate"):
        a.add_profile(None, None)
    for x in samples:
        a.add_profile(None, x)
    with pytest.raises(ValueError, match="settings of the ProfileUpdate differ"):
        a.add_profile(None, odd)
    assert a.count(s) == 2
    hist = copy.deepcopy(cases[0][1]); hist["hist_q_px"], hist["hist_q_en"] = (0.1,), (0.2,)
    a.add_profile(None, host_update(prob, hist))                  # the q history is not a setting
    for _ in range(2):
        b.add_profile(None, odd)
    with pytest.raises(ValueError, match="profile samples differ in their settings"):
        a.merge(b)
    with pytest.raises(ValueError, match="profile samples differ in their settings"):
        a.summarize_merged([b], s, [ens.Request("shift")])
    with pytest.raises(ValueError, match="profile samples differ in their settings"):
        a.compare(b, s, [ens.CompareRequest("shift")])
    with pytest.raises((ValueError, KeyError)):
        a.word_range(s, "dNdp")
    with pytest.raises(ValueError, match="outside"):
        a.word_range(s, "shift", zones=(0, prob.n_grid + 1))
    with pytest.raises(ValueError):
        a.word_range(s, "scalars", zones=(0, 1))                  # the scalars have no zone axis
    short = copy.copy(samples[0]); short.rows = samples[0].rows[:, :-1]
    with pytest.raises(ValueError, match="words"):
        a.add_profile(None, short)


def test_statement_refusals(branches):
    prob, cases = branches["rel"]
    c = copy.deepcopy(cases[0][1])
    for bad in (-1, prob.params.i_shock + 1):
        c["i_trans"] = bad
        with pytest.raises(ValueError, match="i_trans"):
            host_update(prob, c)
    c["i_trans"] = 0
    c["hist_q_px"], c["hist_q_en"] = (1.0, 2.0, 3.0, 4.0), (1.0, 2.0, 3.0, 4.0)
    with pytest.raises(ValueError, match="at most 3"):
        host_update(prob, c)


def test_driver_refusals():
    prob = make_problem(64)
    ob = oracle_backend(prob)
    run = mcs.driver.run
    with pytest.raises(ValueError, match="profile: needs finalize=True"):
        run(prob, ob, n_itrs=1, max_pcuts=1, profile=True)
    e = ens.HostEnsemble(prob.params, 1)
    with pytest.raises(ValueError, match="a trigger on the profile slot needs profile=True"):
        run(prob, ob, n_itrs=2, max_pcuts=1, finalize=True, ensemble=e, triggers=[ens.Trigger(e.profile_slot, "shift", "max", 0.1)])

    class FakeComm:
        enabled, rank, world = True, 0, 2
    with pytest.raises(ValueError, match="communicator"):
        run(prob, ob, comm=FakeComm(), n_itrs=1, max_pcuts=1, finalize=True, profile=True)
    with pytest.raises(ValueError, match="profile: the overlapped run leaves the profile update out"):
        mcs.driver.run_overlapped(prob, [ob], n_itrs=1, profile=True)
    with pytest.raises(ValueError, match="profile: the overlapped run leaves the profile update out"):
        mcs.driver.run_overlapped(prob, [ob], n_itrs=2, ensemble=True, triggers=[ens.Trigger(e.profile_slot, "shift", "max", 0.1)])
    with pytest.raises(ValueError, match="not with smooth_shocks"):
        run(prob, ob, n_itrs=2, max_pcuts=1, smoothing=itf.SmoothingConfig(), profile=True, ensemble=e)


def test_profile_consistency_on_a_constructed_accumulator(branches):
    """Samples whose shift is known: zone 0 always 0 (z = 0), zone 1 constant and non-zero (z = inf, left out of the sum), zone 2 the
    values 1, 2, 3 (mean 2, stderr sqrt(1/3)), a downstream zone like zone 2 (left out of the upstream sum)."""
    prob, samples = _samples(branches, 3)
    n, i_shock = prob.n_grid, prob.params.i_shock
    e = ens.HostEnsemble(prob.params, 1)
    for k, x in enumerate(samples):
        y = copy.deepcopy(x)
        y.rows[9][:] = 0.0
        y.rows[9][1] = 0.25
        y.rows[9][2] = y.rows[9][n - 1] = float(k + 1)
        e.add_profile(None, y)
    with np.errstate(all="ignore"):
        pcn = ens.profile_consistency(e)
    z2 = 2.0 / np.sqrt(2.0 / 6.0)
    assert pcn.n == 3 and pcn.z.shape == (n,) and pcn.z[0] == 0.0 and np.isinf(pcn.z[1]) and np.isclose(pcn.z[2], z2, rtol=1e-15)
    assert np.isclose(pcn.z[n - 1], z2, rtol=1e-15)
    assert pcn.n_upstream == 1 and np.isclose(pcn.chi2_upstream, z2 * z2, rtol=1e-14)
    byx = ens.profile_consistency(e, x_grid_cm=prob.x_grid_cm)
    assert byx.n_upstream == 1 and byx.chi2_upstream == pcn.chi2_upstream and i_shock < n
    one = ens.HostEnsemble(prob.params, 1)
    one.add_profile(None, samples[0])
    with pytest.raises(ValueError, match="at least two profile samples"):
        ens.profile_consistency(one)


def test_run_with_profile_changes_nothing_else():
    """Three iterations with an evolving profile: with profile=True, prob.ux, the tallies and iter_finals are bit for bit those of the
    run without it; the q history handed over is the one iter_finalize averages; ux_next is the profile the host then applied."""
    N = 600
    sm = itf.SmoothingConfig(smooth_shocks=True)
    cfg = mcs.inputs.Config(N_PTS_INJ=N, N_PTS_PCUT=N, N_PTS_PCUT_HI=N, num_iterations=3)
    out = []
    for profile in (False, True):
        prob = mcs.inputs.build_problem(cfg)
        be = orc.OracleBackend(mcs.capi, "det", nthreads=1); be.create(prob)
        uxs = []
        res = mcs.driver.run(prob, be, None, n_itrs=3, max_pcuts=10, smoothing=sm, profile=profile, on_iteration_end=lambda it: uxs.append(prob.ux.copy()))
        out.append((prob, res, uxs))
    (p0, r0, u0), (p1, r1, u1) = out
    assert r0.profile is None and [it for it, _ in r1.profile] == [1, 2, 3]
    assert np.array_equal(p0.ux, p1.ux) and all(np.array_equal(a, b) for a, b in zip(u0, u1))
    assert pc.same_words(r0.tallies_f64, r1.tallies_f64) and np.array_equal(r0.tallies_i64, r1.tallies_i64)
    for (ia, fa, ja), (ib, fb, jb) in zip(r0.iter_finals, r1.iter_finals):
        assert ia == ib and fa == fb and pc.same_words(ja.P_psd_par, jb.P_psd_par) and pc.same_words(ja.dNdp_cr, jb.dNdp_cr)
    n = p1.n_grid
    qs = [(f.q_esc_cal_px, f.q_esc_cal_energy) for _, f, _ in r1.iter_finals]
    for k, (it, upd) in enumerate(r1.profile):
        assert np.allclose([upd.q_px, upd.q_en], qs[k], rtol=1e-12, atol=0)
        assert np.isclose(upd.q_px_avg, np.mean([q[0] for q in qs[:k + 1]]), rtol=1e-12)
        assert np.allclose(upd.ux_next, u1[k][1:n + 1], rtol=1e-11, atol=0)       # what the host's update then wrote
    # a fixed-profile run with an ensemble: one sample per iteration, no history
    prob = mcs.inputs.build_problem(cfg)
    be = orc.OracleBackend(mcs.capi, "det", nthreads=1); be.create(prob)
    e = ens.HostEnsemble(prob.params, 1)
    res = mcs.driver.run(prob, be, None, n_itrs=2, max_pcuts=10, finalize=True, profile=True, ensemble=e)
    assert e.count(e.profile_slot) == 2 and all(upd.q_px_avg == upd.q_px for _, upd in res.profile)
    assert pc.same_words(e.mean(e.profile_slot, "ux_pred"), ens.stats_over([u.words() for _, u in res.profile])[0][7 * n:8 * n])
    assert ens.profile_consistency(e).n == 2
