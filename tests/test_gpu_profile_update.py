"""K13, mcs_profile_update (csrc/mcs_consumers.hip: mcs_k_profile_update) on crafted fluxes, scalars and pressures against the
restatement of tests/profile_common.py: every output word and the three counts bit for bit, in both branches, with NaN in every tally
word the call must not read; the reproducibility of the bits, the path that reads the pressures mcs_thermo_calcs left on the device,
what the call leaves untouched, the refusals, and one real species against the numpy statement on the same context's tallies."""
import copy
import ctypes as ct

import numpy as np
import pytest

import profile_common as pc
from conftest import mcs, make_problem, hip_backend

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
cons = mcs.consumers
itf = mcs.iter_finalize


def pin_of(c, **kw):
    d = {k: c[k] for k in cons.PROFILE_SETTINGS}
    d.update(hist_q_px=c["hist_q_px"], hist_q_en=c["hist_q_en"], pxx_EM=c["pxx_EM"], en_EM=c["en_EM"], atan_x=c["atan_x"])
    d.update(kw)
    return cons.ProfileIn(**d)


def load_case(hb, c):
    """The case's fluxes and scalars into the context's tallies, a NaN in every other fp64 tally word."""
    _, i = hb.read_tallies()
    hb.write_tallies(pc.crafted_tallies(hb.layout, c), i)


def pressures(c):
    return c["P_par"], c["P_perp"], c["e_dens"]


@pytest.fixture(scope="module", params=["rel", "cls"])
def ctx(request):
    prob = make_problem(64) if request.param == "rel" else pc.classical_problem()        # (the classical speed before the context is made)
    assert (prob.params.beta0 >= 0.02) == (request.param == "rel") and prob.n_grid == 99
    hb = hip_backend(prob)
    hb.begin_iteration(1)
    hb.begin_species(1, 1, 1.0, 1.0, prob.pmax, 1.0, 1.0)
    yield prob, hb, pc.make_cases(prob)
    hb.destroy()


def test_crafted_cases(ctx):
    """Every output word and diag equal the restatement's, through the pressures pointer; a second call gives the same bits."""
    prob, hb, cases = ctx
    n = prob.n_grid
    assert len(cases) >= 9
    for name, c in cases:
        ref = pc.restate(c)
        load_case(hb, c)
        out, diag = hb.profile_update(pin_of(c), pressures(c))
        print(f"{name}: diag {diag.tolist()}, shift_rms {out[10 * n + 7]!r}")
        assert pc.same_words(out, ref.words()), (name, pc.first_difference(out, ref.words(), n))
        assert np.array_equal(diag, ref.diag), (name, diag, ref.diag)
        again, diag2 = hb.profile_update(pin_of(c), pressures(c))
        assert np.array_equal(again.view(np.uint64), out.view(np.uint64)) and np.array_equal(diag, diag2), name
        f, _ = hb.read_tallies()
        assert pc.same_words(f, pc.crafted_tallies(hb.layout, c)), name          # the tallies are what they were


def test_refusals(ctx):
    prob, hb, cases = ctx
    lib = hb.lib
    c = cases[0][1]
    load_case(hb, c)
    with pytest.raises(RuntimeError, match="mcs_profile_update: no pressures on the context"):
        hb.profile_update(pin_of(c), None)
    for bad in (-1, prob.params.i_shock + 1):
        with pytest.raises(RuntimeError, match="mcs_profile_update: i_trans"):
            hb.profile_update(pin_of(c, i_trans=bad), pressures(c))
    out = np.zeros(mcs.capi.profile_layout(prob.params).total)
    pr = np.ascontiguousarray(np.concatenate(pressures(c)))
    s = pin_of(c).as_struct()
    s.n_hist = 4
    assert lib.mcs_profile_update(hb.h, ct.byref(s), pr.ctypes.data_as(mcs.capi.c_double_p), out.ctypes.data_as(mcs.capi.c_double_p), None) != 0
    assert b"mcs_profile_update: 4 earlier" in lib.mcs_last_error() and not out.any()
    s = pin_of(c).as_struct()
    s.atan_x = None
    assert lib.mcs_profile_update(hb.h, ct.byref(s), pr.ctypes.data_as(mcs.capi.c_double_p), out.ctypes.data_as(mcs.capi.c_double_p), None) != 0
    assert b"mcs_profile_update: null table" in lib.mcs_last_error() and not out.any()
    fresh = hip_backend(prob)
    try:
        with pytest.raises(RuntimeError, match="mcs_profile_update: no species has begun"):
            fresh.profile_update(pin_of(c), pressures(c))
    finally:
        fresh.destroy()
    h = ct.c_void_p(None)                                   # a context whose grid was never set
    assert lib.mcs_create(ct.byref(prob.params), 0, None, ct.byref(h)) == 0
    try:
        s = pin_of(c).as_struct()
        assert lib.mcs_profile_update(h, ct.byref(s), pr.ctypes.data_as(mcs.capi.c_double_p), out.ctypes.data_as(mcs.capi.c_double_p), None) != 0
        assert b"mcs_profile_update: grid not set" in lib.mcs_last_error() and not out.any()
    finally:
        lib.mcs_destroy(h)


def test_a_real_species_the_resident_pressures_and_what_stays():
    """2000 protons through four pcuts with run(finalize=True, profile=True): the call read the pressures mcs_thermo_calcs left on the
    device.  The same words come from the pointer path fed those pressures and from the numpy statement on the tallies of the same
    context; the tallies, the K4 results on the device and the results of K10, K11 and K12 are what they were; after a products sample
    the resident path is refused."""
    prob = make_problem(2000)
    n = prob.n_grid
    hb = hip_backend(prob)
    try:
        sm = itf.SmoothingConfig(smooth_shocks=False, SMMOE=0.4, artificial_smoothing_start_rg=-3.0)
        res = mcs.driver.run(prob, hb, n_itrs=1, max_pcuts=4, smoothing=sm, profile=True)
        (it, got), = res.profile
        (_, fin, ion), = res.iter_finals
        assert it == 1 and got.diag[0] == 0 and got.diag[1] == 0 and got.shift_rms > 0
        pres = (ion.P_psd_par, ion.P_psd_perp, ion.energy_density_psd)
        wins = cons.momentum_windows(prob, [(1.0e-20, 1.0e-10)])
        others = lambda: np.concatenate([cons.escape_spectra(prob, hb, 1).dndp.ravel(), cons.angle_distributions(prob, hb, 1, wins).dist.ravel(),
                                         cons.tcut_spectra(prob, hb, 1).words()])
        before, o_before = hb.read_tallies(), others()
        pin = cons.profile_in(prob, res.iter_state, sm, 1)
        assert pin.i_trans >= 1 and pin.SMMOE == 0.4
        by_ptr, d_ptr = hb.profile_update(pin, pres)
        resident, d_res = hb.profile_update(pin, None)
        assert pc.same_words(by_ptr, got.words()) and pc.same_words(resident, got.words())
        assert np.array_equal(d_ptr, got.diag) and np.array_equal(d_res, got.diag)
        L = hb.layout
        f = before[0]
        host = cons.profile_update_host(pin, prob.params, prob.ux, prob.gam_sf, prob.x_grid_cm, L.view(f, "pxx_flux"), L.view(f, "energy_flux"),
                                        L.view(f, "scalars"), *pres)
        assert pc.same_words(host.words(), got.words()), pc.first_difference(host.words(), got.words(), n)
        assert np.array_equal(host.diag, got.diag)
        # the host's own update agrees within the twin tolerance (it is not bit-equal: powers)
        mine = copy.deepcopy(prob)
        sm_on = itf.SmoothingConfig(SMMOE=0.4, artificial_smoothing_start_rg=-3.0)
        assert itf.iter_finalize(mine, itf.IterState.create(prob, sm_on, 1), sm_on, 1, f, L, *pres).profile_changed
        assert np.allclose(got.ux_next, mine.ux[1:n + 1], rtol=1e-11, atol=0), float(np.max(np.abs(got.ux_next / mine.ux[1:n + 1] - 1)))
        after, o_after = hb.read_tallies(), others()
        assert pc.same_words(before[0], after[0]) and np.array_equal(before[1], after[1]) and pc.same_words(o_before, o_after)
        # the K4 block on the device is what ion_finalize left: the products sample reads it
        e = ens.HipEnsemble(hb, 1)
        try:
            mcs.driver._add_products(e, prob, hb, ion)
            ps = e.products_slot(0)
            assert pc.same_words(e.mean(ps, "P_psd_par"), ion.P_psd_par) and pc.same_words(e.mean(ps, "energy_density_psd"), ion.energy_density_psd)
            assert pc.same_words(e.mean(ps, "dNdp_sf"), ion.dNdp_cr[0])
            with pytest.raises(RuntimeError, match="mcs_profile_update: no pressures on the context"):
                hb.profile_update(pin, None)
            again, _ = hb.profile_update(pin, pres)           # the pointer path needs none
            assert pc.same_words(again, got.words())
        finally:
            e.destroy()
    finally:
        hb.destroy()
