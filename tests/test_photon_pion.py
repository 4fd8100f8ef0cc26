"""SURVEY.md 8(f-4), third emission process: pion-decay gamma rays of the nuclei (src/photon_calcs.jl:66-88 -> src/photon_pion_decay.jl
-> src/pion_kafexhiu.jl with src/KATV2014.jl: Kafexhiu, Aharonian, Taylor & Vila 2014 -- dead code in the reference, followed as
specification; include/mcs_pion.h lists where it is followed as written against the paper, P1-P3).

CPU: the oracle-side twin (oracle/mcs_consumers.cpp: orc_photon_pion and the three KATV2014 functions) against a direct numpy
restatement written from the Julia text that shares no code with it; what the parametrisation itself promises (the inelastic cross
section of eq. 1 against the paper's quoted behaviour, continuity of the piecewise fits where the paper joins them, the kinematic
limit, a power law of protons giving a power law of photons with the same index); the host wrapper's units.  GPU: the device kernel
(K7: mcs_photon_pion through the C ABI) against the twin on identical input -- 1e-11 relative per entry: the two sides differ in one
ulp of pow / exp / log (ocml against glibc) on sums of positive terms in the same order."""
import math

import numpy as np
import pytest

import photon_fold_common as pf
from conftest import mcs, make_problem, oracle_backend

C, MP = mcs.constants.C, mcs.constants.MP
GEV = 1.602176634e-3
MPC2 = 0.93827208816
TTH, MRES, GRES, MPI = 0.2797, 1.1883, 0.2264, 0.134976          # constants.jl:16-22


# ---- the Julia text restated with numpy (vectorised over T_p or E_gamma; GEANT 4 branch = i_data 1, what the reference hard-wires) ----
def sigma_inel(T):
    r = T / TTH
    return (30.7 - 0.96 * np.log(r) + 0.18 * np.log(r) ** 2) * (1 - r ** -1.9) ** 3


def sigma_pi_np(T):
    T = np.asarray(T, dtype=float)
    s = 2 * MPC2 * (T + 2 * MPC2)
    g = MRES * math.hypot(MRES, GRES)
    K = math.sqrt(8) * MRES * GRES * g / (math.pi * math.sqrt(MRES ** 2 + g))
    fBW = MPC2 * K / (((np.sqrt(s) - MPC2) ** 2 - MRES ** 2) ** 2 + MRES ** 2 * GRES ** 2)
    with np.errstate(invalid="ignore"):
        eta = np.sqrt((s - MPI ** 2 - 4 * MPC2 ** 2) ** 2 - (4 * MPI * MPC2) ** 2) / (2 * MPI * np.sqrt(s))
        low = 7.66e-3 * eta ** 1.95 * (1 + eta + eta ** 5) * fBW ** 1.86 + np.where(T < 2 * TTH, 0.0, 5.7 / (1 + np.exp(-9.3 * (T - 1.4))))
        Q = (T - TTH) / MPC2
        mid = (-6.0e-3 + 0.237 * Q - 0.023 * Q ** 2) * sigma_inel(T)
        xi = np.maximum(T - 3, 1e-300) / MPC2
        high = 0.728 * xi ** 0.2503 * (1 + np.exp(-0.596 * xi ** 0.117)) * (1 - np.exp(-0.491 * xi ** 0.25)) * sigma_inel(T)
    return np.where(T < 2, low, np.where(T < 5, mid, high))


def amax_np(T):
    T = np.asarray(T, dtype=float)
    s = 2 * MPC2 * (T + 2 * MPC2)
    rs = np.sqrt(s)
    Epi = (s - 4 * MPC2 ** 2 + MPI ** 2) / (2 * rs)
    gcm = (T + 2 * MPC2) / rs
    bcm = np.sqrt(1 - 1 / gcm ** 2)
    Ppi = np.sqrt(Epi ** 2 - MPI ** 2)
    Emax_pi = gcm * (Epi + Ppi * bcm)
    gl = Emax_pi / MPI
    bl = np.sqrt(1 - 1 / gl ** 2)
    Egmax = MPI / 2 * gl * (1 + bl)
    sp = sigma_pi_np(T)
    th = T / MPC2
    b = np.where(T < 5, [[9.53], [0.52], [0.054]], [[9.13], [0.35], [0.0097]])
    A = np.where(T < 1, 5.9 * sp / Emax_pi, b[0] * th ** -b[1] * sp / MPC2 * np.exp(b[2] * np.log(th) ** 2))
    return Egmax, A


def F_np(T, E, Egmax):
    """one T_p, an array of photon energies"""
    E = np.asarray(E, dtype=float)
    Y, Ymax = E + MPI ** 2 / E, Egmax + MPI ** 2 / Egmax            # P1: as written
    X = (Y - MPI) / (Ymax - MPI)
    ok = (X >= 0) & (X <= 1)
    Xc = np.clip(X, 0, 1)
    if T < 1:
        out = (1 - Xc) ** (3.29 - 0.2 * (T / MPC2) ** -1.5)
    else:
        q = (T - 1) / MPC2
        mu = 1.25 * q ** 1.25 * math.exp(-1.25 * q)
        if T < 4:
            lam, al, be, ga = 3.0, 1.0, mu + 2.45, mu + 1.45
        elif T < 20:
            lam, al, be, ga = 3.0, 1.0, 1.5 * mu + 4.95, mu + 1.5
        elif T > 100:
            lam, al, be, ga = 3.0, 0.5, 4.9, 1.0
        else:
            lam, al, be, ga = 3.0, 0.5, 4.2, 1.0
        Cc = lam * MPI / Ymax
        out = (1 - Xc ** al) ** be / (1 + Xc / Cc) ** ga
    return np.where(ok, out, 0.0)


def pion_direct(dndp, pe, mc, aa, target, scaling, n_photon, emin_mev, bpd):
    """pion_kafexhiu + the count conversion of photon_pion_decay, per zone"""
    E_erg = 10.0 ** (math.log10(emin_mev * 1.602176634e-6) + np.arange(n_photon) / bpd)
    Eg = E_erg / GEV
    out = np.full((dndp.shape[0], n_photon), 1e-99)
    p2 = pe[:-1] * pe[1:]
    gam = np.sqrt(1 + p2 / mc ** 2)
    T = (gam - 1) * (aa * MPC2) / aa
    vel = np.sqrt(p2) / (gam * aa * MP)
    for z in range(dndp.shape[0]):
        d = dndp[z, :-1]
        cnt = np.where(d <= 1e-99, 1e-99, d * np.diff(pe))
        acc = np.full(n_photon, 1e-99)
        for i in np.flatnonzero((cnt > 1e-99) & (T >= TTH)):
            Egmax, A = (float(np.ravel(v)[0]) for v in amax_np(T[i]))
            acc = acc + target[z] * cnt[i] * vel[i] * (A * F_np(T[i], Eg, Egmax) * Eg * 1e-27) * E_erg
        out[z] = np.where(acc < 1e-99, 1e-99, acc * scaling)
    return E_erg, out


def _synthetic(prob, seed=5):
    """plasma-frame dN/dp of a proton species: power laws of different index and cut-off per zone, some zones empty, holes inside"""
    P = prob.params
    t = mcs.consumers.consumer_tables(prob, 1)
    pe = t.mom_edge_cgs
    rng = np.random.default_rng(seed)
    pc = np.sqrt(pe[:-1] * pe[1:])
    d = np.full((P.n_grid, len(pe)), 1e-99)
    for z in range(P.n_grid):
        if z % 5 == 4:
            continue
        idx = 1.5 + rng.random() * 1.5
        cut = 10.0 ** rng.uniform(0.5, 6.0) * MP * C
        d[z, :-1] = 1e55 * rng.random() * (pc / (MP * C)) ** -idx * np.exp(-pc / cut) / (MP * C)
        d[z, rng.integers(0, len(pe) - 1, 6)] = 1e-99
    d[d < 1e-90] = 1e-99
    target = 1.0 / np.sqrt(np.asarray(prob.gam_sf)[1:P.n_grid + 1] ** 2 - 1 + 1e-3)
    return t, pe, d, np.ascontiguousarray(target)


def test_katv_functions_against_the_julia_text():
    ob = oracle_backend(make_problem(16))
    lib = ob.lib
    import ctypes as ct
    T = np.concatenate([np.geomspace(TTH * 1.0001, 1.0e6, 400), [0.5, 0.9999, 1.0, 1.9999, 2.0, 3.9999, 4.0, 4.9999, 5.0, 19.999, 20.0, 100.0, 100.001]])
    got = np.array([lib.orc_pion_sigma_pi(float(x), 1) for x in T])
    assert np.allclose(got, sigma_pi_np(T), rtol=1e-12, atol=0)
    Eg, A = ct.c_double(), ct.c_double()
    Egmax_np, A_np = amax_np(T)
    for k, x in enumerate(T):
        lib.orc_pion_amax(float(x), 1, ct.byref(Eg), ct.byref(A))
        assert abs(Eg.value / Egmax_np[k] - 1) < 1e-12 and abs(A.value / A_np[k] - 1) < 1e-12
        E = np.geomspace(1e-3, Egmax_np[k] * 1.5, 60)
        f = np.array([lib.orc_pion_F(float(x), float(e), 1, float(Egmax_np[k])) for e in E])
        assert np.allclose(f, F_np(float(x), E, float(Egmax_np[k])), rtol=1e-10, atol=1e-300)
        if Egmax_np[k] > MPI:       # the kinematic limit (P1: as written Y has its minimum at m_pi, not m_pi / 2, so the limit holds
            assert np.all(f[E > Egmax_np[k] * (1 + 1e-12)] == 0.0)      # only once E_gamma^max has passed m_pi: T_p > 0.5 GeV)
        assert np.all((f >= 0) & (f <= 1))
    # the other three event generators differ from GEANT 4 only above their validity thresholds (KATV2014.jl:67-96, 186-211, 266-290)
    for i_data, thr in ((2, 50.0), (3, 100.0), (4, 100.0)):
        assert lib.orc_pion_sigma_pi(thr * 0.99, i_data) == lib.orc_pion_sigma_pi(thr * 0.99, 1)
        assert lib.orc_pion_sigma_pi(thr * 10, i_data) != lib.orc_pion_sigma_pi(thr * 10, 1)
        assert abs(lib.orc_pion_sigma_pi(thr * 10, i_data) / lib.orc_pion_sigma_pi(thr * 10, 1) - 1) < 0.35
    ob.destroy()


def test_parametrisation_is_physical():
    """What the paper says of its own fits, checked on the restated functions through the twin."""
    ob = oracle_backend(make_problem(16))
    lib = ob.lib
    # eq. (1): ~ 30 mb plateau at a few GeV, rising as log^2: ~ 57 mb at T_p = 1e6 GeV (sqrt(s) = 1.4 TeV)
    assert 28 < sigma_inel(np.array([5.0]))[0] < 32 and 50 < sigma_inel(np.array([1e6]))[0] < 65
    # the pi0 cross section vanishes at threshold, grows monotonically; the fits join within 10 % at 2 and 5 GeV
    T = np.geomspace(TTH * 1.001, 1e5, 300)
    s = np.array([lib.orc_pion_sigma_pi(float(x), 1) for x in T])
    assert s[0] < 1e-3 and np.all(np.diff(s) > -0.02 * s[1:])
    for Tj in (2.0, 5.0):
        a, b = lib.orc_pion_sigma_pi(Tj * (1 - 1e-9), 1), lib.orc_pion_sigma_pi(Tj, 1)
        assert abs(a / b - 1) < 0.10
    # E_gamma^max -> T_p + (a little) for T_p >> m_p; at threshold the pion is made at rest in the CM frame
    import ctypes as ct
    Eg, A = ct.c_double(), ct.c_double()
    lib.orc_pion_amax(1.0e5, 1, ct.byref(Eg), ct.byref(A))
    assert 0.9 < Eg.value / 1.0e5 < 1.01
    lib.orc_pion_amax(TTH * 1.0000001, 1, ct.byref(Eg), ct.byref(A))
    g_cm = (TTH + 2 * MPC2) / math.sqrt(2 * MPC2 * (TTH + 2 * MPC2))
    assert abs(Eg.value / (MPI / 2 * g_cm * (1 + math.sqrt(1 - 1 / g_cm ** 2))) - 1) < 0.03        # (T_th is the rounded 0.2797 GeV)
    ob.destroy()


def test_pion_fold_against_direct_evaluation():
    prob = make_problem(64)
    t, pe, d, target = _synthetic(prob)
    ob = oracle_backend(prob)
    for aa, scaling, n_photon, emin, bpd in ((1.0, 1.0, 120, 1.0, 10), (4.0, 2.37, 45, 10.0, 4)):
        mc = aa * MP * C
        E, got = ob.photon_pion(d, pe, mc, aa, target, scaling, n_photon, emin, bpd)
        E_ref, want = pion_direct(d, pe, mc, aa, target, scaling, n_photon, emin, bpd)
        assert np.allclose(E, E_ref, rtol=1e-13)
        assert want.max() > 1e-30 and (want > 1e-99).sum() > 500
        assert np.array_equal(got > 1e-99, want > 1e-99)
        assert np.allclose(got, want, rtol=1e-9, atol=0), float(np.max(np.abs(got / want - 1)))
        empty = np.flatnonzero((d <= 1e-99).all(axis=1))
        assert len(empty) and np.all(got[empty] == 1e-99 * scaling)       # the 1e-99 fill is scaled too (pion_kafexhiu.jl:235-241)
    # linear in the target density and in the scaling factor; the other generators change only the top of the spectrum
    E, a = ob.photon_pion(d, pe, MP * C, 1.0, target, 1.0, 120, 1.0, 10)
    _, b = ob.photon_pion(d, pe, MP * C, 1.0, 3 * target, 2.0, 120, 1.0, 10)
    lit = a > 1e-99
    assert np.allclose(b[lit], 6 * a[lit], rtol=1e-13)
    _, c = ob.photon_pion(d, pe, MP * C, 1.0, target, 1.0, 120, 1.0, 10, i_data=3)
    assert not np.array_equal(a, c)
    # a power law of protons dN/dp ~ p^-s well above threshold radiates dP/dlnE ~ E^(2-s) (scaling of the cross section aside)
    s_idx = 2.3
    pc = np.sqrt(pe[:-1] * pe[1:])
    one = np.full_like(d, 1e-99)
    one[0, :-1] = 1e50 * (pc / (MP * C)) ** -s_idx
    E, em = ob.photon_pion(one, pe, MP * C, 1.0, target, 1.0, 120, 1.0, 10)
    sel = (E / GEV > 5) & (E / GEV < 500)        # (far above, the fit's exp(b3 log^2 theta) and multiplicity harden it by up to 0.35)
    assert sel.sum() >= 15
    slope = np.polyfit(np.log(E[sel]), np.log(em[0][sel]), 1)[0]
    assert -0.02 < slope - (2 - s_idx) < 0.15, slope                  # the rising sigma_inel and multiplicity harden it slightly
    # P1: with Y = E + m^2 / E the spectrum of one proton bin is symmetric in ln E about m_pi (the paper's form: about m_pi / 2)
    one[0, :-1] = 1e-99
    i_p = int(np.searchsorted(pc, 3.0 * MP * C))
    one[0, i_p] = 1e50
    E, em = ob.photon_pion(one, pe, MP * C, 1.0, target, 1.0, 400, 1e-1, 50)
    lit = em[0] > 1e-99
    lo, hi = E[lit].min() / GEV, E[lit].max() / GEV
    assert abs(math.sqrt(lo * hi) / MPI - 1) < 0.06
    ob.destroy()


def test_photon_pion_host_wrapper():
    """consumers.photon_pion end to end on the oracle backend: protons and helium through the transport, get_dNdp_cr, the fold, and
    photon_pion_decay's conversions (src/photon_pion_decay.jl:62-63, 112-125)."""
    prob = make_problem(400, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(4.0, 2.0, 1e6, 0.1)])
    be = oracle_backend(prob, nthreads=8)
    res = mcs.driver.run(prob, be, n_itrs=1)
    be.write_tallies(res.tallies_f64, res.tallies_i64)                 # the tallies of the last species (helium: quirk Q2)
    fin = mcs.consumers.ion_finalize(prob, be, 2)
    ph = mcs.consumers.photon_pion(prob, be, fin, 2, jet_dist_kpc=1.0e3, redshift=0.2)
    assert ph.n_pion_specs == 2
    assert len(ph.energy_MeV) == 120 and abs(ph.energy_MeV[0] - 1) < 1e-12 and abs(ph.energy_MeV[10] / 10 - 1) < 1e-12
    sf = (4 ** 0.375 + 1 ** 0.375 - 1) ** 2 * 1.0 + (4 ** 0.375 + 4 ** 0.375 - 1) ** 2 * 0.1
    assert abs(mcs.consumers.pion_scaling_factor(prob.cfg, 4.0) / sf - 1) < 1e-14
    d_lum = 1.0e3 * 1.2 * mcs.consumers.KPC_CM
    lit = ph.emis_erg_s / (4 * math.pi * d_lum ** 2) >= 1e-99
    assert lit.any()                                                   # accelerated helium above 0.28 GeV per nucleon radiates
    assert np.allclose(ph.energy_flux[lit], ph.emis_erg_s[lit] / (4 * math.pi * d_lum ** 2), rtol=1e-14)
    assert np.all(ph.energy_flux[~lit] == 1e-99) and np.all(ph.photon_flux[~lit] == 1e-99) and np.all(ph.pion_photon_sum[~lit] == 0)
    E_erg = ph.energy_MeV * 1.602176634e-6
    assert np.allclose(ph.photon_flux[lit], (ph.energy_flux / E_erg[None, :])[lit], rtol=1e-14)
    assert np.array_equal(ph.pion_photon_sum[lit], ph.photon_flux[lit])
    # the fold was given the plasma-frame dN/dp and the proton target density of the zone
    t = mcs.consumers.consumer_tables(prob, 2)
    P = prob.params
    target = prob.cfg.species[0].density * P.gam0 * P.beta0 / np.sqrt(np.asarray(prob.gam_sf)[1:P.n_grid + 1] ** 2 - 1)
    _, want = pion_direct(fin.dNdp_cr[1], t.mom_edge_cgs, t.mc, 4.0, target, sf, 120, 1.0, 10)
    assert np.array_equal(ph.emis_erg_s > 1e-99, want > 1e-99)
    assert np.allclose(ph.emis_erg_s, want, rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        eprob = make_problem(16, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(mcs.constants.ME / MP, -1.0, 1e6, 1.0)])
        mcs.consumers.photon_pion(eprob, be, fin, 2)                    # electrons: no pion branch
    be.destroy()


@pytest.mark.gpu
def test_gpu_pion_matches_cpu_twin():
    """K7 on the device against the twin on identical input: synthetic spectra (every branch of the parametrisation is crossed by
    the momentum grid: T_p from below threshold to the top of the grid), all four cross-section data sets, two species."""
    from conftest import hip_backend
    prob = make_problem(64)
    t, pe, d, target = _synthetic(prob, seed=9)
    ob = oracle_backend(prob)
    hb = hip_backend(prob)
    for aa, scaling, n_photon, emin, bpd, i_data in ((1.0, 1.0, 120, 1.0, 10, 1), (4.0, 2.37, 45, 10.0, 4, 1), (1.0, 1.3, 300, 0.5, 25, 2),
                                                    (1.0, 1.0, 120, 1.0, 10, 3), (56.0, 9.1, 120, 1.0, 10, 4)):
        mc = aa * MP * C
        Eo, o = ob.photon_pion(d, pe, mc, aa, target, scaling, n_photon, emin, bpd, i_data)
        Eg, g = hb.photon_pion(d, pe, mc, aa, target, scaling, n_photon, emin, bpd, i_data)
        assert np.allclose(Eg, Eo, rtol=1e-14)
        assert o.max() > 1e-30
        edge = np.abs(np.log(np.maximum(g, 1e-99) / np.maximum(o, 1e-99))) > 1e-6
        # a photon energy within an ulp or so of a bin's kinematic limit may fall on either side of it: every such output must be one
        # the mpmath reference cannot decide either (X within its running bound of 1 in some lit bin: photon_fold_common.py)
        with pf.libm(pf.DEVICE):
            for z, j in zip(*np.nonzero(edge)):
                assert pf.pion_point_undecidable(d[z], pe, mc, aa, i_data, target[z], scaling, Eg[j]), (aa, i_data, z, j, g[z, j], o[z, j])
        ok = ~edge
        assert np.array_equal((g > 1e-99 * scaling)[ok], (o > 1e-99 * scaling)[ok])
        assert np.allclose(g[ok], o[ok], rtol=1e-11, atol=0), float(np.max(np.abs(g[ok] / o[ok] - 1)))
    with pytest.raises(RuntimeError):
        hb.photon_pion(d, pe, MP * C, 1.0, target, 1.0, 120, 1.0, 10, i_data=5)
    # end to end: the wrapper on the device equals the wrapper on the twin, on the dN/dp of a real run
    prob2 = make_problem(1500)
    be = oracle_backend(prob2, nthreads=8)
    res = mcs.driver.run(prob2, be, n_itrs=1)
    be.write_tallies(res.tallies_f64, res.tallies_i64)
    hb2 = hip_backend(prob2)
    hb2.begin_iteration(1)
    hb2.write_tallies(res.tallies_f64, res.tallies_i64)
    fo = mcs.consumers.ion_finalize(prob2, be, 1)
    fg = mcs.consumers.ion_finalize(prob2, hb2, 1)
    po = mcs.consumers.photon_pion(prob2, be, fo, 1)
    pg = mcs.consumers.photon_pion(prob2, hb2, fg, 1)
    assert (po.emis_erg_s > 1e-99).sum() > 100
    assert np.array_equal(pg.emis_erg_s > 1e-99, po.emis_erg_s > 1e-99)
    assert np.allclose(pg.emis_erg_s, po.emis_erg_s, rtol=1e-9, atol=0)
    ob.destroy(); hb.destroy(); be.destroy(); hb2.destroy()
