"""The escape spectra without a GPU: the new entry points and the escape sample's layout (include/mcs.h, "escape sample"), the
restatement of tests/escape_common.py pinned against the CPU oracle's get_dNdp_cr, the default plasma frames of
consumers.escape_spectra, what driver.run and run_overlapped refuse, and the slot numbers of ensemble.Ensemble."""
import ctypes as ct
import os

import numpy as np
import pytest

import consumers_common as cc
import escape_common as ec
from conftest import ROOT, mcs, make_problem, oracle_backend

ens = mcs.ensemble


# ---- (a) the ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_and_layout():
    lib = mcs.capi.load_library()
    for name in ("mcs_dndp_esc", "mcs_ens_add_escape", "mcs_ens_escape_get_layout"):
        assert hasattr(lib, name) and name in mcs.capi.EXPORTED_SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "mcs.h")).read()
    assert "#define MCS_ENS_ESCAPE(s) ((s) | (1 << 27))" in header and mcs.capi.ENS_ESCAPE_BIT == 1 << 27
    for kw in (cc.SMALL_BINNING, cc.LARGE_BINNING, {}):
        P = make_problem(64, **kw).params
        NM = P.num_psd_mom_bins + 2
        X = mcs.capi.McsEnsEscapeLayout()
        assert lib.mcs_ens_escape_get_layout(ct.byref(P), ct.byref(X)) == 0
        got = {name: int(getattr(X, name)) for name, _ in X._fields_}
        assert got == dict(dNdp=0, number=6 * NM, slope=6 * NM + 6, row_n=NM, total=6 * NM + 12)
        mirror = ens.EnsLayout(P)
        assert got == mirror.escape_fields and mirror.escape_total == 6 * NM + 12
        assert mirror.escape == {"dNdp": (0, (6, NM)), "number": (6 * NM, (6,)), "slope": (6 * NM + 6, (6,))}
    assert make_problem(64, **cc.LARGE_BINNING).params.num_psd_mom_bins == 199
    assert lib.mcs_ens_escape_get_layout(None, ct.byref(X)) != 0 and b"mcs_ens_escape_get_layout" in lib.mcs_last_error()


def test_no_context_no_spectra():
    lib = mcs.capi.load_library()
    prob = cc.small_problem()
    s = ec.escape_tables(prob, 1).as_struct()
    dp = mcs.capi.c_double_p
    g, out, num = np.ones(2), np.zeros((2, 3, prob.params.num_psd_mom_bins + 2)), np.zeros((2, 3))
    rc = lib.mcs_dndp_esc(None, ct.byref(s), g.ctypes.data_as(dp), out.ctypes.data_as(dp), num.ctypes.data_as(dp), None)
    assert rc != 0 and b"mcs_dndp_esc" in lib.mcs_last_error() and not out.any()
    assert lib.mcs_ens_add_escape(None, None, 0) != 0 and b"mcs_ens_add_escape" in lib.mcs_last_error()


# ---- (b) the restatement against the oracle --------------------------------------------------------------------------------------------
REL = 4 * cc.U          # one multiply (the oracle's normalisation) and one divide (taking it out again)


@pytest.mark.parametrize("i_ion", (1, 3))
def test_reference_agrees_with_the_oracle(i_ion):
    """A door's slab with one lit cell, copied into a zone's psd slab (stride 201 -> nmom + 2), through OracleBackend.dndp_cr with
    the zone's gam_sf set to the door's gamma: divided by the zone's norm (cc.normalise_row on the restatement's own dN), frames 1
    and 2 agree with the restatement within 4 * 2^-53 and light the same bins; frame 0 likewise.  Every cell of the slab takes part;
    the gammas walk cc.GAMMAS, the weights cc.WEIGHTS."""
    prob0 = cc.small_problem() if i_ion == 1 else cc.three_species_problem()
    prob = mcs.inputs.build_problem(prob0.cfg)
    P = prob.params
    nm, nt, ng = P.num_psd_mom_bins, P.num_psd_tht_bins, P.n_grid
    NM, NT = nm + 2, nt + 2
    L = mcs.capi.Layout(P)
    be = oracle_backend(prob)
    launches = ec.impulse_launches(nm, nt, 2)
    zones = [z for z in range(1, ng + 1) if z % 2]          # door 0 of a launch goes to zone z, door 1 to zone z + 1
    assert ng % 2 and len(zones) * 2 - 1 <= ng
    zones = zones[:-1]
    compared = lit_bins = 0
    worst, diag_all = 0.0, np.zeros(2, dtype=np.int64)
    for r in range(0, len(launches), len(zones)):
        batch = launches[r:r + len(zones)]
        gam0 = batch[0][2]
        f, i = np.zeros(L.total), np.zeros(L.n_i64, dtype=np.int64)
        psd = L.view(f, "psd")
        gam_zone = np.ones(ng)
        refs = {}
        for z, (cells, gam_pf, _) in zip(zones, batch):
            slabs = ec.impulse_slabs(cells)
            for door in range(2):
                psd[z - 1 + door] = slabs[door, :NT, :NM]
                gam_zone[z - 1 + door] = gam_pf[door]
            refs[z] = (slabs, gam_pf)
        cc.set_gammas(prob, gam_zone)
        t = cc.tables(prob0, prob, i_ion)
        t.gam0 = gam0
        dndp, diag = be.dndp_cr(t, tallies=(f, i))
        diag_ref = np.zeros(2, dtype=np.int64)
        for z, (slabs, gam_pf) in refs.items():
            ref = ec.reference(slabs, t, gam_pf, nm, nt)
            diag_ref += ref.diag.sum(axis=0)
            for door in range(2):
                zz = z + door
                for m in range(3):
                    row, norm = cc.normalise_row(cc.F64, [float(v) for v in ref.dN[door, m, :nm + 1]], t.mom_edge_cgs, t.n0, t.gam0, prob.ux[1],
                                                 prob.gam_sf[zz], prob.ux[zz], t.zone_pop[zz - 1])
                    got = dndp[m, zz - 1, :nm + 1]
                    lit = ref.dndp[door, m, :nm + 1] > 1.0e-99
                    assert np.array_equal(got > 1.0e-99, lit), (zz, m, refs[z])
                    compared += 1
                    if not lit.any():
                        continue
                    assert norm > 0
                    rel = np.abs(got[lit] / norm - ref.dndp[door, m, :nm + 1][lit]) / ref.dndp[door, m, :nm + 1][lit]
                    worst = max(worst, float(rel.max()))
                    lit_bins += int(lit.sum())
                    assert rel.max() <= REL, (zz, m, float(rel.max()), refs[z])
        assert np.array_equal(diag, diag_ref)
        diag_all += diag_ref
    be.destroy()
    print(f"species {i_ion}: {compared} rows compared, {lit_bins} lit bins, worst relative difference {worst / cc.U:.2f} u, diag {diag_all.tolist()}")
    assert compared == 6 * len(launches) and lit_bins > len(launches) and np.all(diag_all > 0)


# ---- (c) the default plasma frames ------------------------------------------------------------------------------------------------------
class Recorder:
    """A backend that records what consumers.escape_spectra hands to dndp_esc."""
    def __init__(self, nm):
        self.nm, self.calls = nm, []

    def dndp_esc(self, tabs, gam_pf):
        self.calls.append((tabs, np.array(gam_pf, dtype=np.float64)))
        return np.full((2, 3, self.nm + 2), 1.0e-99), np.zeros((2, 3)), np.zeros((2, 2), dtype=np.int64)


def test_default_plasma_frames_follow_the_profile():
    prob = cc.small_problem()
    P = prob.params
    g = np.asarray(prob.gam_sf, dtype=np.float64).copy()
    g[1:P.n_grid + 1] = 1.0 + 0.01 * np.arange(1, P.n_grid + 1)          # a modified profile: every zone its own gamma
    prob.gam_sf = g
    assert 1 <= P.i_grid_feb < P.n_grid
    be = Recorder(P.num_psd_mom_bins)
    spec = mcs.consumers.escape_spectra(prob, be, 1)
    want = np.array([1.0 + 0.01 * P.i_grid_feb, 1.0 + 0.01 * P.n_grid])
    assert cc.bits_equal(spec.gam_pf, want) and cc.bits_equal(be.calls[0][1], want) and cc.bits_equal(mcs.consumers.escape_gam_pf(prob), want)
    assert spec.dndp.shape == (2, 3, P.num_psd_mom_bins + 2) and spec.number.shape == (2, 3) and spec.diag.shape == (2, 2)
    assert cc.bits_equal(spec.mom_edge_cgs, be.calls[0][0].mom_edge_cgs)
    spec = mcs.consumers.escape_spectra(prob, be, 1, gam_pf=(2.0, 3.0))
    assert cc.bits_equal(spec.gam_pf, [2.0, 3.0]) and cc.bits_equal(be.calls[1][1], [2.0, 3.0])


# ---- (d) refusals and slot numbers --------------------------------------------------------------------------------------------------------
def test_slot_numbers():
    e = ens.HostEnsemble(make_problem(64).params, 3)
    for s in range(3):
        slot = e.escape_slot(s)
        assert slot == s | (1 << 27) and e.is_escape(slot) and not e.is_products(slot) and not e.is_photons(slot) and not e.is_photons_all(slot)
        assert e.count(slot) == 0 and e.names(slot) == ("dNdp", "number", "slope")
        assert not e.is_escape(s) and not e.is_escape(e.products_slot(s)) and not e.is_escape(e.photons_slot(s))
    assert not e.is_escape(e.photons_all_slot) and not e.is_escape(e.iteration_slot) and not e.is_escape(-1)
    for bad in (-1, 3):
        with pytest.raises(ValueError, match="escape slot"):
            e.escape_slot(bad)
    with pytest.raises(ValueError, match="no species slot"):
        e.count(5 | (1 << 27))
    assert [e.escape_row(d, m) for d in range(2) for m in range(3)] == [(r, r + 1) for r in range(6)]
    with pytest.raises(ValueError, match="doors 0, 1"):
        e.escape_row(2, 0)
    NM = e.layout.escape["dNdp"][1][1]
    s = e.escape_slot(1)
    assert e.word_range(s, "dNdp", e.escape_row(1, 2), (3, 9)) == (5 * NM + 3, 6)
    assert e.word_range(s, "number", e.escape_row(0, 2)) == (6 * NM + 2, 1) and e.word_range(s, "slope") == (6 * NM + 6, 6)
    with pytest.raises(KeyError, match="dNdp_pf"):
        e.word_range(s, "dNdp_pf")
    with pytest.raises(ValueError, match="never taken a sample"):
        e.mean(s, "number")


def test_driver_refusals():
    prob = make_problem(64)
    be = oracle_backend(prob)
    e = ens.HostEnsemble(prob.params, 1)
    trig = ens.Trigger(e.escape_slot(0), "number", "max", 0.1, zones=e.escape_row(0, 2))
    with pytest.raises(ValueError, match="escape: needs finalize=True"):
        mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, escape=True)
    with pytest.raises(ValueError, match="escape slot needs escape=True"):
        mcs.driver.run(prob, be, n_itrs=2, max_pcuts=1, finalize=True, ensemble=e, triggers=[trig])
    with pytest.raises(ValueError, match="leaves the escape spectra out"):
        mcs.driver.run_overlapped(prob, [be], n_itrs=1, max_pcuts=1, escape=True)
    with pytest.raises(ValueError, match="leaves the escape spectra out"):
        mcs.driver.run_overlapped(prob, [be], n_itrs=2, max_pcuts=1, ensemble=True, triggers=[trig])
    assert e.count(0) == 0 and e.count(e.escape_slot(0)) == 0
    be.destroy()


def test_host_ensemble_takes_escape_samples():
    """The numpy accumulator's escape sample: dNdp and number as they come, the slopes of the six rows by the products rule."""
    prob = cc.small_problem()
    nm = prob.params.num_psd_mom_bins
    NM = nm + 2
    be = oracle_backend(prob)
    e = ens.HostEnsemble(prob.params, 1)
    rng = np.random.default_rng(2)
    specs = []
    for k in range(3):
        dndp = np.full((2, 3, NM), 1.0e-99)
        dndp[:, :, 2:20] = 10.0 ** rng.uniform(-5, 5, (2, 3, 18))
        dndp[1, 2, 4:] = 1.0e-99                     # two valid bins: no slope
        specs.append(mcs.consumers.EscapeSpectra(dndp, rng.uniform(1, 2, (2, 3)), np.zeros((2, 2), dtype=np.int64), np.ones(2), None))
    with pytest.raises(ValueError, match="no slope window"):
        e.add_escape(be, 0, specs[0])
    x_log = ens.bin_centres_log10(prob)
    e.set_slope_window(0, nm + 1, x_log)
    for s in specs:
        e.add_escape(be, 0, s)
    slot = e.escape_slot(0)
    assert e.count(slot) == 3 and e.count(0) == 0
    from ensemble_common import same_words, stat_of
    want = stat_of([dict(dNdp=s.dndp.reshape(6, NM), number=s.number.ravel()) for s in specs])
    assert same_words(e.mean(slot, "dNdp"), want.mean["dNdp"]) and same_words(e.m2(slot, "number"), want.m2["number"])
    slope = e.mean(slot, "slope")
    assert np.isnan(slope[5]) and np.all(np.isfinite(slope[:5]))
    with pytest.raises(ValueError, match="slope window stays"):
        e.set_slope_window(1, nm + 1, x_log)
    other = ens.HostEnsemble(prob.params, 1)
    other.merge(e)
    assert other.count(slot) == 3 and other.window[:2] == (0, nm + 1) and same_words(other.mean(slot, "slope"), slope)
    (s,) = e.summarize(slot, [ens.Request("dNdp", e.escape_row(0, 1), 0.0, 0.0, (2, 20))])
    assert s.n == 3 and s.n_selected == 18 and s.n_nonfinite == 0
    be.destroy()
