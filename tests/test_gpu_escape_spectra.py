"""K10, mcs_dndp_esc (csrc/mcs_consumers.hip: mcs_k_dndp_esc_rows, mcs_k_dndp_esc_join) on crafted escape slabs against the
restatement of tests/escape_common.py: every output word bit for bit -- the impulse sweep over every cell of a slab, dense slabs at
the small and the largest binning, the reproducibility of the bits, the cells outside the written extent -- the conservation of the
summed weight, that the call leaves mcs_dndp_cr's results alone, and one real run through driver.run(finalize=True, escape=True)."""
import numpy as np
import pytest

import consumers_common as cc
import escape_common as ec
from conftest import mcs, make_problem, hip_backend
from ensemble_common import same_words, stat_of

pytestmark = pytest.mark.gpu

ens = mcs.ensemble


def binning(prob):
    return prob.params.num_psd_mom_bins, prob.params.num_psd_tht_bins


def run_esc(hb, slabs, t, gam_pf):
    ec.write_slabs(hb, slabs)
    return hb.dndp_esc(t, gam_pf)


def assert_equal_to_reference(got, ref, what):
    dndp, number, diag = got
    assert ec.bits_equal(dndp, ref.dndp), f"{what}: dNdp differs in {(dndp != ref.dndp).sum()} words"
    assert ec.bits_equal(number, ref.number), f"{what}: number {number.tolist()} != {ref.number.tolist()}"
    assert np.array_equal(diag, ref.diag), f"{what}: diag {diag.tolist()} != {ref.diag.tolist()}"


SPECIES = {"protons": (cc.small_problem, 1, None), "iron": (cc.three_species_problem, 2, 3), "electrons": (cc.three_species_problem, 3, 3)}


@pytest.mark.parametrize("species", list(SPECIES))
def test_impulse_sweep(species):
    """Every cell of the written part of a slab, last row and column included, in each door, against every gamma of cc.GAMMAS (three
    of them, rotating, for the Fe-like ion and the electrons); the weights walk cc.WEIGHTS, the ISM frame's gamma cc.GAMMAS too."""
    make, i_ion, n_gammas = SPECIES[species]
    prob = make()
    nm, nt = binning(prob)
    assert nm + 2 != ec.PM and nt + 2 != ec.PM                      # (the slab's stride is not the binning's)
    hb = hip_backend(prob)
    t = ec.escape_tables(prob, i_ion)
    launches = ec.impulse_launches(nm, nt, n_gammas)
    seen = {(door, j, i) for cells, _, _ in launches for door, (j, i, _) in enumerate(cells)}
    assert len(seen) == 2 * (nm + 2) * (nt + 2)
    diag_sum, lit = np.zeros((2, 2), dtype=np.int64), 0
    try:
        for n, (cells, gam_pf, gam0) in enumerate(launches):
            t.gam0 = gam0
            slabs = ec.impulse_slabs(cells)
            ref = ec.reference(slabs, t, gam_pf, nm, nt)
            assert_equal_to_reference(run_esc(hb, slabs, t, gam_pf), ref, f"launch {n}: cells {cells}, gam_pf {gam_pf}, gam0 {gam0}")
            diag_sum += ref.diag
            lit += int((ref.dndp[:, 1:] > 1.0e-99).sum())
    finally:
        hb.destroy()
    print(f"{species}: {len(launches)} launches, diag summed {diag_sum.tolist()}, lit bins of frames 1 and 2: {lit}")
    assert np.all(diag_sum > 0) and lit > len(launches)            # the error paths were met, and so was the common one


DENSE = {"small": (cc.SMALL_BINNING, 1.0, (1.5, cc.GAMMAS[4])), "large": (cc.LARGE_BINNING, 0.25, (1.03142, 50.0))}


@pytest.mark.parametrize("size", list(DENSE))
def test_dense_slabs(size):
    kw, fill, gam_pf = DENSE[size]
    prob = make_problem(64, **kw)
    nm, nt = binning(prob)
    if size == "large":
        assert nm == 199 and nt == 199
    hb = hip_backend(prob)
    t = ec.escape_tables(prob, 1)
    try:
        slabs = ec.dense_slabs(nm, nt, 11, fill)
        lit = (slabs[:, :nt + 1, :nm + 1] >= cc.T66).mean()
        assert lit > (0.6 if fill == 1.0 else 0.15)
        ref = ec.reference(slabs, t, gam_pf, nm, nt)
        first = run_esc(hb, slabs, t, gam_pf)
        assert_equal_to_reference(first, ref, size)
        assert (ref.dndp[:, :, :nm + 1] > 1.0e-99).mean() > 0.5 and np.all(ref.number > 0)
        # the same tallies again: the same bits (no atomics; the error bars and comparisons of the ensemble rest on it)
        again = hb.dndp_esc(t, gam_pf)
        assert ec.bits_equal(again[0], first[0]) and ec.bits_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
        # what lies outside the written extent is never read
        garbage = ec.dense_slabs(nm, nt, 11, fill, outside=1.0e30)
        assert ec.bits_equal(garbage[:, :nt + 2, :nm + 2], slabs[:, :nt + 2, :nm + 2])
        if nm + 2 < ec.PM:
            assert garbage[0, 0, nm + 2] == 1.0e30 and garbage[1, nt + 2, 0] == 1.0e30
            assert_equal_to_reference(run_esc(hb, garbage, t, gam_pf), ref, size + ", garbage outside the extent")
    finally:
        hb.destroy()


def test_conservation():
    """With no cell skipped and no search clamped every lit cell's weight v / gamma arrives in the bins: number of frames 1 and 2
    equals the sum over the cells >= 1e-66 of v / gamma within (IMPULSE_ERR_BOUND gamma^2 + n_adds 2^-53) sum |v / gamma|, n_adds the
    adds of the longest chain from a part to the number.  Without the first and the last momentum column, and with mild boosts, every transformed corner stays in the table."""
    prob = cc.small_problem()
    nm, nt = binning(prob)
    hb = hip_backend(prob)
    t = ec.escape_tables(prob, 1)
    t.gam0 = 1.25
    gam_pf = (1.03142, 1.5)
    try:
        full = ec.dense_slabs(nm, nt, 23)
        slabs = ec.empty_slabs()
        slabs[:, :nt + 1, 1:nm] = full[:, :nt + 1, 1:nm]          # (column 0 reaches below the table, column nm above it)
        ref = ec.reference(slabs, t, gam_pf, nm, nt)
        assert not np.any(ref.diag), ref.diag.tolist()
        dndp, number, diag = run_esc(hb, slabs, t, gam_pf)
        assert not np.any(diag)
        for door in range(2):
            v = slabs[door, :nt + 1, :nm + 1]
            v = v[v >= cc.T66]
            assert v.size > 100
            for m, gam in ((1, gam_pf[door]), (2, t.gam0)):
                w = v / gam
                want = float(np.sum(w.astype(np.longdouble)))
                bound = (cc.IMPULSE_ERR_BOUND * gam * gam + int(ref.n_adds[door, m]) * cc.U) * float(np.sum(np.abs(w)))
                err = abs(float(number[door, m]) - want)
                print(f"door {door} frame {m}: number {number[door, m]:.17g}, sum of weights {want:.17g}, error {err:.3e}, bound {bound:.3e}")
                assert err <= bound
    finally:
        hb.destroy()


def test_the_call_leaves_dndp_cr_alone():
    """dndp_cr and thermo_calcs before and after a dndp_esc on the same tallies: identical bits (impulse tallies in the psd, one lit
    cell per zone, so that no bin of theirs takes two atomic adds whose order could differ from run to run), and what they left on the
    device is still there for a products sample."""
    prob = cc.small_problem()
    nm, nt = binning(prob)
    hb = hip_backend(prob)
    try:
        la = cc.impulse_launches(prob, 1)[3]
        f, i = la.f.copy(), la.i.copy()
        L = mcs.capi.Layout(prob.params)
        slabs = ec.dense_slabs(nm, nt, 5)
        L.view(f, "esc_psd_up")[...] = slabs[0]; L.view(f, "esc_psd_down")[...] = slabs[1]
        hb.write_tallies(f, i)
        t = mcs.consumers.consumer_tables(prob, 1)
        dndp0, diag0 = hb.dndp_cr(t)
        thermo0 = hb.thermo_calcs(t)
        assert (dndp0[1] > 1.0e-99).sum() > 10 and np.any(thermo0[0] > 0)
        e = ens.HipEnsemble(hb, 1)
        e.set_slope_window(0, nm + 1, ens.bin_centres_log10(prob))
        esc = hb.dndp_esc(t, (1.5, 1.03142))
        assert np.all(esc[1] > 0)
        e.add_products(hb, 0)                       # the two consumers' results still count, and are what they were
        ps = e.products_slot(0)
        for m, name in enumerate(("dNdp_sf", "dNdp_pf", "dNdp_isf")):
            assert cc.bits_equal(e.mean(ps, name), dndp0[m]), name
        for k, name in enumerate(("P_psd_par", "P_psd_perp", "energy_density_psd")):
            assert cc.bits_equal(e.mean(ps, name), thermo0[k]), name
        dndp1, diag1 = hb.dndp_cr(t)
        thermo1 = hb.thermo_calcs(t)
        assert cc.bits_equal(dndp1, dndp0) and np.array_equal(diag1, diag0)
        assert all(cc.bits_equal(a, b) for a, b in zip(thermo1, thermo0))
        f1, i1 = hb.read_tallies()
        assert cc.bits_equal(f1, f) and np.array_equal(i1, i)
        e.destroy()
    finally:
        hb.destroy()


def test_one_real_run():
    """driver.run(finalize=True, escape=True, ensemble=...) at the golden fixtures' size (200 particles, every pcut), two iterations."""
    prob = make_problem(200, num_iterations=4)
    nm, nt = binning(prob)
    NM, NT = nm + 2, nt + 2
    n_sp = len(prob.cfg.species)
    hb = hip_backend(prob)
    e = ens.Ensemble.for_backend(hb, n_sp)
    try:
        res = mcs.driver.run(prob, hb, n_itrs=2, finalize=True, escape=True, ensemble=e)
        assert res.escape is not None and [(it, ion) for it, ion, _ in res.escape] == [(it, ion) for it in (1, 2) for ion in range(1, n_sp + 1)]
        L = hb.layout
        t = mcs.consumers.consumer_tables(prob, 1)
        dp = np.diff(t.mom_edge_cgs)
        for (it, ion, spec), (it2, ion2, f, _) in zip(res.escape, res.per_species):
            assert (it, ion) == (it2, ion2)
            assert not np.any(spec.diag), spec.diag.tolist()
            assert cc.bits_equal(spec.gam_pf, [prob.gam_sf[prob.params.i_grid_feb], prob.gam_sf[prob.params.n_grid]])
            for door, name in enumerate(("esc_psd_up", "esc_psd_down")):
                col = cc.shock_frame_row(L.view(f, name)[:NT, :NM])[:nm + 1]
                want = np.full(NM, 1.0e-99)
                with np.errstate(divide="ignore"):
                    want[:nm + 1] = np.where(col < cc.T66, 1.0e-99, col / dp)
                assert cc.bits_equal(spec.dndp[door, 0], want), (it, ion, door)
        protons = res.escape[0][2]
        print("protons, iteration 1: number", protons.number.tolist())
        assert protons.number[0][0] > 0
        print("lit bins of the protons' upstream door, iteration 1:", (protons.dndp[0] > 1.0e-99).sum(axis=1).tolist())
        for ion in range(1, n_sp + 1):
            s = e.escape_slot(ion - 1)
            assert e.count(s) == 2
            mine = [dict(dNdp=spec.dndp, number=spec.number.ravel()) for _, i2, spec in res.escape if i2 == ion]
            want = stat_of([{k: v.reshape(6, -1) if k == "dNdp" else v for k, v in m.items()} for m in mine])
            assert same_words(e.mean(s, "dNdp"), want.mean["dNdp"]) and same_words(e.m2(s, "dNdp"), want.m2["dNdp"])
            assert same_words(e.mean(s, "number"), want.mean["number"]) and same_words(e.m2(s, "number"), want.m2["number"])
    finally:
        e.destroy(); hb.destroy()


def test_species_on_a_second_context():
    """run(species_backends=[...], escape=True): a species that ran on a secondary context gets its spectra from THAT context's slabs
    (they do not travel with the running sums), before its merge; the ensemble's sample comes from there too."""
    S = mcs.inputs.Species
    prob = make_problem(200, num_iterations=2, species=[S(1.0, 1.0, 1e6, 1.0), S(4.0, 2.0, 1e6, 0.1), S(12.0, 6.0, 1e6, 0.01)])
    nm, nt = binning(prob)
    NM, NT = nm + 2, nt + 2
    hb, hb2 = hip_backend(prob), hip_backend(prob)
    e = ens.Ensemble.for_backend(hb, 3)
    try:
        res = mcs.driver.run(prob, hb, n_itrs=1, finalize=True, escape=True, ensemble=e, species_backends=[hb2])
        assert [k for _, _, k, _, _ in sorted(res.species_spans)] == [0, 1, 0]          # He ran on the secondary
        assert [(it, ion) for it, ion, _ in res.escape] == [(1, 1), (1, 2), (1, 3)]
        L = hb.layout
        dp = np.diff(mcs.consumers.consumer_tables(prob, 1).mom_edge_cgs)
        for (it, ion, spec), (_, _, f, _) in zip(res.escape, res.per_species):
            assert not np.any(spec.diag)
            for door, name in enumerate(("esc_psd_up", "esc_psd_down")):
                col = cc.shock_frame_row(L.view(f, name)[:NT, :NM])[:nm + 1]
                want = np.full(NM, 1.0e-99)
                want[:nm + 1] = np.where(col < cc.T66, 1.0e-99, col / dp)
                assert cc.bits_equal(spec.dndp[door, 0], want), (ion, door)
                assert (want > 1.0e-99).sum() > 3
            s = e.escape_slot(ion - 1)
            assert e.count(s) == 1 and cc.bits_equal(e.mean(s, "dNdp"), spec.dndp.reshape(6, NM)) and cc.bits_equal(e.mean(s, "number"), spec.number.ravel())
        assert not cc.bits_equal(res.escape[0][2].dndp, res.escape[1][2].dndp)
    finally:
        e.destroy(); hb.destroy(); hb2.destroy()
