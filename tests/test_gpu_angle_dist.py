"""K11, mcs_angle_dist (csrc/mcs_consumers.hip: mcs_k_angle_dist) on crafted tallies against the restatement of tests/angles_common.py:
every output word bit for bit (a NaN as a NaN) -- the impulse sweep over every cell of the slab, dense tallies at the small and the
largest binning with both settings of therm_from_hist, the reproducibility of the bits, zones at rest -- then the partition of the
momentum range, the normalisation, that the call leaves the other consumers' results and the tallies alone, its refusals, and one real
run through driver.run(finalize=True, angles=[...])."""
import math

import numpy as np
import pytest

import angles_common as ac
import consumers_common as cc
from conftest import mcs, make_problem, hip_backend

pytestmark = pytest.mark.gpu

ens = mcs.ensemble


def binning(prob):
    return prob.params.num_psd_mom_bins, prob.params.num_psd_tht_bins


def call(hb, t, windows):
    return hb.angle_dist(t, [w[0] for w in windows], [w[1] for w in windows])


def test_impulse_sweep():
    """Every cell of the (nt+2) x (nm+2) slab once, one lit cell per zone: the last row and the last column, which take no part, the
    weights at, below and above 1e-66, the zone gammas on both sides of 1.000001, four gammas of the ISM frame.  Windows: the whole
    range, one single bin, two neighbours that share an edge, and one single bin that no image of the launch lies in."""
    prob0, prob = cc.small_problem(), cc.small_problem()
    P = prob.params
    nm, nt = binning(prob)
    ng = P.n_grid
    launches = ac.impulse_launches(prob)
    seen = {(j, k) for la in launches for j, k, _ in la[4].values()}
    assert len(seen) == (nm + 2) * (nt + 2) and {la[3] for la in launches} == {1.03142, 1.5, 5.0, 50.0}
    assert {g for la in launches for g in la[2].tolist()} == set(cc.GAMMAS)
    hb = hip_backend(prob)
    hb.begin_iteration(1)
    empty_rows = lit_rows = moved = 0
    try:
        for n, (f, i, gam_zone, gam0, cells) in enumerate(launches):
            cc.set_gammas(prob, gam_zone)
            hb.set_grid(prob)
            hb.write_tallies(f, i)
            t = cc.tables(prob0, prob, 1)
            t.gam0 = gam0
            reached = set()
            for z, (j, k, v) in cells.items():
                if j <= nt and k <= nm and v > cc.T66:
                    reached |= {k} | {int(ac.image_of(P, t, g)[1][j, k]) for g in (float(prob.gam_sf[z + 1]), gam0)}
            free = min(b for b in range(nm + 1) if b not in reached)
            windows = ((0, nm + 1), (5, 6), (10, 17), (17, 25), (free, free + 1))
            ref = ac.reference(prob, t, f, i, windows)
            ac.assert_equal_to_reference(call(hb, t, windows), ref, f"launch {n}, gam0 {gam0}")
            assert np.all(ref.number[:, :, 4] == 0.0)
            empty_rows += int((ref.number == 0.0).sum())
            lit_rows += int((ref.number > 0.0).sum())
            # the cells that take no part, and those that are not lit
            for z, (j, k, v) in cells.items():
                if j > nt or k > nm or not v > cc.T66:
                    assert np.all(ref.number[:, z] == 0.0), (z, j, k, v)
                else:
                    assert np.all(ref.number[:, z, 0] == v) and ref.dist[0, z, 0, j] > 1.0e-99
                    moved += int(ref.dist[1, z, 0, j] == 1.0e-99)
    finally:
        hb.destroy()
    print(f"{len(launches)} launches: {lit_rows} rows with a number, {empty_rows} empty rows, {moved} cells whose plasma-frame image left their angle row")
    assert empty_rows > lit_rows > 3 * len(launches) and moved > 10          # the empty rule and the common path were both met


DENSE = {"small": (cc.SMALL_BINNING, 1.0, None), "large": (cc.LARGE_BINNING, 0.25, (7, 8, 50, 51, 98))}


def dense_windows(nm):
    return ((0, nm + 1), (nm // 2, nm // 2 + 1), (nm // 8, nm // 3), (nm // 3, nm // 2), (3 * nm // 4, nm + 1), (nm // 16, 2 * nm // 3))


@pytest.mark.parametrize("size", list(DENSE))
def test_dense_tallies(size):
    kw, fill, zones = DENSE[size]
    prob0, prob = make_problem(64, **kw), make_problem(64, **kw)
    P = prob.params
    nm, nt = binning(prob)
    if size == "large":
        assert (nm, nt) == (199, 199)
    f, i = cc.dense_tallies(prob, seed=7, lit_zones=zones, fill=fill)
    lit_zones = [z - 1 for z in (zones or [z for z in range(1, P.n_grid + 1) if z % 5])]
    assert {int(i[z]) != 0 for z in lit_zones} == {False, True}          # crossings in some lit zones, none in others
    assert np.any(mcs.capi.Layout(P).view(f, "therm_sf")[lit_zones[0]] > 0)
    cc.set_gammas(prob, cc.dense_gammas(P.n_grid))
    windows = dense_windows(nm)
    hb = hip_backend(prob)
    hb.begin_iteration(1)
    try:
        hb.write_tallies(f, i)
        numbers = []
        for hist in (True, False):
            t = cc.tables(prob0, prob, 1, hist)
            ref = ac.reference(prob, t, f, i, windows)
            first = call(hb, t, windows)
            ac.assert_equal_to_reference(first, ref, f"{size}, therm_from_hist {hist}")
            assert np.all(ref.number[:, lit_zones, 0] > 0) and (ref.dist[:, lit_zones, 0] > 1.0e-99).mean() > 0.3
            assert np.all(ref.lit[lit_zones] > (0.15 if fill < 1 else 0.5) * (nm + 1) * (nt + 1))
            # the same tallies again: the same bits (no atomics; the error bars and comparisons of the ensemble rest on it)
            again = call(hb, t, windows)
            assert all(ac.same_words(a, b) for a, b in zip(again, first))
            numbers.append(ref.number)
        assert not cc.bits_equal(numbers[0], numbers[1])                  # (the thermal crossings counted)
    finally:
        hb.destroy()


@pytest.fixture(scope="module")
def small_dense():
    """The small binning, dense tallies, a context that holds them, and the tables."""
    prob0, prob = cc.small_problem(), cc.small_problem()
    f, i = cc.dense_tallies(prob, seed=9)
    hb = hip_backend(prob)
    hb.begin_iteration(1)
    hb.write_tallies(f, i)
    yield prob0, prob, f, i, hb
    hb.destroy()


def test_zones_at_rest(small_dense):
    """gamma = 1 in every zone: beta = 0 by the rule, the image of a cell is the cell, and frame 1 equals frame 0 bit for bit."""
    prob0, prob, f, i, hb = small_dense
    nm, nt = binning(prob)
    before = prob.gam_sf.copy()
    try:
        cc.set_gammas(prob, np.ones(prob.params.n_grid))
        hb.set_grid(prob)
        t = cc.tables(prob0, prob, 1)
        dist, number, moments = call(hb, t, dense_windows(nm))
        assert ac.same_words(dist[1], dist[0]) and ac.same_words(number[1], number[0]) and ac.same_words(moments[1], moments[0])
        assert not ac.same_words(dist[2], dist[0]) and np.any(number[0] > 0)
    finally:
        prob.gam_sf = before
        hb.set_grid(prob)


def test_partition_and_normalisation(small_dense):
    """Windows that partition [0, nm + 1): the number of the whole equals the sum of the parts within K_BOUND (lit cells + nt + parts +
    2) 2^-53 number (every weight is added once on either side, the parts' rows and the parts once more; all positive).  And
    sum_j dist[j] (cos_edge[j+1] - cos_edge[j]) = 1 within K_BOUND (nt + 5) 2^-53: number is the serial sum of the nt + 1 row sums, and
    a term takes three roundings (the two divisions and the test's product)."""
    prob0, prob, f, i, hb = small_dense
    P = prob.params
    nm, nt = binning(prob)
    cc.set_gammas(prob, cc.dense_gammas(P.n_grid))
    hb.set_grid(prob)
    t = cc.tables(prob0, prob, 1)
    parts = ((0, 7), (7, 8), (8, 20), (20, nm + 1))
    dist, number, moments = call(hb, t, ((0, nm + 1),) + parts)
    lit = cc.lit_cells_per_zone(mcs.capi.Layout(P), f, ("psd", "therm_sf"))
    whole = number[:, :, 0]
    total = number[:, :, 1] + number[:, :, 2] + number[:, :, 3] + number[:, :, 4]
    bound = cc.K_BOUND * (lit[None, :] + nt + len(parts) + 2) * cc.U * whole
    err = np.abs(total - whole)
    print("partition: worst error / bound", float(np.max(err[whole > 0] / bound[whole > 0])), "zones with a number:", int((whole[0] > 0).sum()))
    assert (whole > 0).sum() > 100 and np.all(err <= bound)
    dcos = np.diff(t.cos_edge)
    worst = 0.0
    for fr, z, m in zip(*np.nonzero(number > 0)):
        s = math.fsum((dist[fr, z, m, :nt + 1] * dcos).tolist())
        worst = max(worst, abs(s - 1.0))
    print("normalisation: worst |sum - 1| / bound", worst / (cc.K_BOUND * (nt + 5) * cc.U))
    assert worst <= cc.K_BOUND * (nt + 5) * cc.U
    empty = number == 0
    assert empty.any() and np.all(dist[empty] == 1.0e-99) and np.all(np.isnan(moments[empty])) and not np.isnan(moments[~empty]).any()


def test_the_call_leaves_the_others_alone():
    """dndp_cr and thermo_calcs before and after an angle_dist on the same tallies: identical bits (impulse tallies, one lit cell per
    zone, so that no bin of theirs takes two atomic adds whose order could differ from run to run); what they left on the device is
    still there for a products sample, the array of dndp_2d for photon_ic, the result of dndp_esc for an escape sample; the tallies are
    unchanged."""
    prob = cc.small_problem()
    nm, nt = binning(prob)
    hb = hip_backend(prob)
    hb.begin_iteration(1)
    try:
        la = cc.impulse_launches(prob, 1)[3]
        f, i = la.f.copy(), la.i.copy()
        hb.write_tallies(f, i)
        t = mcs.consumers.consumer_tables(prob, 1)
        dndp0, diag0 = hb.dndp_cr(t)
        thermo0 = hb.thermo_calcs(t)
        esc0 = hb.dndp_esc(t, (1.5, 1.03142))
        hb.dndp_2d(t, prob.params.gam0, prob.params.beta0, download=False)
        alpha_in, n_in = mcs.consumers.photon_field_cmb(0.3)
        ic_args = (t.mom_edge_cgs, t.mc, nt, alpha_in, n_in, 25, 1e-2, 10, 4 * math.pi * (3.0e24) ** 2 * 0.1)
        ic0 = hb.photon_ic(*ic_args)
        e = ens.HipEnsemble(hb, 1)
        e.set_slope_window(0, nm + 1, ens.bin_centres_log10(prob))
        dist, number, moments = call(hb, t, ((0, nm + 1), (3, 9)))
        assert (number > 0).sum() > 50
        ic1 = hb.photon_ic(*ic_args)                # K6's array is still there, and is what it was
        assert cc.bits_equal(ic1[1], ic0[1])
        e.add_products(hb, 0)
        e.add_escape(hb, 0)
        ps, xs = e.products_slot(0), e.escape_slot(0)
        for m, name in enumerate(("dNdp_sf", "dNdp_pf", "dNdp_isf")):
            assert cc.bits_equal(e.mean(ps, name), dndp0[m]), name
        for k, name in enumerate(("P_psd_par", "P_psd_perp", "energy_density_psd")):
            assert cc.bits_equal(e.mean(ps, name), thermo0[k]), name
        assert cc.bits_equal(e.mean(xs, "dNdp"), esc0[0].reshape(6, -1)) and cc.bits_equal(e.mean(xs, "number"), esc0[1].ravel())
        dndp1, diag1 = hb.dndp_cr(t)
        thermo1 = hb.thermo_calcs(t)
        assert cc.bits_equal(dndp1, dndp0) and np.array_equal(diag1, diag0)
        assert all(cc.bits_equal(a, b) for a, b in zip(thermo1, thermo0))
        f1, i1 = hb.read_tallies()
        assert cc.bits_equal(f1, f) and np.array_equal(i1, i)
        e.destroy()
    finally:
        hb.destroy()


def test_refusals(small_dense):
    prob0, prob, f, i, hb = small_dense
    nm, nt = binning(prob)
    t = cc.tables(prob0, prob, 1)
    good = call(hb, t, ((0, nm + 1),))
    for lo, hi in (([], []), ([0] * 9, [1] * 9), ([-1], [3]), ([3], [3]), ([5], [2]), ([0], [nm + 2]), ([0, 4], [nm + 1, nm + 2])):
        with pytest.raises(RuntimeError, match="mcs_angle_dist"):
            hb.angle_dist(t, lo, hi)
    t.gam0 = 0.5
    with pytest.raises(RuntimeError, match="Lorentz factor"):
        call(hb, t, ((0, nm + 1),))
    # a refused call changes nothing: the last good result is still what a sample takes
    e = ens.HipEnsemble(hb, 1)
    e.set_angle_windows([0], [nm + 1])
    e.add_angles(hb, 0)
    s = e.angles_slot(0)
    assert ac.same_words(e.mean(s, "number"), good[1].ravel()) and ac.same_words(e.mean(s, "dist"), good[0].reshape(-1, nt + 2))
    assert ac.same_words(e.mean(s, "mean_mu"), good[2][..., 0].ravel()) and ac.same_words(e.mean(s, "mean_mu2"), good[2][..., 1].ravel())
    e.destroy()


def test_one_real_run():
    """driver.run(finalize=True, angles=[...]) at N = 2e4, two iterations: one entry per species and iteration, each equal to the
    restatement on that species' downloaded tallies; and a run without angles= is what it was."""
    prob = make_problem(20000, num_iterations=4)
    P = prob.params
    nm, nt = binning(prob)
    n_sp = len(prob.cfg.species)
    x = 10.0 ** ens.bin_centres_log10(prob)
    angles = [(x[0] * 0.5, x[-1] * 2.0), (x[nm // 4], x[nm // 2]), (x[nm // 2] * 1.0001, x[3 * nm // 4])]
    hb = hip_backend(prob)
    try:
        res = mcs.driver.run(prob, hb, n_itrs=2, finalize=True, angles=angles)
        assert res.angles is not None and [(it, ion) for it, ion, _ in res.angles] == [(it, ion) for it in (1, 2) for ion in range(1, n_sp + 1)]
        windows = mcs.consumers.momentum_windows(prob, angles)
        assert windows[0] == (0, nm + 1) and windows[1][1] == windows[2][0]
        for (it, ion, d), (it2, ion2, f, i) in zip(res.angles, res.per_species):
            assert (it, ion) == (it2, ion2) and d.windows == windows
            t = mcs.consumers.consumer_tables(prob, ion)
            ref = ac.reference(prob, t, f, i, windows)
            ac.assert_equal_to_reference(d, ref, f"iteration {it}, species {ion}")
        first = res.angles[0][2]
        lit = first.number[0, :, 0] > 0
        print("protons, iteration 1: zones with particles", int(lit.sum()), "<mu> shock / plasma / ISM frame at the last zone:",
              first.mean_mu[:, P.n_grid - 1, 0].tolist())
        assert lit.sum() > P.n_grid // 2 and not ac.same_words(res.angles[0][2].number, res.angles[n_sp][2].number)
    finally:
        hb.destroy()
