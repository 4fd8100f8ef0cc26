"""The tally consumers cell by cell on crafted tallies, CPU side: the oracle (oracle/mcs_consumers.cpp) against restatements that share
no code with it (tests/consumers_common.py), every output judged against its own size and never against the largest entry of its array.

Impulse tier: one lit psd cell per zone, every cell of the slab x every gamma class x the threshold weights, three species.  The fp64
one-cell form must equal the oracle bit for bit (it does: the two are the same operations in the same order, mcsm::log10 included);
the 60-digit form bounds what the oracle's arithmetic costs, in units of the cell's own weight.  Dense tier: power laws over 80
decades; each bin against the exactly rounded sum of its own parts with the bound (adds) x 2^-53 x (sum of |parts|).
"""
import numpy as np
import pytest

import consumers_common as cc
from conftest import mcs, oracle_backend
from test_consumers import thermo_numpy
from test_photon_ic import dndp_2d_numpy


@pytest.fixture(scope="module")
def sweeps():
    return cc.impulse_sweeps()


def _one_cell_rows(A, sw, run, z, j, k, v):
    """The one-cell form's normalised rows of zone z in the plasma and the ISM frame, and the counts the cell adds to diag."""
    prob, P = sw.prob, sw.prob.params
    t = run["t"][1]
    nm = P.num_psd_mom_bins
    lb = [float(x) for x in t.mom_log_cgs]
    rows, diag = [], [0, 0]
    for gam in (float(run["gsf"][z]), float(P.gam0)):
        parts, e, c = cc.cell_parts(A, (t.mom_edge_cgs[k], t.mom_edge_cgs[k + 1]), (t.cos_edge[j], t.cos_edge[j + 1]), v, t.rest_energy, gam, lb, nm)
        diag[0] += e; diag[1] += c
        dN = [A.num(0.0)] * (nm + 1)
        for l, p in parts:
            dN[l] = dN[l] + p
        row, norm = cc.normalise_row(A, dN, t.mom_edge_cgs, t.n0, t.gam0, prob.ux[1], run["gsf"][z], prob.ux[z], t.zone_pop[z - 1])
        rows.append((row, norm, gam, e))
    return rows, diag


def test_fp64_form_equals_the_oracle_bit_for_bit(sweeps):
    """dN/dp of all three frames and diag over the whole impulse sweep.  The error and clamp paths are taken: diag is non-zero in both
    entries and equal to the count of the one-cell form."""
    seen = {}
    for name, sw in sweeps.items():
        P = sw.prob.params
        nm, nt = P.num_psd_mom_bins, P.num_psd_tht_bins
        total = np.zeros(2, dtype=np.int64)
        gammas, cells = set(), set()
        for run in sw.runs:
            la, d = run["la"], run["dndp"]
            psd = mcs.capi.Layout(P).view(la.f, "psd")
            want_diag = [0, 0]
            for z in range(1, P.n_grid + 1):
                t = run["t"][1]
                sf, _ = cc.normalise_row(cc.F64, cc.shock_frame_row(psd[z - 1])[:nm + 1].tolist(), t.mom_edge_cgs, t.n0, t.gam0, sw.prob.ux[1],
                                         run["gsf"][z], sw.prob.ux[z], t.zone_pop[z - 1])
                assert cc.bits_equal(d[0, z - 1, :nm + 1], sf), (name, z, "shock frame")
                assert d[0, z - 1, nm + 1] == psd[z - 1][:, nm + 1].sum()         # (one lit cell: the sum is that cell)
                if z not in la.cells:
                    assert np.all(d[1:, z - 1, :nm + 1] == 1e-99) and np.all(d[1:, z - 1, nm + 1] == 0)
                    continue
                j, k, v = la.cells[z]
                cells.add((j, k)); gammas.add(float(run["gsf"][z]))
                if j > nt or k > nm:                                              # the CR loops ignore row nt+1 and column nm+1
                    assert np.all(d[1:, z - 1, :nm + 1] == 1e-99) and np.all(d[1:, z - 1, nm + 1] == 0), (name, z, j, k)
                    continue
                rows, dg = _one_cell_rows(cc.F64, sw, run, z, j, k, v)
                want_diag[0] += dg[0]; want_diag[1] += dg[1]
                for m in (1, 2):
                    assert cc.bits_equal(d[m, z - 1, :nm + 1], rows[m - 1][0]), (name, z, j, k, v, rows[m - 1][2], m)
            assert run["diag"].tolist() == want_diag, name
            total += run["diag"]
        assert len(cells) == (nm + 2) * (nt + 2) and gammas == set(cc.GAMMAS)
        assert total[0] > 0 and total[1] > 0, (name, total)
        seen[name] = total.tolist()
    print("diag over the sweeps:", seen)


def test_oracle_against_the_high_precision_form(sweeps):
    """|oracle - 60-digit form| of a cell's normalised row, summed over the bins, in units of the cell's own weight psd / gamma.  The
    Lorentz transform of a forward corner cancels, p_x - beta E / c ~ p / (2 gamma^2), so the fp64 error grows with gamma^2 of the frame:
    the figure is kept per gamma^2 (consumers_common.IMPULSE_ERR_*).  Weights next to the 1e-66 threshold are left to the fp64 form: a
    1e-15 leak there switches a bin between lit and unlit, which is the whole weight."""
    A = cc.MP()
    worst = {}
    n = 0
    for name, sw in sweeps.items():
        P = sw.prob.params
        nm, nt = P.num_psd_mom_bins, P.num_psd_tht_bins
        for run in sw.runs:
            d = run["dndp"]
            t = run["t"][1]
            dp = [A.num(t.mom_edge_cgs[l + 1]) - A.num(t.mom_edge_cgs[l]) for l in range(nm + 1)]
            for z, (j, k, v) in run["la"].cells.items():
                if j > nt or k > nm or v not in (1.0, 1.0e60):
                    continue
                rows, _ = _one_cell_rows(A, sw, run, z, j, k, v)
                rows64, _ = _one_cell_rows(cc.F64, sw, run, z, j, k, v)
                for m in (1, 2):
                    row, norm, gam, e = rows[m - 1]
                    if e or rows64[m - 1][3]:
                        assert e == rows64[m - 1][3], (name, z, j, k, "the error paths of identify_corners differ between the arithmetics")
                        continue
                    w = A.num(v) / A.num(gam)
                    err = A.num(0.0)
                    for l in range(nm + 1):
                        a = A.num(d[m, z - 1, l]) if d[m, z - 1, l] > 1e-99 else 0
                        b = row[l] if row[l] > 1e-99 else 0
                        err = err + abs(a - b) * dp[l]
                    err = float(err / norm / w) / gam ** 2
                    n += 1
                    if err > worst.get(name, (0.0,))[0]:
                        worst[name] = (err, z, j, k, v, gam, m)
    print("cells compared:", n, "worst error / gamma^2 [cell weights]:", worst)
    assert n > 3000
    for name, w in worst.items():
        assert w[0] <= cc.IMPULSE_ERR_BOUND, (name, w)


def test_impulse_thermo_and_dndp_2d_against_numpy(sweeps):
    """The other two consumers on the same launches against the vectorised restatements of test_consumers.py and test_photon_ic.py,
    per zone and per cell: an output is one addend here, so the two may differ by the few roundings of a differently associated
    product.  Fixes the spellings of the 1e-66 threshold (w <= 1e-66 skipped in thermo_calcs, w > 1e-66 taken in get_dNdp_2D) and
    the three num_crossings branches; the cold branch must give the exact 1/3 : 2/3 : 3/2 split."""
    tol = 32 * cc.U
    branches = set()
    for name, sw in sweeps.items():
        prob, P = sw.prob, sw.prob.params
        L = mcs.capi.Layout(P)
        for run in sw.runs[::3]:
            la = run["la"]
            prob.gam_sf = run["gsf"]
            for h in (0, 1):
                t = run["t"][h]
                want = thermo_numpy(prob, t, la.f, la.i, L)
                got = run["thermo"][h]
                assert np.all(np.abs(got - want) <= tol * np.abs(want)), (name, h, float(np.max(np.abs(got - want) / np.abs(want))))
                w2, _ = dndp_2d_numpy(prob, t, la.f, la.i, L, *run["frame"])
                g2 = run["d2"][h]
                assert np.array_equal(g2 > 1e-90, w2 > 1e-90), (name, h)
                assert np.all(np.abs(g2 - w2) <= tol * w2), (name, h)
                for z in range(1, P.n_grid + 1):
                    lit_psd = z in la.cells and la.cells[z][2] > cc.T66 and la.cells[z][0] <= P.num_psd_tht_bins and la.cells[z][1] <= P.num_psd_mom_bins
                    lit_th = bool(h) and L.view(la.f, "therm_pf")[z - 1].max() > cc.T66
                    nc = int(la.i[z - 1])
                    if not lit_psd and not lit_th and nc == 0:
                        pc = t.cold_pressure[z - 1]
                        assert got[0, z - 1] == 1.0 / 3 * pc and got[1, z - 1] == 2.0 / 3 * pc and got[2, z - 1] == 1.5 * pc, (name, z)
                        branches.add("cold")
                    elif nc == 0:
                        branches.add("no crossings, lit")
                    else:
                        branches.add("crossings")
    assert branches == {"cold", "no crossings, lit", "crossings"}


def test_large_binning_sits_at_the_limit():
    """The Config of the largest-binning GPU case reaches MCS_PSD_MAX - 1 bins on both axes: one more and mcs_create refuses."""
    P = cc.small_problem(**cc.LARGE_BINNING).params
    assert P.num_psd_mom_bins + 1 == 200 and P.num_psd_tht_bins + 1 == 200


# ---- dense tier ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    prob0 = cc.small_problem()
    prob = cc.small_problem()
    f, i = cc.dense_tallies(prob)
    cc.set_gammas(prob, cc.dense_gammas(prob.params.n_grid))
    return prob0, prob, f, i


def test_dense_tallies_span_the_decades(dense):
    prob0, prob, f, i = dense
    psd = mcs.capi.Layout(prob.params).view(f, "psd")
    lit = [z for z in range(prob.params.n_grid) if psd[z].max() > 0]
    assert 0 < len(lit) < prob.params.n_grid
    for z in lit:
        c = psd[z][psd[z] > cc.T66]
        assert np.log10(c.max() / c.min()) > 60, z
        assert (psd[z] == 0).any() and (psd[z] == 1e-99).any()


def test_dense_dndp_cr_every_bin_against_its_own_parts(dense):
    """consumers_common.dndp_cr_reference states the bound and its derivation; no bin is exempt."""
    prob0, prob, f, i = dense
    be = oracle_backend(prob)
    t = cc.tables(prob0, prob, 1)
    got, diag = be.dndp_cr(t, tallies=(f, i))
    be.destroy()
    ref, bound, rdiag = cc.dndp_cr_reference(prob, t, f)
    assert diag.tolist() == rdiag.tolist() and diag[0] > 0 and diag[1] > 0
    assert np.array_equal(got > 1e-90, ref > 1e-90)
    r, rest_equal = cc.excess(got, ref, bound)
    print("dndp_cr dense: worst |oracle - ref| / bound =", r, "lit bins:", int((ref > 1e-90).sum()),
          "decades of lit outputs:", float(np.log10(ref[ref > 1e-90].max() / ref[ref > 1e-90].min())))
    assert rest_equal and r <= 1.0


@pytest.mark.parametrize("hist", [True, False])
def test_dense_dndp_2d_and_thermo_against_their_own_addends(dense, hist):
    prob0, prob, f, i = dense
    P = prob.params
    be = oracle_backend(prob)
    t = cc.tables(prob0, prob, 1, hist)
    for gx, bx in cc.FRAMES_2D:
        gx, bx = (P.gam0, P.beta0) if gx is None else (gx, bx)
        got = be.dndp_2d(t, gx, bx, tallies=(f, i))
        ref, bound = cc.dndp_2d_reference(prob, t, f, i, gx, bx)
        assert np.array_equal(got > 1e-90, ref > 1e-90)
        r, rest_equal = cc.excess(got, ref, bound)
        print("dndp_2d dense, frame", gx, ": worst / bound =", r)
        assert rest_equal and r <= 1.0, (gx, r)
    got = np.array(be.thermo_calcs(t, tallies=(f, i)))
    be.destroy()
    ref, bound = cc.thermo_reference(prob, t, f, i)
    r, rest_equal = cc.excess(got, ref, bound)
    print("thermo dense: worst / bound =", r)
    assert rest_equal and r <= 1.0
