"""The tally consumer kernels (csrc/mcs_consumers.hip: mcs_k_dndp_cr, mcs_k_thermo, mcs_k_dndp_2d) cell by cell on crafted tallies,
against the oracle on identical tallies (written to both with write_tallies) and against the references of consumers_common.py.

Impulse tier: one lit cell per zone, so that every output bin receives at most one add per frame and every block sum adds one
non-zero to zeros: no freedom in the order of the adds is left, and device and oracle must agree BIT FOR BIT in dN/dp of all three
frames, diag, the three thermo outputs and the whole dndp_2d array -- over every cell of the slab, every gamma class of the zone
(beta = 0 branch and its threshold included), the 1e-66 threshold weights, three species, the num_crossings branches and four dndp_2d
frames.  Dense tier: every output against the exactly rounded sum of its own addends, with the bound derived in consumers_common.py;
once on the small binning, once on the largest binning mcs_create accepts (nm = nt = 199).
"""
import numpy as np
import pytest

import consumers_common as cc
from conftest import hip_backend, mcs, oracle_backend

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("species", ["protons", "iron", "electrons"])
def test_gpu_impulse_sweep_is_bit_equal_to_the_oracle(species):
    sw = cc.impulse_sweeps(only=species)[species]
    prob = sw.prob
    hb = hip_backend(prob)
    hb.begin_iteration(1)
    total = np.zeros(2, dtype=np.int64)
    for n, run in enumerate(sw.runs):
        la = run["la"]
        prob.gam_sf = run["gsf"]
        hb.set_grid(prob)
        hb.write_tallies(la.f, la.i)
        d_g, g_g = hb.dndp_cr(run["t"][1])
        assert g_g.tolist() == run["diag"].tolist(), (n, g_g, run["diag"])
        total += g_g
        for m, frame in enumerate(("shock", "plasma", "ISM")):
            assert cc.bits_equal(d_g[m], run["dndp"][m]), (n, frame, _first_difference(d_g[m], run["dndp"][m], la))
        for h in (0, 1):
            th_g = np.array(hb.thermo_calcs(run["t"][h]))
            assert cc.bits_equal(th_g, run["thermo"][h]), (n, "thermo", h, _first_difference(th_g.T, run["thermo"][h].T, la))
            d2_g = hb.dndp_2d(run["t"][h], *run["frame"])
            assert cc.bits_equal(d2_g, run["d2"][h]), (n, "dndp_2d", h, run["frame"], _first_difference(d2_g, run["d2"][h], la))
    hb.destroy()
    assert total[0] > 0 and total[1] > 0, total
    print(species, "launches:", len(sw.runs), "diag over the sweep:", total.tolist())


def _first_difference(a, b, la):
    """(zone, index..., device, oracle, the zone's lit cell) of the first entry that differs: the message of a failing comparison."""
    bad = np.argwhere(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64))
    if not len(bad):
        return None
    idx = tuple(int(v) for v in bad[0])
    return len(bad), idx, float(a[idx]), float(b[idx]), la.cells.get(idx[0] + 1), float(la.gam_zone[idx[0]])


def _dense_check(prob0, prob, f, i, zones=None, frames=cc.FRAMES_2D, hists=(True, False)):
    """Device and oracle on the same dense tallies, each against the reference with its per-output bound; masks equal everywhere."""
    P = prob.params
    be, hb = oracle_backend(prob), hip_backend(prob)
    hb.begin_iteration(1)
    hb.write_tallies(f, i)
    zs = slice(None) if zones is None else [z - 1 for z in zones]
    worst = {}
    t = cc.tables(prob0, prob, 1)
    d_o, g_o = be.dndp_cr(t, tallies=(f, i))
    d_g, g_g = hb.dndp_cr(t)
    ref, bound, rdiag = cc.dndp_cr_reference(prob, t, f, zones)
    assert g_g.tolist() == g_o.tolist()
    if zones is None:
        assert g_o.tolist() == rdiag.tolist()
    assert np.array_equal(d_g > 1e-90, d_o > 1e-90) and np.array_equal(d_o[:, zs] > 1e-90, ref[:, zs] > 1e-90)
    assert cc.bits_equal(d_g[0], d_o[0]), "shock-frame dN/dp is summed in the reference's order: bit-exact"
    for who, d in (("device", d_g), ("oracle", d_o)):
        r, rest = cc.excess(d[:, zs], ref[:, zs], bound[:, zs])
        worst["dndp_cr " + who] = r
        assert rest and r <= 1.0, (who, r)
    if zones is not None:                    # the zones without a reference are dark
        dark = np.ones(P.n_grid, dtype=bool); dark[zs] = False
        assert cc.bits_equal(d_g[:, dark], d_o[:, dark]) and not (d_o[:, dark] > 1e-90).any()
    for hist in hists:
        t = cc.tables(prob0, prob, 1, hist)
        for gx, bx in frames:
            gx, bx = (P.gam0, P.beta0) if gx is None else (gx, bx)
            ref, bound = cc.dndp_2d_reference(prob, t, f, i, gx, bx)
            o, g = be.dndp_2d(t, gx, bx, tallies=(f, i)), hb.dndp_2d(t, gx, bx)
            assert np.array_equal(g > 1e-90, ref > 1e-90) and np.array_equal(o > 1e-90, ref > 1e-90)
            for who, d in (("device", g), ("oracle", o)):
                r, rest = cc.excess(d, ref, bound)
                worst["dndp_2d " + who] = max(r, worst.get("dndp_2d " + who, 0.0))
                assert rest and r <= 1.0, (who, gx, hist, r)
        ref, bound = cc.thermo_reference(prob, t, f, i)
        for who, d in (("device", np.array(hb.thermo_calcs(t))), ("oracle", np.array(be.thermo_calcs(t, tallies=(f, i))))):
            r, rest = cc.excess(d, ref, bound)
            worst["thermo " + who] = max(r, worst.get("thermo " + who, 0.0))
            assert rest and r <= 1.0, (who, hist, r)
    be.destroy(); hb.destroy()
    return worst


def test_gpu_dense_every_output_against_its_own_addends():
    prob0, prob = cc.small_problem(), cc.small_problem()
    f, i = cc.dense_tallies(prob)
    cc.set_gammas(prob, cc.dense_gammas(prob.params.n_grid))
    print("dense, nm = 32, nt = 9: worst |x - ref| / bound:", _dense_check(prob0, prob, f, i))


def test_gpu_dense_at_the_largest_binning():
    """nm = nt = 199: 201 entries per axis in the kernels' 208-entry LDS tables, 157 passes of the 256 threads over a zone's 40 000
    cells.  Two zones are lit, a quarter of their cells (the one-cell form of dndp_cr's reference costs 20 us per cell and frame in
    Python); every zone's dndp_2d and thermo output has its reference."""
    prob0, prob = cc.small_problem(**cc.LARGE_BINNING), cc.small_problem(**cc.LARGE_BINNING)
    P = prob.params
    assert (P.num_psd_mom_bins, P.num_psd_tht_bins) == (199, 199)
    zones = (7, P.i_shock + 2)
    f, i = cc.dense_tallies(prob, seed=11, lit_zones=zones, fill=0.25)
    cc.set_gammas(prob, cc.dense_gammas(P.n_grid))
    print("dense, nm = 199, nt = 199: worst |x - ref| / bound:",
          _dense_check(prob0, prob, f, i, zones=zones, frames=cc.FRAMES_2D[:1] + cc.FRAMES_2D[3:], hists=(True,)))
