"""The three photon fold kernels (csrc/mcs_consumers.hip: K5 mcs_k_photon_synch, K6 mcs_k_photon_ic, K7 mcs_k_photon_pion) term by
term on the device, through the C ABI, against the mpmath reference of photon_fold_common.py -- which shares no code with
include/mcs_synch.h, mcs_ic.h and mcs_pion.h, the headers that kernel and CPU twin both compile.

Term by term: the calls and points of test_photon_folds_host.py, the reference evaluated at the energies the call returns, the
bound computed for the device's libm (photon_fold_common.DEVICE).  Sum structure: a dense spectrum is the ordered sum of the
device's own impulse outputs -- bit for bit for K5 and K7, which pins loop bounds, order and indexing with no tolerance (K6: see
photon_fold_common.ic_sum_structure).  Zones, shapes, and the points test_photon_pion.py::test_gpu_pion_matches_cpu_twin excuses."""
import numpy as np
import pytest

import photon_fold_common as pf
from conftest import hip_backend, make_problem, oracle_backend

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device_libm():
    pf.use_libm(pf.DEVICE)
    yield
    pf.use_libm(pf.GLIBC)


@pytest.fixture(scope="module")
def electrons():
    prob = pf.synch_problem()
    hb = hip_backend(prob)
    yield hb, prob
    hb.destroy()


@pytest.fixture(scope="module")
def protons():
    prob = pf.pion_problem()
    hb = hip_backend(prob)
    yield hb, prob
    hb.destroy()


# ---- K5 ----------------------------------------------------------------------------------------------------------------------------
def test_gpu_synch_impulses(electrons):
    hb, prob = electrons
    pf.synch_term_by_term(hb, prob, "K5 device", "impulses").check(min_lit=800, branches=pf.K5_BRANCHES[:5])


def test_gpu_synch_thresholds(electrons):
    hb, prob = electrons
    pf.synch_term_by_term(hb, prob, "K5 device", "thresholds").check(min_lit=200, branches=pf.K5_BRANCHES)


def test_gpu_synch_field_cuts():
    prob = pf.synch_problem(flat=False)
    hb = hip_backend(prob)
    pf.synch_field_cuts(hb, prob, "K5 device").check(min_lit=50, branches=("skip:B<1e-20", "skip:w_c<1e-55", "F_small"))
    hb.destroy()


def test_gpu_synch_sum_structure_stock(electrons):
    hb, prob = electrons
    assert pf.synch_sum_structure(hb, prob) == 0.0


def test_gpu_synch_sum_structure_largest_binning():
    prob = pf.large_problem()
    hb = hip_backend(prob)
    assert pf.synch_sum_structure(hb, prob, seed=13, pe=pf.electron_edges(201)) == 0.0
    hb.destroy()


def test_gpu_synch_zones_and_shapes(electrons):
    hb, prob = electrons
    pf.synch_zones(hb, prob)
    pf.synch_shapes(hb, prob, "K5 device").check(min_lit=100)


# ---- K7 ----------------------------------------------------------------------------------------------------------------------------
def test_gpu_pion_impulses(protons):
    hb, prob = protons
    pf.pion_term_by_term(hb, prob, "K7 device", "impulses").check(min_lit=2000)


@pytest.mark.parametrize("half", [0, 1])
def test_gpu_pion_thresholds(protons, half):
    hb, prob = protons
    cases = pf.PION_CASES[4 * half:4 * half + 4]                 # protons with the four data sets; helium and iron
    want = [b for b in pf.K7_BRANCHES if half == 0 or not b.endswith(",d2")]
    T = pf.pion_term_by_term(hb, prob, "K7 device", "thresholds", cases)
    T.check(min_lit=400, branches=want)
    assert half == 0 or pf.PION_TP_HIT <= T.exact_hits, T.exact_hits         # bins whose T_p IS a branch point: < against <=


def test_gpu_pion_sum_structure_stock(protons):
    hb, prob = protons
    assert pf.pion_sum_structure(hb, prob) < 0.01


def test_gpu_pion_sum_structure_largest_binning():
    prob = pf.large_problem()
    hb = hip_backend(prob)
    assert pf.pion_sum_structure(hb, prob, seed=14) < 0.01
    hb.destroy()


def test_gpu_pion_zones_and_shapes(protons):
    hb, prob = protons
    pf.pion_zones(hb, prob)
    pf.pion_shapes(hb, prob, "K7 device").check(min_lit=100)


def test_gpu_pion_excused_points_are_undecidable():
    """The five parameter sets of test_photon_pion.py::test_gpu_pion_matches_cpu_twin: every output at which device and twin differ
    by more than that test's 1e-6 sits, in some lit bin of its zone, within the reference's bound of a decision (the kinematic
    limit X = 1 or a branch point of T_p)."""
    from test_photon_pion import _synthetic
    prob = make_problem(64)
    t, pe, d, target = _synthetic(prob, seed=9)
    ob, hb = oracle_backend(prob), hip_backend(prob)
    n_excused = 0
    for aa, scaling, n_photon, emin, bpd, i_data in pf.PION_TWIN_SETS:
        mc = aa * pf.MPROT * pf.C
        Eo, o = ob.photon_pion(d, pe, mc, aa, target, scaling, n_photon, emin, bpd, i_data)
        Eg, g = hb.photon_pion(d, pe, mc, aa, target, scaling, n_photon, emin, bpd, i_data)
        assert np.array_equal(Eo, Eg)
        edge = np.abs(np.log(np.maximum(g, 1e-99) / np.maximum(o, 1e-99))) > 1e-6
        for z, j in zip(*np.nonzero(edge)):
            n_excused += 1
            open_bins = pf.pion_point_undecidable(d[z], pe, mc, aa, i_data, target[z], scaling, Eg[j])
            print("excused:", (aa, i_data, n_photon), "zone", z, "energy", j, "device", g[z, j], "twin", o[z, j], "open bins", open_bins)
            assert open_bins, (aa, i_data, z, j, g[z, j], o[z, j])
    print("excused points in all five sets:", n_excused)
    ob.destroy(); hb.destroy()


# ---- K6 ----------------------------------------------------------------------------------------------------------------------------
def test_gpu_ic_impulses(electrons):
    hb, prob = electrons
    pf.ic_term_by_term(pf.IcSide(hb, prob), "K6 device", "impulses").check(min_lit=2000)


def test_gpu_ic_thresholds(electrons):
    hb, prob = electrons
    pf.ic_term_by_term(pf.IcSide(hb, prob), "K6 device", "thresholds").check(min_lit=100, branches=pf.K6_BRANCHES)


def test_gpu_ic_cone_and_field_shapes(electrons):
    hb, prob = electrons
    pf.ic_shapes(pf.IcSide(hb, prob), "K6 device").check(min_lit=150)


def test_gpu_ic_n_photon_shapes(electrons):
    hb, prob = electrons
    pf.ic_shapes_n_photon(pf.IcSide(hb, prob), "K6 device").check(min_lit=100)


def test_gpu_ic_sum_structure_stock(electrons):
    hb, prob = electrons
    pf.ic_sum_structure(pf.IcSide(hb, prob))


def test_gpu_ic_sum_structure_largest_binning():
    prob = pf.large_problem()
    hb = hip_backend(prob)
    pf.ic_sum_structure(pf.IcSide(hb, prob, pe=pf.electron_edges(201)), seed=16, pool=24)
    hb.destroy()
