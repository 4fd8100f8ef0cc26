"""mcs_ens_compare (csrc/mcs_ensemble.hip) and what is built on it -- ensemble.HipEnsemble.compare, ensemble.Agreement,
ensemble.check_agreements -- against the plain-numpy restatement of ens_compare_common.py, on its crafted pair of sample sets:
five samples against four on the stock binning, 100 decades of dynamic range, the 1e-99 floor in every seventh word (z = 0), one
word in 25 constant on either side (degenerate), a block of zones of psd 1.5 times off, three words whose |z| tie."""
import ctypes as ct

import numpy as np
import pytest

from conftest import mcs, make_problem, hip_backend
from ensemble_common import AS_IS, INCREMENTS, assert_tail_is_exercised, bits_equal
from ens_summary_common import iteration_offsets, same_bits, slot_vectors, species_offsets
from ens_compare_common import (FIELDS, N_A, N_B, TIE, as_dict, assert_exact, assert_same_bits, assert_sums, check_recipe, compare_ranges,
                                crafted_pair, restate, species_vectors, value_of)
from test_gpu_ens_products import consume, shaped_buffers, slot_words

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
R, D = mcs.capi.McsEnsCmpRange, mcs.capi.McsEnsDifference


def feed(hb, e, bufs, L, slot=0, iteration=True):
    """Every buffer as a species sample of `slot` and, with iteration, as an iteration sample (as test_gpu_ens_summary.feed)."""
    prev = np.zeros(L.total)
    for f, i in bufs:
        if iteration:
            hb.write_tallies(prev, i)
            e.begin_iteration(hb)
        hb.write_tallies(f, i)
        e.add_species(hb, slot)
        if iteration:
            e.add_iteration(hb)
        prev = f


def raw_compare(a, slot_a, b, slot_b, ranges):
    """One mcs_ens_compare call for ranges [(first, count, floor_frac, zcut)] -> [dict of FIELDS]."""
    rs = (R * len(ranges))(*[R(*r) for r in ranges])
    out = (D * len(ranges))()
    rc = a.lib.mcs_ens_compare(a.h, slot_a, b.h, slot_b, len(ranges), rs, out)
    assert rc == 0, a.lib.mcs_last_error().decode()
    return [{k: getattr(o, k) for k in FIELDS} for o in out]


def restated(va, vb, n_a, n_b, ranges):
    return [restate(va[0][f:f + c], va[1][f:f + c], n_a, vb[0][f:f + c], vb[1][f:f + c], n_b, ff, zcut) for f, c, ff, zcut in ranges]


@pytest.fixture(scope="module")
def crafted():
    prob = make_problem(64)
    L = mcs.capi.Layout(prob.params)
    bufs_a, bufs_b = crafted_pair(L)
    # the recipe's conditions on the restatement alone, before anything of the package's ensemble module is looked at
    check_recipe(L, species_vectors(L, bufs_a), species_vectors(L, bufs_b))
    assert_tail_is_exercised(ens.EnsLayout(prob.params).fields)
    hb = hip_backend(prob)
    a, b = ens.HipEnsemble(hb, 1), ens.HipEnsemble(hb, 1)
    feed(hb, a, bufs_a, L)
    feed(hb, b, bufs_b, L)
    sp_off, sp_total = species_offsets(L)
    it_off, it_total = iteration_offsets(L, INCREMENTS + AS_IS)
    assert sp_total == a.layout.species_total and it_total == a.layout.iteration_total
    vec = {(e, slot): slot_vectors(e, slot) for e in (a, b) for slot in (0, 1)}
    # the ranges of both slots, one call each, and the restatement of every range: computed once, shared by the tests
    ranges = {0: compare_ranges(L, sp_off, sp_total), 1: [(0, it_total, ff, 3.0) for ff in (0.0, 1e-3, 1.0)]}
    for name, (first, shape) in it_off.items():
        ranges[1] += [(first, int(np.prod(shape)), 1e-3, 2.0), (first, int(np.prod(shape)), 1.0, 2.0)]
    ranges[1] += [(1, it_total - 2, 1e-3, 1.0), (it_total - 1, 1, 0.0, 0.0), (it_total, 0, 0.0, 0.0)]
    want = {slot: restated(vec[a, slot], vec[b, slot], N_A, N_B, ranges[slot]) for slot in (0, 1)}
    got = {slot: raw_compare(a, slot, b, slot, ranges[slot]) for slot in (0, 1)}
    yield dict(prob=prob, L=L, bufs=(bufs_a, bufs_b), hb=hb, a=a, b=b, sp_off=sp_off, it_off=it_off, vec=vec, ranges=ranges, want=want, got=got)
    a.destroy(); b.destroy(); hb.destroy()


def test_exact_fields_and_sums(crafted):
    c = crafted
    worst = 0.0
    for slot in (0, 1):
        assert len(c["ranges"][slot]) <= 256
        for r, got, want in zip(c["ranges"][slot], c["got"][slot], c["want"][slot]):
            assert_exact(got, want, f"slot {slot} range {r}")
            assert_sums(got, want, f"slot {slot} range {r}")
            assert r[1] == 0 or want["n_selected"] >= 1, r
            assert want["n_nonfinite"] == 0
            for k in ("sum_abs_z", "sum_z2", "sum_abs_diff", "sum_scale"):
                if want[k] > 0:
                    worst = max(worst, abs(got[k] - want[k]) / want[k] / 2.0 ** -53)
    print(f"sums against fsum: worst difference {worst:.2f} units of 2^-53 relative (the bound is n_selected of them)")
    whole = c["want"][0][0]
    assert 0 < whole["n_over"] < whole["n_selected"] - whole["n_degenerate"] and whole["n_degenerate"] > 0
    # Ensemble.compare maps names, zones and bins to these ranges
    a, b, ng = c["a"], c["b"], c["prob"].params.n_grid
    reqs = [ens.CompareRequest(name, None, 1e-3, 2.0) for name in c["sp_off"]] + [ens.CompareRequest("psd", (10, 37), 1e-3, 3.0)]
    for q, d in zip(reqs, a.compare(b, 0, reqs)):
        first, count = a.word_range(0, q.name, q.zones)
        k = c["ranges"][0].index((first, count, q.floor_frac, q.zcut))
        assert as_dict(d) == c["got"][0][k] and (d.n_a, d.n_b) == (N_A, N_B), q
    first, shape = c["it_off"]["spectra_sf"]
    k = c["ranges"][1].index((first, int(np.prod(shape)), 1e-3, 2.0))
    full, zoned = a.compare(b, 1, [ens.CompareRequest("spectra_sf", None, 1e-3, 2.0), ens.CompareRequest("spectra_sf", (0, ng), 1e-3, 2.0)])
    assert as_dict(full) == as_dict(zoned) == c["got"][1][k]
    q = ens.CompareRequest("psd_mom", (45, 46), 0.0, 3.0, (10, 90))
    first, count = a.word_range(0, "psd_mom", (45, 46), (10, 90))
    assert count == 80 and as_dict(a.compare(b, 0, [q])[0]) == raw_compare(a, 0, b, 0, [(first, count, 0.0, 3.0)])[0]


def test_repeatable_and_symmetric(crafted):
    c = crafted
    some_sign = False
    for slot in (0, 1):
        again = raw_compare(c["a"], slot, c["b"], slot, c["ranges"][slot])
        back = raw_compare(c["b"], slot, c["a"], slot, c["ranges"][slot])
        for r, x, y, z in zip(c["ranges"][slot], again, c["got"][slot], back):
            assert_same_bits(x, y, f"slot {slot} range {r}, a second call")
            assert_same_bits(z, y, f"slot {slot} range {r}, B against A", but_sign_of_sum_z=True)
            some_sign = some_sign or (y["sum_z"] != 0.0 and z["sum_z"] == -y["sum_z"])
    assert some_sign


def test_ties_keep_the_lower_word(crafted):
    c = crafted
    n_psd = int(np.prod(c["L"].shapes["psd"]))
    rs, got = c["ranges"][0], c["got"][0]
    whole, floor, pair, pair1 = (rs.index(r) for r in ((0, n_psd, 0.0, 3.0), (TIE[0], TIE[1] - TIE[0] + 1, 1.0, 3.0), (TIE[1], 2, 0.0, 3.0),
                                                        (TIE[1], 2, 1.0, 1e9)))
    assert TIE[1] - TIE[0] > 8192          # (more than two blocks' words apart: the two meet in the join of the partials)
    assert got[whole]["argmax"] == TIE[0] and got[floor]["argmax"] == 0 and got[floor]["n_selected"] == 2
    assert got[pair]["argmax"] == got[pair1]["argmax"] == 0 and got[pair]["n_selected"] == 2 and got[pair1]["n_over"] == 0
    for k in (floor, pair, pair1):
        assert same_bits(got[k]["max_abs_z"], got[whole]["max_abs_z"]) and got[k]["max_abs_z"] > 1e5


def test_non_finite_words_are_counted_and_left_out(crafted):
    c = crafted
    L, hb = c["L"], c["hb"]
    n_psd = int(np.prod(L.shapes["psd"]))
    bufs_a = [(f.copy(), i) for f, i in c["bufs"][0]]
    bufs_b = [(f.copy(), i) for f, i in c["bufs"][1]]
    nan_word, inf_word, huge = 4098, 250000, 9001
    extra = bufs_b[0][0].copy()
    extra[nan_word], extra[inf_word] = np.nan, np.inf
    bufs_b.append((extra, bufs_b[0][1]))                     # one extra sample of B
    bufs_a[3][0][huge] = 1e200                               # a finite mean, 2e199, with an M2 that overflowed -- in A only
    flux = L.offsets["pxx_flux"]
    bufs_a[1][0][flux + 40] = -np.inf
    a, b = ens.HipEnsemble(hb, 1), ens.HipEnsemble(hb, 1)
    feed(hb, a, bufs_a, L, iteration=False)
    feed(hb, b, bufs_b, L, iteration=False)
    va, vb = slot_vectors(a, 0), slot_vectors(b, 0)
    assert np.isfinite(va[0][huge]) and np.isinf(va[1][huge]) and np.isfinite(vb[1][huge]) and abs(va[0][huge]) > 1e199
    assert np.isnan(vb[0][nan_word]) and not np.isfinite(vb[0][inf_word]) and np.isfinite(va[0][[nan_word, inf_word]]).all()
    sp = c["sp_off"]
    ranges = [(0, n_psd, 1e-3, 3.0), (0, n_psd, 0.0, 3.0), (0, va[0].size, 1e-3, 3.0), (nan_word, 2, 0.0, 0.0), (nan_word, 1, 0.0, 0.0),
              (sp["pxx_flux"][0], L.n_grid, 1e-3, 2.0), (sp["psd_mom"][0], int(np.prod(sp["psd_mom"][1])), 1e-3, 2.0), (8000, 2001, 1.0, 0.0),
              (huge, 1, 0.0, 0.0)]
    got = raw_compare(a, 0, b, 0, ranges)
    for r, g, w in zip(ranges, got, restated(va, vb, N_A, N_B + 1, ranges)):
        assert_exact(g, w, f"range {r}")
        assert_sums(g, w, f"range {r}")
    assert got[0]["n_nonfinite"] == 3 and got[3]["n_nonfinite"] == 1 and got[3]["n_selected"] == 1
    assert got[4]["n_nonfinite"] == 1 and got[4]["n_selected"] == 0 and got[4]["argmax"] == -1 and got[4]["amax"] == 0.0
    assert got[8]["n_nonfinite"] == 1 and got[8]["amax"] == 0.0
    assert got[5]["n_nonfinite"] == 1 and got[5]["n_selected"] >= 1 and got[6]["n_nonfinite"] >= 1
    # amax is that of the finite words: the tie's 5e40, not the 2e199
    assert same_bits(got[0]["amax"], c["got"][0][c["ranges"][0].index((0, n_psd, 0.0, 3.0))]["amax"]) and got[7]["n_selected"] >= 1
    # an agreement over such a part is not met, whatever its value
    for name in ("psd", "pxx_flux"):
        t = ens.Agreement(0, name, "weighted_diff", 1e9)
        row = ens.check_agreements(a, b, [t])[0]
        assert row.difference.n_nonfinite > 0 and row.value <= t.threshold and not row.met
    assert ens.check_agreements(a, b, [ens.Agreement(0, "pxz_flux", "weighted_diff", 1e9)])[0].met
    a.destroy(); b.destroy()


def test_two_slots_of_one_accumulator(crafted):
    c = crafted
    L, hb = c["L"], c["hb"]
    both = ens.HipEnsemble(hb, 2)
    feed(hb, both, c["bufs"][0], L, 0, iteration=False)
    feed(hb, both, c["bufs"][1], L, 1, iteration=False)
    for k, slot in enumerate((0, 1)):
        for x, y in zip(slot_vectors(both, slot)[:2], c["vec"][(c["a"], c["b"])[k], 0]):
            assert bits_equal(x, y)
    got = raw_compare(both, 0, both, 1, c["ranges"][0])
    for r, x, y in zip(c["ranges"][0], got, c["got"][0]):
        assert_same_bits(x, y, f"range {r}: slots 0 and 1 of one accumulator against two accumulators")
    d = both.compare(both, 0, [ens.CompareRequest("psd", None, 0.0, 3.0)], other_slot=1)[0]
    n_psd = int(np.prod(L.shapes["psd"]))
    assert as_dict(d) == c["got"][0][c["ranges"][0].index((0, n_psd, 0.0, 3.0))] and (d.n_a, d.n_b) == (N_A, N_B)
    both.destroy()


def test_products_slots(crafted):
    c = crafted
    prob, L, hb = c["prob"], c["L"], c["hb"]
    ng, NM = prob.params.n_grid, prob.params.num_psd_mom_bins + 2
    tabs = mcs.consumers.consumer_tables(prob, 1)
    x_log = ens.bin_centres_log10(prob)
    a, b, other = ens.HipEnsemble(hb, 1), ens.HipEnsemble(hb, 1), ens.HipEnsemble(hb, 1)
    for e, window, seeds in ((a, (0, NM - 1), (0, 1, 2)), (b, (0, NM - 1), (10, 11)), (other, (1, NM - 1), (20, 21))):
        e.set_slope_window(*window, x_log)
        for seed in seeds:
            hb.write_tallies(*shaped_buffers(L, seed))
            consume(hb, tabs)
            e.add_products(hb, 0)
    ps = a.products_slot(0)
    va, vb = slot_words(a, ps), slot_words(b, ps)
    z = ng - 1
    reqs = [ens.CompareRequest("dNdp_pf", (z, z + 1), 1e-6, 2.0, (60, 111)), ens.CompareRequest("dNdp_sf", (7, 8), 0.0, 1.0, (0, NM)),
            ens.CompareRequest("slope_sf", None, 0.0, 2.0), ens.CompareRequest("slope_pf", (2, 50), 0.5, 2.0), ens.CompareRequest("P_psd_par", None, 0.0, 3.0),
            ens.CompareRequest("dNdp_isf", None, 1e-9, 3.0)]
    got = a.compare(b, ps, reqs)
    for q, d in zip(reqs, got):
        first, count = a.word_range(ps, q.name, q.zones, q.bins)
        s_ = slice(first, first + count)
        with np.errstate(invalid="ignore"):
            want = restate(va[0][s_], va[1][s_], 3, vb[0][s_], vb[1][s_], 2, q.floor_frac, q.zcut)
        assert (d.n_a, d.n_b) == (3, 2)
        assert_exact(as_dict(d), want, repr(q))
        assert_sums(as_dict(d), want, repr(q))
    assert got[0].n_selected > 0 and got[1].n_selected > 0
    # zone 0 has nothing above the floor in either set: its slope is NaN, and counted
    assert got[2].n_nonfinite >= 1 and got[2].n_selected >= 1 and np.isnan(va[0][a.word_range(ps, "slope_sf")[0]])
    assert not ens.Agreement(ps, "slope_sf", "weighted_diff", 1e9).met(got[2])
    # accumulators whose slope windows differ, a products slot against a species slot, a products slot never sampled
    fresh = ens.HipEnsemble(hb, 1)
    before = slot_words(a, ps)
    for who, call in (("slope windows differ", lambda: a.compare(other, ps, reqs)), ("slope windows differ", lambda: other.compare(a, ps, reqs)),
                      ("never taken a sample", lambda: a._compare(fresh, ps, ps, 3, 0, [(0, 1, 0.0, 0.0)])),
                      ("kind or length", lambda: a._compare(c["a"], ps, 0, 3, 5, [(0, 1, 0.0, 0.0)]))):
        with pytest.raises(RuntimeError, match="mcs_ens_compare.*" + who):
            call()
    with pytest.raises(ValueError, match="products slot with a species slot"):
        a.compare(c["a"], ps, reqs, other_slot=0)
    after = slot_words(a, ps)
    assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(before, after))
    assert as_dict(a.compare(b, ps, reqs[:1])[0]) == as_dict(got[0])
    for e in (a, b, other, fresh):
        e.destroy()


def test_refusals_change_nothing(crafted):
    c = crafted
    hb, a, b = c["hb"], c["a"], c["b"]
    lib = a.lib
    one = ens.HipEnsemble(hb, 2)                        # slot 1 of it: a species slot with one sample; slot 0: none
    hb.write_tallies(*c["bufs"][0][-1])
    one.add_species(hb, 1)
    hb2 = hip_backend(make_problem(64, num_psd_bins_per_decade=(8, 10)))
    odd = ens.HipEnsemble(hb2, 1)                       # another layout
    total, it_total = c["vec"][a, 0][0].size, c["vec"][a, 1][0].size
    out = (D * 257)()
    nan = float("nan")

    def rng(first, count, ff=1e-3, zcut=3.0):
        return (R * 1)(R(first, count, ff, zcut))
    refused = [
        ("null argument", lambda: lib.mcs_ens_compare(None, 0, b.h, 0, 1, rng(0, 1), out)),
        ("null argument", lambda: lib.mcs_ens_compare(a.h, 0, None, 0, 1, rng(0, 1), out)),
        ("null argument", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, None, out)),
        ("null argument", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, rng(0, 1), None)),
        ("slot", lambda: lib.mcs_ens_compare(a.h, 2, b.h, 0, 1, rng(0, 1), out)),
        ("slot", lambda: lib.mcs_ens_compare(a.h, 0, b.h, -1, 1, rng(0, 1), out)),
        ("slot", lambda: lib.mcs_ens_compare(a.h, 0, b.h, (1 << 30) | 1, 1, rng(0, 1), out)),
        ("same slot", lambda: lib.mcs_ens_compare(a.h, 0, a.h, 0, 1, rng(0, 1), out)),
        ("same slot", lambda: lib.mcs_ens_compare(b.h, 1, b.h, 1, 1, rng(0, 1), out)),
        ("kind or length", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 1, 1, rng(0, 1), out)),
        ("kind or length", lambda: lib.mcs_ens_compare(a.h, 1, a.h, 0, 1, rng(0, 1), out)),
        ("kind or length", lambda: lib.mcs_ens_compare(a.h, 1, one.h, 1, 1, rng(0, 1), out)),      # iteration slot against a species slot
        ("layouts differ", lambda: lib.mcs_ens_compare(a.h, 0, odd.h, 0, 1, rng(0, 1), out)),
        ("layouts differ", lambda: lib.mcs_ens_compare(odd.h, 0, a.h, 0, 1, rng(0, 1), out)),
        ("two samples", lambda: lib.mcs_ens_compare(a.h, 0, one.h, 1, 1, rng(0, 1), out)),         # n_b = 1
        ("two samples", lambda: lib.mcs_ens_compare(one.h, 1, a.h, 0, 1, rng(0, 1), out)),         # n_a = 1
        ("two samples", lambda: lib.mcs_ens_compare(a.h, 0, one.h, 0, 1, rng(0, 1), out)),         # n_b = 0
        ("n_ranges", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, -1, rng(0, 1), out)),
        ("n_ranges", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 257, (R * 257)(), out)),
        ("outside", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, rng(-1, 2), out)),
        ("outside", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, rng(total - 1, 2), out)),
        ("outside", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, rng(total + 1, 0), out)),
        ("outside", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, rng(0, -1), out)),
        ("outside", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, rng(2 ** 62, 2 ** 62), out)),
        ("outside", lambda: lib.mcs_ens_compare(a.h, 1, b.h, 1, 1, rng(0, it_total + 1), out)),
        ("floor_frac", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, rng(0, 1, nan), out)),
        ("floor_frac", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, rng(0, 1, -0.1), out)),
        ("floor_frac", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, rng(0, 1, 1.5), out)),
        ("zcut", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, rng(0, 1, 1e-3, -1.0), out)),
        ("zcut", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 1, rng(0, 1, 1e-3, nan), out)),
        ("range 1", lambda: lib.mcs_ens_compare(a.h, 0, b.h, 0, 2, (R * 2)(R(0, 1, 0.0, 0.0), R(0, 1, 2.0, 0.0)), out)),      # the second range of a call
    ]
    for k, (why, call) in enumerate(refused):
        assert call() != 0, k
        msg = lib.mcs_last_error()
        assert b"mcs_ens_compare" in msg and why.encode() in msg, (k, why, msg)
    assert lib.mcs_ens_compare(a.h, 0, b.h, 0, 0, None, None) == 0                # nothing to do
    # the Python layer refuses what it can see before the library is asked
    for exc, call in ((ValueError, lambda: a.compare(one, 0, [ens.CompareRequest("psd")], other_slot=1)),
                      (ValueError, lambda: a.compare(a, 0, [ens.CompareRequest("psd")])),
                      (ValueError, lambda: a.compare(b, 0, [ens.CompareRequest("psd")], other_slot=1)),
                      (ValueError, lambda: a.compare(odd, 0, [ens.CompareRequest("psd")])),
                      (ValueError, lambda: a.compare(ens.HostEnsemble(c["prob"].params, 1), 0, [ens.CompareRequest("psd")]))):
        with pytest.raises(exc):
            call()
    for e in (a, b):
        for slot in (0, 1):
            mean, m2 = slot_vectors(e, slot)
            assert bits_equal(mean, c["vec"][e, slot][0]) and bits_equal(m2, c["vec"][e, slot][1])
            assert e.count(slot) == (N_A if e is a else N_B)
    # the contexts and the accumulators go on working
    for slot, k in ((0, 1), (1, 0)):
        assert raw_compare(a, slot, b, slot, [c["ranges"][slot][k]])[0] == c["got"][slot][k]
    one.add_species(hb, 1)
    assert one.compare(a, 1, [ens.CompareRequest("pxx_flux")], other_slot=0)[0].n_a == 2
    one.destroy(); odd.destroy(); hb2.destroy()


N_PCUTS = 6
ONE_WAVE = (1, 64)          # (one wave per launch, as plain_run of test_gpu_ens_summary.py)


def test_driver_runs_compared_through_check_agreements():
    """Two runs of three iterations each over different iteration numbers -- a null pair -- and check_agreements on their
    ensembles: every row is the restatement of the slot vectors it was taken from.  No statistical threshold is asserted."""
    prob = make_problem(300, num_iterations=6)
    runs = []
    for first_iter in (1, 4):
        hb = hip_backend(prob)
        hb.set_launch(*ONE_WAVE)
        e = ens.Ensemble.for_backend(hb, 1)
        mcs.driver.run(prob, hb, n_itrs=3, max_pcuts=N_PCUTS, ensemble=e, first_iter=first_iter, fused_pcuts=False)
        assert e.count(0) == e.count(1) == 3
        runs.append((hb, e))
    (hb_a, a), (hb_b, b) = runs
    A = ens.Agreement
    rules = [A(0, "pxx_flux", "max_z", 5.0), A(0, "psd_mom", "chi2_per_word", 3.0, floor_frac=1e-4), A(1, "spectra_sf", "fraction_over", 0.5, zcut=2.0),
             A(0, "energy_flux", "mean_z", 1.0, zones=(prob.params.n_grid // 2, prob.params.n_grid)), A(0, "psd", "weighted_diff", 1.0, floor_frac=0.0),
             A(0, "psd_mom", "max_z", 5.0, zones=(prob.params.n_grid - 1, prob.params.n_grid), bins=(1, 100))]
    rows = ens.check_agreements(a, b, rules)
    assert [row.agreement for row in rows] == rules
    vec = {(e, slot): slot_vectors(e, slot) for e in (a, b) for slot in (0, 1)}
    for row in rows:
        t = row.agreement
        first, count = a.word_range(t.slot, t.name, t.zones, t.bins)
        s_ = slice(first, first + count)
        (ma, qa), (mb, qb) = vec[a, t.slot], vec[b, t.other_slot]
        want = restate(ma[s_], qa[s_], 3, mb[s_], qb[s_], 3, t.floor_frac, t.zcut)
        # (six pcuts couple nothing yet: the iteration slot's spectra are empty, and the row says so)
        assert (row.difference.n_a, row.difference.n_b) == (3, 3) and (want["n_selected"] > 0 or t.slot == 1), t
        assert_exact(as_dict(row.difference), want, repr(t))
        assert_sums(as_dict(row.difference), want, repr(t))
        # (the sums are within their bounds of the restatement's, so the value is that of the row's own difference)
        assert same_bits(row.value, t.value(row.difference)) and row.met == t.met(row.difference)
        if t.statistic in ("max_z", "fraction_over"):
            assert same_bits(row.value, value_of(t.statistic, want))
        print(t.name, t.statistic, row.value, row.met, "degenerate:", row.difference.n_degenerate, "selected:", row.difference.n_selected)
    for hb, e in runs:
        e.destroy(); hb.destroy()
