"""The comparison of two ensemble slots without a GPU: the crafted pair of ens_compare_common.py meets its recipe on the
restatement alone; ensemble.HostEnsemble.compare and ensemble.difference_of against that restatement; the name / zone / bin
mapping of ensemble.CompareRequest; ensemble.Agreement and check_agreements; the refusals of the Python layer; the exported symbol."""
import ctypes as ct
import dataclasses
import math

import numpy as np
import pytest

from conftest import mcs, make_problem
from ensemble_common import AS_IS, INCREMENTS, bits_equal
from ens_summary_common import iteration_offsets, same_bits, slot_vectors, species_offsets
from ens_compare_common import (N_A, N_B, SHIFTED_ZONES, TIE, UNSHIFTED_ZONES, as_dict, assert_exact, assert_same_bits, assert_sums, check_recipe,
                                compare_ranges, crafted_pair, restate, species_vectors, swapped, value_of)

ens = mcs.ensemble


class _Buffers:
    """The least a backend is to the host accumulator: the parameters and a tally buffer to read and write."""

    def __init__(self, prob):
        self.P = prob.params
        self.layout = mcs.capi.Layout(self.P)
        self.f, self.i = np.zeros(self.layout.total), np.zeros(self.layout.n_i64, dtype=np.int64)

    def read_tallies(self):
        return self.f.copy(), self.i.copy()

    def write_tallies(self, f, i):
        self.f, self.i = np.array(f, dtype=np.float64), np.array(i, dtype=np.int64)


def feed(be, e, bufs, L, slot=0, iteration=True):
    prev = np.zeros(L.total)
    for f, i in bufs:
        be.write_tallies(prev, i)
        if iteration:
            e.begin_iteration(be)
        be.write_tallies(f, i)
        e.add_species(be, slot)
        if iteration:
            e.add_iteration(be)
        prev = f


@pytest.fixture(scope="module")
def pair():
    prob = make_problem(64)
    L = mcs.capi.Layout(prob.params)
    bufs_a, bufs_b = crafted_pair(L)
    # the recipe's conditions on the restatement alone, before anything of the package's ensemble module is looked at
    va, vb = species_vectors(L, bufs_a), species_vectors(L, bufs_b)
    whole = check_recipe(L, va, vb)
    be = _Buffers(prob)
    a, b = ens.HostEnsemble(prob.params, 1), ens.HostEnsemble(prob.params, 1)
    feed(be, a, bufs_a, L)
    feed(be, b, bufs_b, L)
    return prob, L, a, b, (va, vb), whole


def test_host_compare_equals_the_restatement(pair):
    prob, L, a, b, (va, vb), whole = pair
    sp_off, sp_total = species_offsets(L)
    it_off, it_total = iteration_offsets(L, INCREMENTS + AS_IS)
    ng, NM = prob.params.n_grid, prob.params.num_psd_mom_bins + 2
    assert a.count(0) == a.count(1) == N_A and b.count(0) == b.count(1) == N_B
    # the accumulator's vectors are the restatement's
    for e, v in ((a, va), (b, vb)):
        mean, m2 = slot_vectors(e, 0)
        assert bits_equal(mean, v[0]) and bits_equal(m2, v[1])
    for slot, table in ((0, sp_off), (1, it_off)):
        (ma, qa), (mb, qb) = slot_vectors(a, slot), slot_vectors(b, slot)
        reqs = [ens.CompareRequest(name, None, ff, 2.0) for name in table for ff in (0.0, 1e-3, 1.0) if ff > 0 or np.prod(table[name][1]) < 1e5]
        reqs += [ens.CompareRequest(name, (3, ng - 5), 1e-3, 1.0) for name in table if name in ens.ZONE_PARTS]
        if slot == 0:
            reqs += [ens.CompareRequest("psd", SHIFTED_ZONES, 0.0, 3.0), ens.CompareRequest("psd", UNSHIFTED_ZONES, 0.0, 3.0),
                     ens.CompareRequest("psd_mom", (45, 46), 0.0, 3.0, (10, 90)), ens.CompareRequest("therm_pf_tht", (ng - 1, ng), 1e-3, 0.5, (1, 2))]
        got = a.compare(b, slot, reqs)
        assert len(got) == len(reqs)
        for q, s in zip(reqs, got):
            first, shape = table[q.name]
            count = int(np.prod(shape))
            if q.zones is not None:
                per = count // shape[0]
                first, count = first + q.zones[0] * per, (q.zones[1] - q.zones[0]) * per
                if q.bins is not None:
                    first, count = first + q.bins[0], q.bins[1] - q.bins[0]
            assert a.word_range(slot, q.name, q.zones, q.bins) == (first, count), q
            s_ = slice(first, first + count)
            want = restate(ma[s_], qa[s_], N_A, mb[s_], qb[s_], N_B, q.floor_frac, q.zcut)
            assert s.n_a == N_A and s.n_b == N_B and want["n_selected"] >= 1, q
            assert_exact(as_dict(s), want, f"slot {slot} {q}")
            assert_sums(as_dict(s), want, f"slot {slot} {q}")
    # raw ranges through difference_of: odd ends, one word, no word, the ties
    (ma, qa), (mb, qb) = slot_vectors(a, 0), slot_vectors(b, 0)
    for first, count, ff, zcut in compare_ranges(L, sp_off, sp_total)[-16:] + [(0, sp_total, 0.0, 3.0)]:
        s_ = slice(first, first + count)
        got = as_dict(ens.difference_of(ma[s_], qa[s_], N_A, mb[s_], qb[s_], N_B, ff, zcut))
        want = restate(ma[s_], qa[s_], N_A, mb[s_], qb[s_], N_B, ff, zcut)
        assert_exact(got, want, f"range {(first, count, ff, zcut)}")
        assert_sums(got, want, f"range {(first, count, ff, zcut)}")
    assert_exact(got, whole, "the whole species vector")
    s = a.compare(b, 0, [ens.CompareRequest("psd", (0, 1), 1.0, 3.0)])[0]
    assert s.argmax == TIE[0] and s.n_selected == len(TIE)
    s = a.compare(b, 0, [ens.CompareRequest("pxx_flux", (7, 7))])[0]
    assert as_dict(s) == restate([], [], N_A, [], [], N_B, 1e-3, 3.0) and s.argmax == -1 and s.amax == 0.0


def test_difference_of_handles_non_finite_degenerate_and_tied_words():
    #              0    1     2       3    4    5       6    7     8     9
    ma = np.array([1.0, -4.0, np.nan, 2.0, 4.0, 1e308, 8.0, 0.0, 1e-9, 3.0])
    qa = np.array([0.5, 8.0, 1.0, np.nan, 8.0, 1.0, np.inf, 3.0, 0.0, 0.0])
    mb = np.array([1.25, -2.0, 1.0, 2.0, 2.0, -1e308, 8.0, 0.0, 1e-9, 4.0])
    qb = np.array([0.5, 8.0, 1.0, 1.0, 8.0, 1.0, 1.0, 3.0, 0.0, 0.0])
    for ff, zcut in ((0.0, 0.5), (1e-3, 1.0), (1.0, 0.0)):
        got, want = as_dict(ens.difference_of(ma, qa, 4, mb, qb, 3, ff, zcut)), restate(ma, qa, 4, mb, qb, 3, ff, zcut)
        assert_exact(got, want)
        assert_sums(got, want)
        # words 2, 3 (a NaN), 5 (d overflows), 6 (an infinite M2): no finite words, and the 8.0 and the 1e308 are not amax
        assert got["n_nonfinite"] == 4 and got["amax"] == 4.0
    d = ens.difference_of(ma, qa, 4, mb, qb, 3, 0.0, 0.5)
    assert d.n_selected == 5 and d.n_degenerate == 1          # words 0, 1, 4, 8 (z = 0), 9 (degenerate); the zero scale is never selected
    assert d.argmax == 1                                      # words 1 and 4 tie in |z| (z = -2 / s and 2 / s): the lower one
    assert d.sum_abs_diff == math.fsum([0.25, 2.0, 2.0, 0.0, 1.0]) and d.sum_scale == math.fsum([1.25, 4.0, 4.0, 1e-9, 4.0])
    assert ens.difference_of(ma, qa, 4, mb, qb, 3, 1.0, 0.0).n_selected == 3


def test_swapping_the_sides_changes_the_sign_of_sum_z_alone(pair):
    prob, L, a, b, _, whole = pair
    reqs = [ens.CompareRequest("psd", None, 0.0, 3.0), ens.CompareRequest("pxx_flux", None, 1e-3, 1.0), ens.CompareRequest("psd_mom", (3, 50), 1e-3, 2.0)]
    ab, ba = a.compare(b, 0, reqs), b.compare(a, 0, reqs)
    for q, x, y in zip(reqs, ab, ba):
        assert (x.n_a, x.n_b) == (y.n_b, y.n_a) == (N_A, N_B)
        assert_same_bits(as_dict(x), as_dict(y), repr(q), but_sign_of_sum_z=True)
    (ma, qa), (mb, qb) = slot_vectors(a, 0), slot_vectors(b, 0)
    back = restate(mb, qb, N_B, ma, qa, N_A, 0.0, 3.0)
    assert_same_bits(back, swapped(whole), "the restatement, swapped")


def test_agreement_values_and_refusals():
    A = ens.Agreement
    d = ens.Difference(amax=10.0, max_abs_z=4.5, sum_z=-6.0, sum_abs_z=9.0, sum_z2=24.0, sum_abs_diff=3.0, sum_scale=60.0, n_selected=10, n_over=2,
                       n_nonfinite=0, n_degenerate=2, argmax=4, n_a=5, n_b=4)
    r = {k: getattr(d, k) for k in ("max_abs_z", "sum_z", "sum_z2", "sum_abs_diff", "sum_scale", "n_selected", "n_over", "n_degenerate")}
    cases = (("max_z", 4.5), ("chi2_per_word", 24.0 / 8), ("fraction_over", 2 / 8), ("mean_z", -6.0 / 8), ("weighted_diff", 3.0 / 60.0))
    clean = dataclasses.replace(d, n_degenerate=0, n_selected=8)
    for stat, want in cases:
        t = A(0, "psd_mom", stat, abs(want), zcut=2.5)
        assert same_bits(t.value(d), want) and same_bits(t.value(d), value_of(stat, r)), stat
        # a degenerate word: only weighted_diff is met
        assert t.met(d) == (stat == "weighted_diff"), stat
        if stat != "weighted_diff":
            assert same_bits(t.value(clean), want) and t.met(clean) and not A(0, "psd_mom", stat, abs(want) / 2).met(clean), stat
        assert not A(0, "psd_mom", stat, abs(want) / 2).met(d)
        assert t.request == ens.CompareRequest("psd_mom", None, 1e-3, 2.5) and t.slot == t.other_slot == 0
        for kw in (dict(n_selected=0, n_degenerate=0), dict(n_nonfinite=1)):
            assert not t.met(dataclasses.replace(clean, **kw)), (stat, kw)
        assert math.isnan(t.value(dataclasses.replace(clean, n_selected=0)))
    # every selected word degenerate: only weighted_diff has a value
    alld = dataclasses.replace(d, n_degenerate=10)
    assert math.isnan(A(0, "psd", "max_z", 1.0).value(alld)) and A(0, "psd", "weighted_diff", 1.0).met(alld)
    t = A(0, "dNdp_pf", "chi2_per_word", 2.0, zones=(3, 4), bins=(5, 50), floor_frac=0.0, other_slot=1)
    assert t.request == ens.CompareRequest("dNdp_pf", (3, 4), 0.0, 3.0, (5, 50)) and (t.slot, t.other_slot) == (0, 1)
    for args, kw in ((("psd", "median", 0.1), {}), (("psd", "max_z", 0.0), {}), (("psd", "max_z", -1.0), {}), (("psd", "max_z", float("nan")), {}),
                     (("esc_psd_up", "max_z", 0.1), dict(zones=(0, 2))), (("no_such_part", "max_z", 0.1), {}),
                     (("psd", "max_z", 0.1), dict(floor_frac=1.5)), (("psd", "max_z", 0.1), dict(floor_frac=float("nan"))),
                     (("psd", "max_z", 0.1), dict(zcut=-1.0)), (("psd", "max_z", 0.1), dict(zcut=float("nan"))),
                     (("psd", "max_z", 0.1), dict(bins=(1, 2))), (("psd_mom", "max_z", 0.1), dict(zones=(0, 2), bins=(1, 2))),
                     (("psd", "max_z", 0.1), dict(other_slot=-1))):
        with pytest.raises(ValueError):
            A(0, *args, **kw)
    with pytest.raises(ValueError):
        A(-1, "psd", "max_z", 0.1)
    for kw in (dict(floor_frac=-0.1), dict(zcut=float("nan")), dict(zones=(0, 1), bins=(0, 1))):
        with pytest.raises(ValueError):
            ens.CompareRequest("psd", **kw)


def test_check_agreements_and_the_refusals_of_compare(pair):
    prob, L, a, b, _, whole = pair
    A = ens.Agreement
    rules = [A(0, "psd", "chi2_per_word", 3.0, zones=UNSHIFTED_ZONES, floor_frac=0.0), A(1, "spectra_sf", "max_z", 1e9),
             A(0, "psd", "chi2_per_word", 3.0, zones=SHIFTED_ZONES, floor_frac=0.0), A(0, "pxx_flux", "weighted_diff", 1.0)]
    rows = ens.check_agreements(a, b, rules)
    assert [row.agreement for row in rows] == rules
    for row in rows:
        t = row.agreement
        first, count = a.word_range(t.slot, t.name, t.zones, t.bins)
        (ma, qa), (mb, qb) = slot_vectors(a, t.slot), slot_vectors(b, t.other_slot)
        s_ = slice(first, first + count)
        want = restate(ma[s_], qa[s_], N_A, mb[s_], qb[s_], N_B, t.floor_frac, t.zcut)
        assert_exact(as_dict(row.difference), want, repr(t))
        assert_sums(as_dict(row.difference), want, repr(t))
        assert same_bits(row.value, t.value(row.difference)) and row.met == t.met(row.difference)
    # the crafted pair has degenerate words all over psd: a chi-square rule over them is not met whatever its value; the shifted
    # block's chi-square per word is the larger one
    assert rows[2].value > rows[0].value and not rows[0].met and rows[0].difference.n_degenerate > 0 and rows[3].met
    fresh, two = ens.HostEnsemble(prob.params, 1), ens.HostEnsemble(prob.params, 2)
    other = ens.HostEnsemble(make_problem(64, num_psd_bins_per_decade=(8, 10)).params, 1)         # another layout
    q = [ens.CompareRequest("pxx_flux")]
    before = [slot_vectors(e, s) for e in (a, b) for s in (0, 1)]
    with pytest.raises(ValueError, match="two samples"):
        a.compare(fresh, 0, q)
    with pytest.raises(ValueError, match="two samples"):
        fresh.compare(a, 0, q)
    with pytest.raises(ValueError, match="itself"):
        a.compare(a, 0, q)
    with pytest.raises(ValueError, match="species slot with a iteration slot|iteration slot with a species slot"):
        a.compare(b, 0, q, other_slot=1)
    with pytest.raises(ValueError, match="outside"):
        a.compare(b, 0, q, other_slot=2)
    with pytest.raises(ValueError, match="two samples"):
        a.compare(b, a.products_slot(0), [ens.CompareRequest("dNdp_pf")])      # never sampled
    with pytest.raises(KeyError):
        a.compare(b, 1, q)
    with pytest.raises(ValueError, match="at most"):
        a.compare(b, 0, q * 257)
    with pytest.raises(ValueError, match="zones"):
        a.compare(b, 0, [ens.CompareRequest("pxx_flux", (0, prob.params.n_grid + 1))])
    with pytest.raises(ValueError, match="same kind and layout"):
        a.compare(object(), 0, q)
    with pytest.raises(ValueError, match="same kind and layout"):
        a.compare(other, 0, q)
    assert a.compare(b, 0, []) == []
    for v, (e, s) in zip(before, [(e, s) for e in (a, b) for s in (0, 1)]):
        mean, m2 = slot_vectors(e, s)
        assert bits_equal(mean, v[0]) and bits_equal(m2, v[1])
    # two slots of one ensemble are two ensembles
    be = _Buffers(prob)
    bufs_a, bufs_b = crafted_pair(L)
    feed(be, two, bufs_a, L, 0, iteration=False)
    feed(be, two, bufs_b, L, 1, iteration=False)
    reqs = [ens.CompareRequest("psd", None, 0.0, 3.0), ens.CompareRequest("energy_flux", None, 1e-3, 1.0)]
    for x, y in zip(two.compare(two, 0, reqs, other_slot=1), a.compare(b, 0, reqs)):
        assert x == y


def test_symbol_is_exported_and_refuses_without_an_accumulator():
    lib = mcs.capi.load_library()
    assert hasattr(lib, "mcs_ens_compare") and "mcs_ens_compare" in mcs.capi.EXPORTED_SYMBOLS
    assert ct.sizeof(mcs.capi.McsEnsCmpRange) == 32 and ct.sizeof(mcs.capi.McsEnsDifference) == 96
    r, out = mcs.capi.McsEnsCmpRange(0, 1, 0.0, 3.0), mcs.capi.McsEnsDifference()
    assert lib.mcs_ens_compare(None, 0, None, 0, 1, ct.byref(r), ct.byref(out)) != 0
    assert b"mcs_ens_compare" in lib.mcs_last_error() and b"null argument" in lib.mcs_last_error()
