"""mcs_ens_summarize_merged (csrc/mcs_ensemble.hip) and what is built on it -- ensemble.HipEnsemble.summarize_merged,
driver.run_overlapped(triggers=...) -- on the crafted buffers and the range lists of test_gpu_ens_summary.py: six samples on the stock
binning, split over several accumulators of one home context as an overlapped run would feed them.  Three references: the
plain-numpy restatement of ens_summary_common.py on a numpy fold of the vectors read back, mcs_ens_merge into a fresh accumulator
followed by mcs_ens_summarize (bit for bit, the sums included), and a second call."""
import ctypes as ct

import numpy as np
import pytest

from conftest import mcs, make_problem, hip_backend
from ensemble_common import AS_IS, INCREMENTS, assert_tail_is_exercised, bits_equal, crafted_buffers
from ens_summary_common import FIELDS, as_dict, assert_exact, assert_sums, iteration_offsets, restate, same_bits, slot_vectors, species_offsets
from test_gpu_ens_summary import raw_summarize, species_ranges

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
N = 6
SPLITS = ((2, 2, 2), (3, 3), (1, 1), (0, 3, 0, 3), (6,))
TALLY_RTOL = 1e-11          # of each array's maximum: two GPU runs differ by the order of their atomic adds (test_gpu_parity.py)


def raw_merged(parts, slot, ranges):
    """One mcs_ens_summarize_merged call over the accumulators `parts` -> ([dict of FIELDS], n_total)."""
    lib = parts[0].lib
    hs = (ct.c_void_p * len(parts))(*[e.h.value for e in parts])
    rs = (mcs.capi.McsEnsRange * len(ranges))(*[mcs.capi.McsEnsRange(*r) for r in ranges])
    out = (mcs.capi.McsEnsSummary * len(ranges))()
    n = ct.c_int64(-1)
    rc = lib.mcs_ens_summarize_merged(len(parts), hs, slot, len(ranges), rs, out, ct.byref(n))
    assert rc == 0, lib.mcs_last_error().decode()
    return [{k: getattr(o, k) for k in FIELDS} for o in out], int(n.value)


def feed_split(hb, L, bufs, counts):
    """len(counts) accumulators on the home context hb; the buffers go round-robin to those that take samples, as the iterations
    of an overlapped run go to its contexts, until each has its count.  Every buffer is a species sample of slot 0 and an
    iteration sample (every section changes between snapshot and sample)."""
    parts = [ens.HipEnsemble(hb, 1) for _ in counts]
    left, k, a = list(counts), 0, 0
    prev = np.zeros(L.total)
    while sum(left):
        if left[a]:
            f, i = bufs[k]
            hb.write_tallies(prev, i)
            parts[a].begin_iteration(hb)
            hb.write_tallies(f, i)
            parts[a].add_species(hb, 0)
            parts[a].add_iteration(hb)
            left[a] -= 1
            prev, k = f, k + 1
        a = (a + 1) % len(counts)
    assert [e.count(0) for e in parts] == list(counts) == [e.count(1) for e in parts]
    return parts


def numpy_fold(parts, slot):
    """(mean, M2, n) of the left fold of the merge formula over the accumulators that have samples, from the vectors read back."""
    m = q = None
    na = 0
    for e in parts:
        nb = e.count(slot)
        if nb == 0:
            continue
        mb, qb = slot_vectors(e, slot)
        if na == 0:
            m, q = mb, qb
        else:
            n = float(na + nb)
            f_mean, f_m2 = float(nb) / n, float(na) * float(nb) / n
            with np.errstate(over="ignore", invalid="ignore"):
                d = mb - m
                m = m + d * f_mean
                q = (q + qb) + (d * d) * f_m2
        na += nb
    return m, q, na


def assert_same_bits(a, b, what):
    for k in FIELDS:
        assert same_bits(a[k], b[k]) if isinstance(b[k], float) else a[k] == b[k], (what, k, a[k], b[k])


@pytest.fixture(scope="module")
def crafted():
    prob = make_problem(64)
    L = mcs.capi.Layout(prob.params)
    assert_tail_is_exercised(ens.EnsLayout(prob.params).fields)
    bufs = crafted_buffers(L, N)
    hb = hip_backend(prob)
    sp_off, sp_total = species_offsets(L)
    it_off, it_total = iteration_offsets(L, INCREMENTS + AS_IS)
    ranges = {0: species_ranges(L, sp_off, sp_total)[0]}
    ranges[1] = [(0, it_total, ff, 0.1) for ff in (0.0, 1e-3, 1.0)]
    for name, (first, shape) in it_off.items():
        ranges[1] += [(first, int(np.prod(shape)), 1e-3, 0.05), (first, int(np.prod(shape)), 1.0, 0.05)]
    ranges[1] += [(1, it_total - 2, 1e-3, 0.3), (it_total - 1, 1, 0.0, 0.0)]
    yield dict(prob=prob, L=L, bufs=bufs, hb=hb, sp_off=sp_off, it_off=it_off, ranges=ranges, totals={0: sp_total, 1: it_total})
    hb.destroy()


def check_split(c, bufs, counts):
    hb, L, n_total = c["hb"], c["L"], sum(counts)
    parts = feed_split(hb, L, bufs, counts)
    before = [(e.mean(0, "therm_sf"), e.m2(0, "therm_sf"), e.mean(1, "spectra_sf"), e.m2(1, "spectra_sf")) for e in parts]
    into = ens.HipEnsemble(hb, 1)
    for e in parts:
        into.merge(e)
    worst = 0.0
    for slot in (0, 1):
        ranges = c["ranges"][slot]
        got, n = raw_merged(parts, slot, ranges)
        assert n == n_total and into.count(slot) == n_total
        mean, m2, n_fold = numpy_fold(parts, slot)
        assert n_fold == n_total and mean.size == c["totals"][slot]
        via_merge = raw_summarize(into, slot, ranges)
        again, _ = raw_merged(parts, slot, ranges)
        for r, g, v, a in zip(ranges, got, via_merge, again):
            want = restate(mean[r[0]:r[0] + r[1]], m2[r[0]:r[0] + r[1]], n_total, r[2], r[3])
            what = f"{counts} slot {slot} range {r}"
            assert_exact(g, want, what)
            assert_sums(g, want, what)
            # (the iteration slot's increments telescope: a mean of 1e-22 beside samples of 1e39 may round to zero, nothing selected)
            assert slot == 1 or r[1] == 0 or want["n_selected"] >= 1, what
            assert_same_bits(g, v, what + ": mcs_ens_merge + mcs_ens_summarize")
            assert_same_bits(a, g, what + ": a second call")
            for k in ("sum_se", "sum_abs_mean", "sum_rel2"):
                if want[k] > 0:
                    worst = max(worst, abs(g[k] - want[k]) / want[k] / 2.0 ** -53)
        if len(counts) == 1:
            for r, g, s in zip(ranges, got, raw_summarize(parts[0], slot, ranges)):
                assert_same_bits(g, s, f"one accumulator, slot {slot} range {r}: mcs_ens_summarize")
    print(f"{counts}: sums against fsum: worst difference {worst:.2f} units of 2^-53 relative (the bound is n_selected of them)")
    # the Python call maps names and zones to these ranges, and says the total count
    reqs = [ens.Request(name, None, 1e-3, 0.05) for name in ("psd", "pxx_flux", "therm_pf_tht")] + [ens.Request("psd", (10, 37), 1e-3, 0.1)]
    ranges0 = [parts[0].word_range(0, q.name, q.zones) + (q.floor_frac, q.tol) for q in reqs]
    raw0, _ = raw_merged(parts, 0, ranges0)
    for q, s, g in zip(reqs, parts[0].summarize_merged(parts[1:], 0, reqs), raw0):
        assert as_dict(s) == g and s.n == n_total, q
    # no accumulator was changed
    for e, cnt, b in zip(parts, counts, before):
        assert e.count(0) == cnt and e.count(1) == cnt
        now = (e.mean(0, "therm_sf"), e.m2(0, "therm_sf"), e.mean(1, "spectra_sf"), e.m2(1, "spectra_sf"))
        for x, y in zip(now, b):
            assert bits_equal(x, y)
    for e in parts + [into]:
        e.destroy()


@pytest.mark.parametrize("counts", SPLITS, ids=lambda c: "-".join(map(str, c)))
def test_merged_summary_against_three_references(crafted, counts):
    check_split(crafted, crafted["bufs"], counts)


def test_the_widest_list(crafted):
    """MCS_ENS_MAX_MERGED accumulators of one sample each: the fold of eight and the largest by-value kernel argument (the splits above
    fold at most three).  The six crafted buffers and, for the last two accumulators, halves of the first two (exact, and no sample
    twice)."""
    bufs = crafted["bufs"] + [(0.5 * f, i) for f, i in crafted["bufs"][:2]]
    check_split(crafted, bufs, (1,) * 8)


def test_a_merge_that_is_not_finite_is_counted(crafted):
    """One word, 1e160 in the samples of one accumulator and -1e160 in those of the other: finite in both, (d * d) of the merge is
    not.  With counts (2, 1) its merged mean, 3.3e159, is finite and the largest of the part: the first pass selected with it, the
    repeated second sweep selects with the amax of the finite words."""
    c = crafted
    hb, L = c["hb"], c["L"]
    first, shape = c["sp_off"]["pxx_flux"]
    w = 40
    bufs = [(f.copy(), i) for f, i in c["bufs"][:3]]
    for k, (f, _) in enumerate(bufs):
        f[L.offsets["pxx_flux"] + w] = -1e160 if k == 1 else 1e160
    parts = feed_split(hb, L, bufs, (2, 1))
    for e in parts:
        assert np.isfinite(e.mean(0, "pxx_flux")[w]) and np.isfinite(e.m2(0, "pxx_flux")[w])
    mean, m2, n = numpy_fold(parts, 0)
    assert n == 3 and np.isfinite(mean[first + w]) and np.isinf(m2[first + w]) and abs(mean[first + w]) == np.abs(mean).max()
    ranges = [(first, shape[0], 1e-3, 0.05), (first, shape[0], 0.0, 0.05), (first + w, 1, 0.0, 0.0), (first + w - 1, 3, 1.0, 0.0),
              (0, mean.size, 1e-3, 0.05)]
    got, n_total = raw_merged(parts, 0, ranges)
    into = ens.HipEnsemble(hb, 1)
    for e in parts:
        into.merge(e)
    for r, g, v in zip(ranges, got, raw_summarize(into, 0, ranges)):
        want = restate(mean[r[0]:r[0] + r[1]], m2[r[0]:r[0] + r[1]], 3, r[2], r[3])
        assert_exact(g, want, f"range {r}")
        assert_sums(g, want, f"range {r}")
        assert_same_bits(g, v, f"range {r}")
    assert n_total == 3 and got[0]["n_nonfinite"] == 1 and got[0]["n_selected"] >= 1 and got[0]["amax"] < 1e42
    assert got[2]["n_nonfinite"] == 1 and got[2]["n_selected"] == 0 and got[2]["argmax"] == -1 and got[4]["n_nonfinite"] == 1
    t = ens.Trigger(0, "pxx_flux", "max", 1e9)
    s = parts[0].summarize_merged(parts[1:], 0, [t.request])[0]
    assert s.n_nonfinite == 1 and not t.met(s)
    for e in parts + [into]:
        e.destroy()


def test_refusals_change_nothing(crafted):
    c = crafted
    hb, L = c["hb"], c["L"]
    a, b = feed_split(hb, L, c["bufs"], (2, 1))
    lone = feed_split(hb, L, c["bufs"], (1,))[0]
    empty, wide = ens.HipEnsemble(hb, 1), ens.HipEnsemble(hb, 2)
    lib, R, S = a.lib, mcs.capi.McsEnsRange, mcs.capi.McsEnsSummary
    total = c["totals"][0]
    out, n = (S * 2)(), ct.c_int64(-7)
    vec = [slot_vectors(e, 0) for e in (a, b)]

    def call(parts, slot=0, first=0, count=1, n_ranges=1, ff=1e-3, tol=0.0):
        hs = (ct.c_void_p * len(parts))(*[e.h.value for e in parts])
        return lib.mcs_ens_summarize_merged(len(parts), hs, slot, n_ranges, (R * 1)(R(first, count, ff, tol)), out, ct.byref(n))
    refused = [
        ("a duplicate", lambda: call([a, b, a])),
        ("a duplicate", lambda: call([a, a])),
        ("a total count of 1", lambda: call([lone, empty])),
        ("a total count of 0", lambda: call([empty])),
        ("a slot out of range", lambda: call([a, b], slot=2)),
        ("a slot out of range", lambda: call([a, b], slot=-1)),
        ("a range outside the vector", lambda: call([a, b], first=total - 1, count=2)),
        ("a range outside the vector", lambda: call([a, b], first=-1, count=2)),
        ("a range outside the vector", lambda: call([a, b], slot=1, count=c["totals"][1] + 1)),
        ("other slots", lambda: call([a, wide])),
        ("floor_frac", lambda: call([a, b], ff=1.5)),
        ("tol", lambda: call([a, b], tol=float("nan"))),
        ("n_ranges", lambda: call([a, b], n_ranges=257)),
    ]
    for what, f in refused:
        assert f() != 0, what
        assert b"mcs_ens_summarize_merged" in lib.mcs_last_error(), (what, lib.mcs_last_error())
        assert n.value == -7, what
    with pytest.raises(RuntimeError, match="mcs_ens_summarize_merged"):
        a.summarize_merged([b, a], 0, [ens.Request("pxx_flux")])
    with pytest.raises(ValueError, match="merged summary"):
        a.summarize_merged([ens.HostEnsemble(c["prob"].params, 1)], 0, [ens.Request("pxx_flux")])
    # nothing to do: the count is still said
    hs = (ct.c_void_p * 2)(a.h.value, b.h.value)
    assert lib.mcs_ens_summarize_merged(2, hs, 0, 0, None, None, ct.byref(n)) == 0 and n.value == 3
    assert [e.count(0) for e in (a, b, lone, empty, wide)] == [2, 1, 1, 0, 0] and [e.count(1) for e in (a, b, lone, empty)] == [2, 1, 1, 0]
    for e, (m0, q0) in zip((a, b), vec):
        m1, q1 = slot_vectors(e, 0)
        assert bits_equal(m0, m1) and bits_equal(q0, q1)
    # the accumulators go on working: empty ones are skipped wherever they stand in the list
    r = [(c["sp_off"]["pxx_flux"][0], L.n_grid, 1e-3, 0.0)]
    assert raw_merged([empty, a, b], 0, r) == raw_merged([a, b], 0, r) == raw_merged([a, empty, b], 0, r)
    assert a.summarize_merged([], 0, [ens.Request("pxx_flux")]) == a.summarize(0, [ens.Request("pxx_flux")])
    for e in (a, b, lone, empty, wide):
        e.destroy()


N_ITRS, N_PCUTS = 6, 6          # (the driver run of test_gpu_ensemble.py: 2000 protons, its N_PCUTS; a cap of six iterations)


def _overlapped(prob, K, **kw):
    """-> (result, species and iteration slot vectors, counts); the ensemble is destroyed before its home context."""
    bes = [hip_backend(prob) for _ in range(K)]
    res = mcs.driver.run_overlapped(prob, bes, max_pcuts=N_PCUTS, ensemble=True, **kw)
    e = res.ensemble
    vec = [slot_vectors(e, slot) for slot in (0, 1)]
    n = [e.count(0), e.count(1)]
    e.destroy()
    for be in bes:
        be.destroy()
    return res, vec, n


@pytest.mark.parametrize("K", (2, 3))
def test_overlapped_run_stops_at_the_predicted_round(K):
    """The threshold comes from a first run whose trigger cannot be met: the value at the earliest round end, from the second on,
    that lies below every earlier one by more than (1 + 1e-6)^2, times (1 + 1e-6).  Two GPU runs differ by the order of their tallies'
    atomic adds, at most TALLY_RTOL = 1e-11 of an array's maximum, hence at most 1e-8 relative in a word selected with
    floor_frac = 1e-3 and about as much in the value: the margin of 1e-6 is far above it."""
    prob = make_problem(2000, num_iterations=N_ITRS)
    L = mcs.capi.Layout(prob.params)
    rounds = list(range(K, N_ITRS + 1, K))
    first, _, _ = _overlapped(prob, K, n_itrs=N_ITRS, triggers=[ens.Trigger(0, "therm_sf_mom", "rms", 1e-12)])
    c1 = first.convergence
    assert [it for it, _ in c1.checks] == rounds and c1.stopped_at == N_ITRS and not c1.satisfied
    v = {it: rows[0].value for it, rows in c1.checks}
    print(f"K = {K}: rms relative error of therm_sf_mom by round end:", v)
    stop = next((rounds[k] for k in range(1, len(rounds)) if all(v[rounds[k]] < v[r] / (1.0 + 1e-6) ** 2 for r in rounds[:k])), None)
    assert stop is not None, v
    trig = ens.Trigger(0, "therm_sf_mom", "rms", v[stop] * (1.0 + 1e-6))
    seen = []
    res, vec, n = _overlapped(prob, K, n_itrs=N_ITRS, triggers=[trig], on_iteration_end=seen.append)
    c = res.convergence
    print("checks of the run with the trigger:", [(it, rows[0].value, rows[0].met) for it, rows in c.checks], "stopped at", c.stopped_at)
    assert c.stopped_at == stop and c.satisfied and [it for it, _ in c.checks] == [r for r in rounds if r <= stop]
    assert seen == list(range(1, stop + 1)) and n == [stop, stop] and len(res.iter_finals) == stop
    for (it, rows), (_, rows1) in zip(c.checks, c1.checks):
        assert rows[0].summary.n == it and rows[0].met == (it == stop)
        assert abs(rows[0].value - rows1[0].value) <= 1e-6 * rows1[0].value
    short, vec_s, n_s = _overlapped(prob, K, n_itrs=stop)
    assert short.convergence is None and n_s == n
    assert np.array_equal(res.tallies_i64, short.tallies_i64)
    for name in L.offsets:
        a, b = L.view(res.tallies_f64, name), L.view(short.tallies_f64, name)
        assert float(np.max(np.abs(a - b))) <= TALLY_RTOL * float(np.max(np.abs(b))), name
    e_lay = ens.EnsLayout(prob.params)
    for slot, table in ((0, e_lay.species), (1, e_lay.iteration)):
        mean, mean_s = vec[slot][0], vec_s[slot][0]
        for name, (off, shape) in table.items():
            cnt = int(np.prod(shape))
            a, b = mean[off:off + cnt], mean_s[off:off + cnt]
            assert float(np.max(np.abs(a - b))) <= TALLY_RTOL * float(np.max(np.abs(b))), (slot, name)
