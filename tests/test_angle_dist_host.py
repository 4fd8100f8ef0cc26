"""The pitch-angle distributions (K11, include/mcs.h mcs_angle_dist) without a GPU: the restatement of tests/angles_common.py against
an independent numpy form and at rest, the angles slot of the numpy ensemble with every refusal and the window rules of merge,
merged summary and comparison, consumers.momentum_windows, the refusals of the driver, and the header and ctypes table."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import angles_common as ac
import consumers_common as cc
from conftest import ROOT, mcs, make_problem, oracle_backend
from ensemble_common import same_words, stat_of

ens = mcs.ensemble


# ---- (a) the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binning", ["small", "stock", "large"])
def test_rest_frame_image_is_the_cell_itself(binning):
    """At gamma = 1 (beta = 0 by the rule) the image of every cell is the cell itself, with the library's log10 and acos: frame 1 of
    a zone at rest then equals frame 0."""
    kw = {"small": cc.SMALL_BINNING, "stock": {}, "large": cc.LARGE_BINNING}[binning]
    prob = make_problem(64, **kw)
    P = prob.params
    nm, nt = P.num_psd_mom_bins, P.num_psd_tht_bins
    assert (nm, nt) == {"small": (32, 9), "stock": (155, 159), "large": (199, 199)}[binning]
    t = mcs.consumers.consumer_tables(prob, 1)
    jb, kb = ac.image(P, t, 1.0)
    J, K = np.meshgrid(np.arange(nt + 1), np.arange(nm + 1), indexing="ij")
    misses = int(((jb != J) | (kb != K)).sum())
    print(f"{binning}: {misses} misses of {(nm + 1) * (nt + 1)} cells")
    assert misses == 0
    # and below the edge of the rule, where beta is 0 but gamma is not 1, the image is still made by the statements (no shortcut)
    jb2, kb2 = ac.image(P, t, cc.GAMMAS[1])
    assert jb2.shape == jb.shape and jb2.min() >= 0 and jb2.max() <= nt and kb2.min() >= 0 and kb2.max() <= nm


@pytest.mark.parametrize("binning", ["small", "large"])
def test_restatement_against_the_independent_form(binning):
    """Every A[j] of the restatement (serial adds in cell order) against the exactly rounded sum of the same addends grouped with
    numpy: within K_BOUND n_adds 2^-53 A[j]; all addends are positive."""
    prob = make_problem(64, **(cc.SMALL_BINNING if binning == "small" else cc.LARGE_BINNING))
    P = prob.params
    nm, nt = P.num_psd_mom_bins, P.num_psd_tht_bins
    zones = (3, 7, 10) if binning == "small" else (7,)
    f, i = cc.dense_tallies(prob, seed=3, lit_zones=zones, fill=1.0 if binning == "small" else 0.25)
    cc.set_gammas(prob, cc.dense_gammas(P.n_grid))
    t = mcs.consumers.consumer_tables(prob, 1)
    windows = ((0, nm + 1), (5, 6), (nm // 3, nm // 2), (nm // 2, nm))
    ref = ac.reference(prob, t, f, i, windows)
    checked = 0
    for z in zones:
        for fr in range(3):
            A, n_adds = ac.numpy_form(prob, t, f, i, windows, fr, z - 1)
            got = ref.A[fr, z - 1]
            bound = cc.K_BOUND * n_adds * ac.U * A
            assert np.all(np.abs(got - A) <= bound), (z, fr, float(np.max(np.abs(got - A) / np.maximum(bound, 1e-300))))
            assert np.array_equal(got > 0, n_adds > 0)
            checked += int((n_adds > 0).sum())
    assert checked > 3 * len(zones) * (nt // 2)
    # zones without a lit cell: the empty rule
    dark = [z for z in range(P.n_grid) if z + 1 not in zones]
    assert np.all(ref.number[:, dark] == 0.0) and np.all(ref.dist[:, dark] == 1.0e-99) and np.all(np.isnan(ref.moments[:, dark]))
    lit = [z - 1 for z in zones]
    assert np.all(ref.number[:, lit, 0] > 0) and np.all(np.isfinite(ref.moments[:, lit, 0]))
    assert np.all(np.abs(ref.moments[:, lit, 0, 0]) <= 1) and np.all(ref.moments[:, lit, 0, 1] <= 1)


def test_weights_follow_the_header():
    """The weight of a cell: thermal crossings only with therm_from_hist and crossings, psd only above 1e-66, NaN never lit."""
    nm, nt = 3, 2
    psd = np.zeros((nt + 2, nm + 2)); ths = np.zeros((nt + 2, nm + 2))
    psd[0, 0] = cc.T66; psd[0, 1] = np.nextafter(cc.T66, 1.0); psd[1, 1] = np.nan; psd[1, 2] = 2.0
    ths[0, 0] = 3.0; ths[1, 2] = 0.5; ths[2, 3] = np.nan
    v = ac.weights(psd, ths, 0, True, nm, nt)
    assert v[0, 0] == 0.0 and v[0, 1] == psd[0, 1] and v[1, 1] == 0.0 and v[1, 2] == 2.0
    v = ac.weights(psd, ths, 4, True, nm, nt)
    assert v[0, 0] == 3.0 and v[1, 2] == 2.5 and np.isnan(v[2, 3])
    A, n_lit = ac.row_sums(v, *np.meshgrid(np.arange(nt + 1), np.arange(nm + 1), indexing="ij"), ((0, nm + 1),), nt)
    assert n_lit == 3 and A[0] == [3.0 + psd[0, 1], 2.5, 0.0]
    assert np.array_equal(ac.weights(psd, ths, 4, False, nm, nt), ac.weights(psd, ths, 0, True, nm, nt), equal_nan=True)


# ---- (b) momentum_windows -----------------------------------------------------------------------------------------------------------------
def test_momentum_windows():
    prob = cc.small_problem()
    nm = prob.params.num_psd_mom_bins
    x = 10.0 ** ens.bin_centres_log10(prob)
    w = mcs.consumers.momentum_windows(prob, [(x[0] * 0.5, x[-1] * 2), (x[4], x[4]  * 1.0001), (x[4] * 1.0001, x[9])])
    assert w == ((0, nm + 1), (4, 5), (5, 10))
    l_lo, l_hi, _ = ens.slope_window(prob, x[3], x[12])
    assert mcs.consumers.momentum_windows(prob, [(x[3], x[12])]) == ((l_lo, l_hi),)
    with pytest.raises(ValueError, match="no momentum bin"):
        mcs.consumers.momentum_windows(prob, [(x[4] * 1.001, x[5] * 0.999)])
    with pytest.raises(ValueError, match="1..8 windows"):
        mcs.consumers.momentum_windows(prob, [(x[0], x[5])] * 9)
    with pytest.raises(ValueError, match="1..8 windows"):
        mcs.consumers.momentum_windows(prob, [])
    with pytest.raises(ValueError, match="0 < p_lo < p_hi"):
        mcs.consumers.momentum_windows(prob, [(x[5], x[4])])


# ---- (c) the numpy ensemble ---------------------------------------------------------------------------------------------------------------
def crafted_distributions(prob, windows, k, rng, empty_row=None):
    P = prob.params
    ng, nt = P.n_grid, P.num_psd_tht_bins
    nw = len(windows)
    dist = 10.0 ** rng.uniform(-3, 3, (3, ng, nw, nt + 2)); dist[..., nt + 1] = 1.0e-99
    number = rng.uniform(1, 2, (3, ng, nw)) * 10.0 ** k
    mu = rng.uniform(-1, 1, (3, ng, nw)); mu2 = rng.uniform(0, 1, (3, ng, nw))
    if empty_row is not None:
        fr, z, m = empty_row
        dist[fr, z, m] = 1.0e-99; number[fr, z, m] = 0.0; mu[fr, z, m] = np.nan; mu2[fr, z, m] = np.nan
    return mcs.consumers.AngleDistributions(dist, number, mu, mu2, tuple(windows), np.zeros(nt + 2), np.zeros(nt + 1))


def test_slot_numbers_and_layout():
    prob = make_problem(64)
    P = prob.params
    ng, nt, nm = P.n_grid, P.num_psd_tht_bins, P.num_psd_mom_bins
    e = ens.HostEnsemble(P, 3)
    for s in range(3):
        slot = e.angles_slot(s)
        assert slot == s | (1 << 26) and e.is_angles(slot)
        assert not (e.is_products(slot) or e.is_photons(slot) or e.is_photons_all(slot) or e.is_escape(slot))
        assert e.count(slot) == 0 and e.names(slot) == ("dist", "number", "mean_mu", "mean_mu2")
        assert not any(e.is_angles(x) for x in (s, e.products_slot(s), e.photons_slot(s), e.escape_slot(s)))
    assert not e.is_angles(e.photons_all_slot) and not e.is_angles(e.iteration_slot) and not e.is_angles(-1)
    for bad in (-1, 3):
        with pytest.raises(ValueError, match="angles slot"):
            e.angles_slot(bad)
    with pytest.raises(ValueError, match="no species slot"):
        e.count(5 | (1 << 26))
    s = e.angles_slot(1)
    with pytest.raises(ValueError, match="no angle windows"):
        e.angles_row(0, 0, 0)
    with pytest.raises(ValueError, match="no windows yet"):
        e.word_range(s, "dist")
    e.set_angle_windows([0, 4], [nm + 1, 9])
    e.set_angle_windows([0, 4, 9], [nm + 1, 9, 12])                 # (may be repeated until the first sample)
    rows, NT = 3 * ng * 3, nt + 2
    assert e.angles_row(0, 0, 0) == (0, 1) and e.angles_row(2, ng - 1, 2) == (rows - 1, rows) and e.angles_row(1, 4, 1) == ((ng + 4) * 3 + 1, (ng + 4) * 3 + 2)
    for bad in ((3, 0, 0), (0, ng, 0), (0, 0, 3), (0, -1, 0)):
        with pytest.raises(ValueError, match="frames 0, 1, 2"):
            e.angles_row(*bad)
    r = e.angles_row(1, 4, 1)
    assert e.word_range(s, "dist", r, (3, 9)) == (r[0] * NT + 3, 6) and e.word_range(s, "dist") == (0, rows * NT)
    assert e.word_range(s, "number", r) == (rows * NT + r[0], 1)
    assert e.word_range(s, "mean_mu", r) == (rows * NT + rows + r[0], 1) and e.word_range(s, "mean_mu2") == (rows * NT + 2 * rows, rows)
    with pytest.raises(KeyError, match="dNdp"):
        e.word_range(s, "dNdp")
    with pytest.raises(ValueError, match="never taken a sample"):
        e.mean(s, "number")
    # the layout mirror against the library, which needs no GPU for it
    lib = mcs.capi.load_library()
    for n_win in (1, 3, 8):
        out = mcs.capi.McsEnsAnglesLayout()
        assert lib.mcs_ens_angles_get_layout(ct.byref(P), n_win, ct.byref(out)) == 0
        assert {name: getattr(out, name) for name, _ in out._fields_} == e.layout.angles_fields(n_win)
    for n_win in (0, 9):
        assert lib.mcs_ens_angles_get_layout(ct.byref(P), n_win, ct.byref(out)) != 0 and b"n_win" in lib.mcs_last_error()


def test_window_rules():
    prob = cc.small_problem()
    nm = prob.params.num_psd_mom_bins
    e = ens.HostEnsemble(prob.params, 1)
    for lo, hi in (([], []), ([0] * 9, [1] * 9), ([0, 1], [2]), ([-1], [3]), ([3], [3]), ([4], [3]), ([0], [nm + 2]), ([0.5], [3])):
        with pytest.raises(ValueError, match="angle window"):
            e.set_angle_windows(lo, hi)
    assert not e.has_angle_windows()
    e.set_angle_windows([0, 0, nm], [nm + 1, 1, nm + 1])            # the largest, the first and the last bin; they overlap
    assert e.has_angle_windows() and e.angle_windows == ((0, 0, nm), (nm + 1, 1, nm + 1))


def test_host_ensemble_takes_angles_samples():
    prob = cc.small_problem()
    P = prob.params
    ng, nt, nm = P.n_grid, P.num_psd_tht_bins, P.num_psd_mom_bins
    windows = ((0, nm + 1), (4, 9))
    be = oracle_backend(prob)
    rng = np.random.default_rng(4)
    samples = [crafted_distributions(prob, windows, k, rng, empty_row=(2, 5, 1) if k == 1 else None) for k in range(3)]
    e = ens.HostEnsemble(P, 2)
    with pytest.raises(ValueError, match="no angle windows"):
        e.add_angles(be, 0, samples[0])
    e.set_angle_windows([0, 4], [nm + 1, 10])
    with pytest.raises(ValueError, match="windows of the AngleDistributions differ"):
        e.add_angles(be, 0, samples[0])
    e.set_angle_windows([0, 4], [nm + 1, 9])
    with pytest.raises(ValueError, match="takes its angles sample from an AngleDistributions"):
        e.add_angles(be, 0, None)
    with pytest.raises(ValueError, match="no species slot"):
        e.add_angles(be, e.iteration_slot, samples[0])
    with pytest.raises(ValueError):
        e.add_angles(be, 2, samples[0])
    for s in samples:
        e.add_angles(be, 0, s)
    slot = e.angles_slot(0)
    assert e.count(slot) == 3 and e.count(0) == 0 and e.count(e.angles_slot(1)) == 0
    rows = 3 * ng * 2
    parts = lambda s: dict(dist=s.dist.reshape(rows, nt + 2), number=s.number.ravel(), mean_mu=s.mean_mu.ravel(), mean_mu2=s.mean_mu2.ravel())
    with np.errstate(invalid="ignore"):
        want = stat_of([parts(s) for s in samples])
        mean, err, n = ens.stats_over([np.concatenate([p.ravel() for p in parts(s).values()]) for s in samples])
    for name in ens.ANGLES_NAMES:
        assert same_words(e.mean(slot, name), want.mean[name]) and same_words(e.m2(slot, name), want.m2[name]), name
    assert n == 3 and same_words(e._read(slot, 0, 0, mean.size), mean) and same_words(e._read(slot, 2, 0, mean.size), err)
    with pytest.raises(ValueError, match="angle windows stay"):
        e.set_angle_windows([0, 4], [nm + 1, 9])
    # a Request and a Trigger on a row: a good one, and the row that was empty in one sample (NaN moments: never met)
    good, empty = e.angles_row(2, 4, 1), e.angles_row(2, 5, 1)
    got = e.summarize(slot, [ens.Request("mean_mu", good, 0.0), ens.Request("mean_mu", empty, 0.0), ens.Request("dist", good, 0.0, 0.0, (2, 7)),
                             ens.Request("number", empty, 0.0)])
    assert [s.n for s in got] == [3] * 4 and got[0].n_selected == 1 and got[0].n_nonfinite == 0 and got[1].n_nonfinite == 1
    assert got[2].n_selected == 5 and got[3].n_nonfinite == 0
    assert np.isnan(e.mean(slot, "mean_mu").ravel()[empty[0]]) and np.isfinite(e.mean(slot, "number").ravel()[empty[0]])
    t_good = ens.Trigger(slot, "mean_mu", "max", 1.0e6, zones=good, floor_frac=0.0)
    t_nan = ens.Trigger(slot, "mean_mu", "max", 1.0e6, zones=empty, floor_frac=0.0)
    e.check_trigger(t_good); e.check_trigger(t_nan)
    assert t_good.met(got[0]) and not t_nan.met(got[1])
    with pytest.raises(ValueError, match="outside"):
        e.check_trigger(ens.Trigger(slot, "dist", "max", 1.0, zones=good, bins=(0, nt + 3)))
    # load_mean takes species slots only
    with pytest.raises(ValueError):
        e.load_mean(slot, be)
    be.destroy()


def test_merge_summary_and_compare_hold_the_windows():
    prob = cc.small_problem()
    P = prob.params
    nm = P.num_psd_mom_bins
    windows = ((0, nm + 1), (4, 9))
    be = oracle_backend(prob)
    rng = np.random.default_rng(6)
    samples = [crafted_distributions(prob, windows, 0, rng) for _ in range(5)]

    def filled(which, lo=(0, 4), hi=(nm + 1, 9), slot=0):
        e = ens.HostEnsemble(P, 2)
        e.set_angle_windows(lo, hi)
        for k in which:
            e.add_angles(be, slot, samples[k])
        return e

    a, b = filled((0, 1, 2)), filled((3, 4))
    slot = a.angles_slot(0)
    req = [ens.Request("dist", a.angles_row(1, 3, 0), 0.0), ens.Request("mean_mu2", None, 0.0)]
    merged = a.summarize_merged([b], slot, req)
    whole = filled((0, 1, 2, 3, 4))
    assert [s.n for s in merged] == [5, 5]
    # a destination without windows takes the source's; one merge equals the merged summary
    dst = ens.HostEnsemble(P, 2)
    dst.merge(a)
    assert dst.angle_windows == a.angle_windows and dst.count(slot) == 3
    dst.merge(b)
    assert dst.count(slot) == 5
    for s, w in zip(merged, dst.summarize(slot, req)):
        assert s == w
    assert np.allclose(dst.mean(slot, "number"), whole.mean(slot, "number"), rtol=1e-14, atol=0)
    with pytest.raises(ValueError, match="angle windows stay"):
        dst.set_angle_windows([0], [3])
    # an ensemble that merely HAS other windows and no sample still differs
    other = ens.HostEnsemble(P, 2)
    other.set_angle_windows([0, 4], [nm + 1, 10])
    with pytest.raises(ValueError, match="angle windows differ"):
        a.merge(other)
    with pytest.raises(ValueError, match="angle windows differ"):
        a.summarize_merged([other], slot, req)
    # compare: two species' angles slots of one ensemble, and two ensembles; windows that differ are refused
    both = filled((0, 1, 2))
    for k in (3, 4):
        both.add_angles(be, 1, samples[k])
    creq = [ens.CompareRequest("dist", both.angles_row(0, 2, 1), 0.0), ens.CompareRequest("number", None, 0.0)]
    d = both.compare(both, both.angles_slot(0), creq, both.angles_slot(1))
    assert (d[0].n_a, d[0].n_b) == (3, 2) and d[0].n_selected == P.num_psd_tht_bins + 2 and d[1].n_selected == 3 * P.n_grid * 2
    d2 = a.compare(b, slot, creq)
    assert d2[0] == d[0] and d2[1] == d[1]
    agree = ens.check_agreements(a, b, [ens.Agreement(slot, "number", "max_z", 1.0e9, floor_frac=0.0)])
    assert agree[0].met
    c = ens.HostEnsemble(P, 2)
    c.set_angle_windows([0, 5], [nm + 1, 9])
    fake = [mcs.consumers.AngleDistributions(s.dist, s.number, s.mean_mu, s.mean_mu2, ((0, nm + 1), (5, 9)), s.cos_edge, s.cos_center) for s in samples[:2]]
    for s in fake:
        c.add_angles(be, 0, s)
    with pytest.raises(ValueError, match="angle windows differ"):
        a.compare(c, slot, creq)
    with pytest.raises(ValueError, match="comparison of a"):
        a.compare(b, slot, creq, b.escape_slot(0))
    be.destroy()


# ---- (d) the driver and the consumers entry -------------------------------------------------------------------------------------------------
def test_the_oracle_backend_has_no_angle_dist():
    prob = make_problem(64)
    be = oracle_backend(prob)
    x = 10.0 ** ens.bin_centres_log10(prob)
    with pytest.raises(ValueError, match="no angle_dist"):
        mcs.consumers.angle_distributions(prob, be, 1, ((0, 5),))
    with pytest.raises(ValueError, match="no angle_dist"):
        mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, finalize=True, angles=[(x[2], x[20])])
    be.destroy()


class Recorder:
    """A backend that records what consumers.angle_distributions hands to angle_dist."""
    def __init__(self, P):
        self.P, self.calls = P, []

    def angle_dist(self, tabs, l_lo, l_hi):
        self.calls.append((tabs, tuple(l_lo), tuple(l_hi)))
        ng, nt, nw = self.P.n_grid, self.P.num_psd_tht_bins, len(l_lo)
        mom = np.zeros((3, ng, nw, 2)); mom[..., 1] = 0.5
        return np.full((3, ng, nw, nt + 2), 1.0e-99), np.ones((3, ng, nw)), mom


def test_angle_distributions_entry():
    prob = cc.small_problem()
    P = prob.params
    be = Recorder(P)
    d = mcs.consumers.angle_distributions(prob, be, 1, [(0, 5), (3, 4)], therm_from_hist=False)
    tabs, lo, hi = be.calls[0]
    assert (lo, hi) == ((0, 3), (5, 4)) and tabs.therm_from_hist == 0 and d.windows == ((0, 5), (3, 4))
    assert d.dist.shape == (3, P.n_grid, 2, P.num_psd_tht_bins + 2) and d.number.shape == d.mean_mu.shape == d.mean_mu2.shape == (3, P.n_grid, 2)
    assert np.all(d.mean_mu == 0.0) and np.all(d.mean_mu2 == 0.5)
    assert cc.bits_equal(d.cos_edge, tabs.cos_edge) and cc.bits_equal(d.cos_center, tabs.cos_center)
    for bad in ([], [(0, 1)] * 9, [(3, 3)], [(0, P.num_psd_mom_bins + 2)]):
        with pytest.raises(ValueError):
            mcs.consumers.angle_distributions(prob, be, 1, bad)
    assert len(be.calls) == 1


def test_driver_refusals():
    prob = make_problem(64)
    be = oracle_backend(prob)
    e = ens.HostEnsemble(prob.params, 1)
    x = 10.0 ** ens.bin_centres_log10(prob)
    win = [(x[2], x[20])]
    with pytest.raises(ValueError, match="angles: needs finalize=True"):
        mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, angles=win)
    e.set_angle_windows([2], [21])
    trig = ens.Trigger(e.angles_slot(0), "mean_mu", "max", 0.1, zones=e.angles_row(0, 3, 0))
    with pytest.raises(ValueError, match="angles slot needs angles="):
        mcs.driver.run(prob, be, n_itrs=2, max_pcuts=1, finalize=True, ensemble=e, triggers=[trig])
    with pytest.raises(ValueError, match="leaves the pitch-angle distributions out"):
        mcs.driver.run_overlapped(prob, [be], n_itrs=1, max_pcuts=1, angles=win)
    with pytest.raises(ValueError, match="leaves the pitch-angle distributions out"):
        mcs.driver.run_overlapped(prob, [be], n_itrs=2, max_pcuts=1, ensemble=True, triggers=[trig])
    with pytest.raises(ValueError, match="1..8 windows"):
        mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, finalize=True, angles=win * 9)
    assert e.count(0) == 0 and e.count(e.angles_slot(0)) == 0
    res = mcs.driver.run(prob, be, n_itrs=1, max_pcuts=1, finalize=True)
    assert res.angles is None and dataclass_last_field(res) == "angles"
    be.destroy()


def dataclass_last_field(res):
    import dataclasses
    return dataclasses.fields(res)[-1].name


# ---- (e) header and ctypes ------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table():
    src = open(os.path.join(ROOT, "include", "mcs.h")).read()
    lib = mcs.capi.load_library()
    for name in ("mcs_angle_dist", "mcs_ens_angles_get_layout", "mcs_ens_set_angle_windows", "mcs_ens_add_angles"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(lib, name) and name in mcs.capi.EXPORTED_SYMBOLS, name
    assert re.search(r"#define\s+MCS_ANGLE_MAX_WINDOWS\s+8\b", src) and ens.ANGLE_MAX_WINDOWS == 8
    assert re.search(r"#define\s+MCS_ENS_ANGLES\(s\)\s+\(\(s\)\s*\|\s*\(1\s*<<\s*26\)\)", src)
    assert mcs.capi.ENS_ANGLES_BIT == 1 << 26 == ens.ANGLES_BIT
    m = re.search(r"typedef struct mcs_ens_angles_layout \{(.*?)\} mcs_ens_angles_layout;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [w.strip() for decl in re.findall(r"int64_t([^;]*);", body) for w in decl.split(",")]
    assert fields == [name for name, _ in mcs.capi.McsEnsAnglesLayout._fields_]
    # without a GPU the call itself is refused, as every call on a null context
    assert lib.mcs_angle_dist(None, None, 1, None, None, None, None, None) != 0 and b"null context" in lib.mcs_last_error()
