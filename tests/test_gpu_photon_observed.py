"""K9 on the device (csrc/mcs_consumers.hip: mcs_k_photon_observe_zone, mcs_k_photon_observe_shells, through
HipBackend.photon_observe) against consumers.shell_spectra_host and the serial restatement of include/mcs.h "observed shell spectra":
every word is required to have the host's bits."""
import math

import numpy as np
import pytest

from conftest import mcs, make_problem, hip_backend
from ensemble_common import crafted_buffers
from photon_observed_common import BETAS, bits_equal, crafted_emis, flux_classes, serial_restatement, tables

pytestmark = pytest.mark.gpu

cons = mcs.consumers


def same_words(a, b):
    """Bit-equal, where a NaN equals a NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


@pytest.fixture(scope="module")
def ctx():
    prob = make_problem(64)
    hb = hip_backend(prob)
    yield prob, hb
    hb.destroy()


def crafted_case(process, ng, n_photon):
    """Zones as photon_observed_common.crafted_emis lays them out, zones 13..15 dark; beta cycles through BETAS (5 values against 6
    kinds of zone: 30 zones meet every pair).  Shells: a boundary 0 (a dark row), zones 2..7, the one zone 8 (a line), zones 9..12,
    the dark zones 13..15, zones 16..ng-4; zone 1 and the last four lie outside every shell."""
    ends = [0, 2, 8, 9, 13, 16, ng - 3]
    tabs = tables(process, ng, n_photon, BETAS, ends)
    emis = crafted_emis(process, ng, n_photon, tabs)
    emis[12:15] = 0.0
    return emis, tabs


@pytest.mark.parametrize("n_photon", [24, 25])
@pytest.mark.parametrize("process", cons.PHOTON_PROCESSES)
def test_crafted_zones_have_the_host_bits(ctx, process, n_photon):
    prob, hb = ctx
    ng = prob.params.n_grid
    assert ng >= 36
    emis, tabs = crafted_case(process, ng, n_photon)
    floor, low, lit = flux_classes(process, emis, tabs)
    assert floor > 0 and low >= 5 and lit > 5 * n_photon
    want = cons.shell_spectra_host(process, emis, **tabs)
    got = hb.photon_observe(process, emis=emis, **tabs)
    n = n_photon - 1
    assert got.shape == want.shape == (7, n)
    print(f"{process}: {(want > 1e-99).sum()} lit words of {want.size}; {(got != want).sum()} differ")
    assert bits_equal(got, want)
    # the rows the layout says are dark are dark, the others are not; what was shifted beyond the grid is gone
    assert np.all(want[0] == 1e-99) and np.all(want[4] == 1e-99) and all((want[s] > 1e-99).any() for s in (1, 2, 3, 5, 6))
    assert np.all(want[:, n - 1] == 1e-99) or process == "ic"
    # two calls give identical bits
    assert bits_equal(hb.photon_observe(process, emis=emis, **tabs), got)


@pytest.mark.parametrize("process", cons.PHOTON_PROCESSES)
def test_three_zones_have_the_serial_restatement_s_bits(ctx, process):
    prob, hb = ctx
    ng, n_photon = prob.params.n_grid, 24
    ends = [0, 3, 4, 5, 6]                               # zone 3 (dense, beta 0.6), zone 4 (top lines, 0.9), zone 5 (sub-1e-90, 0.9798)
    tabs = tables(process, ng, n_photon, BETAS, ends)
    emis = crafted_emis(process, ng, n_photon, tabs)
    got = hb.photon_observe(process, emis=emis, **tabs)
    sub = dict(tabs, gam_ef=tabs["gam_ef"][2:5], beta_ef=tabs["beta_ef"][2:5], gam3_ef=tabs["gam3_ef"][2:5], shell_ends=np.array([0, 1, 2, 3, 4]))
    want = serial_restatement(process, emis[2:5], **sub)
    assert bits_equal(got, want) and (want[-1] > 1e-99).sum() >= n_photon - 2


def test_stock_shapes_have_the_host_bits(ctx):
    prob, hb = ctx
    ng = prob.params.n_grid
    rng = np.random.default_rng(7)
    ends = [1, 5, 6, ng // 2, ng + 1]
    for process in cons.PHOTON_PROCESSES:
        n_photon = cons.photon_n_photon(process)
        assert n_photon == {"synch": 180, "ic": 140, "pion": 120}[process]
        tabs = tables(process, ng, n_photon, rng.choice(BETAS, ng), ends, e_min_mev=cons.photon_e_min(process))
        flux = np.where(rng.random((ng, n_photon)) < 0.8, 10.0 ** rng.uniform(-20, -2, (ng, n_photon)), 1e-99)
        emis = flux * tabs["energy_div"][None, :] * (cons.MEV_ERG if process == "ic" else tabs["area"] * (cons.MEV_ERG if process == "synch" else 1.0))
        want = cons.shell_spectra_host(process, emis, **tabs)
        got = hb.photon_observe(process, emis=emis, **tabs)
        print(f"{process}: {(want > 1e-99).sum()} lit words of {want.size}; {(got != want).sum()} differ")
        assert (want > 1e-99).mean() > 0.9 and bits_equal(got, want), process


def folds_on(prob, hb, tabs_c, n_photon):
    """K4 and the three folds on the context's tallies -> process -> (E_erg, emis) as the device returned them."""
    P = prob.params
    dndp, _ = hb.dndp_cr(tabs_c)
    out = {"synch": hb.photon_synch(dndp[1], tabs_c.mom_edge_cgs, tabs_c.mc, n_photon["synch"], 1e-13, 10)}
    target = np.full(P.n_grid, 1.0)
    out["pion"] = hb.photon_pion(dndp[1], tabs_c.mom_edge_cgs, tabs_c.mc, 1.0, target, 1.0, n_photon["pion"], 1.0, 10)
    hb.dndp_2d(tabs_c, P.gam0, P.beta0, download=False)
    alpha_in, n_in = cons.photon_field_cmb(0.0)
    out["ic"] = hb.photon_ic(tabs_c.mom_edge_cgs, tabs_c.mc, P.num_psd_tht_bins, alpha_in, n_in, n_photon["ic"], 1e-2, 10, 4 * math.pi * (3.0e24) ** 2 * 0.03)
    return out


def test_chain_from_the_tallies(ctx):
    """emis = NULL takes what the fold left on the context: the same words as the call fed the array the fold returned; the flag is clear
    before a fold, after a write of the tallies and after begin_species."""
    prob, hb = ctx
    ng = prob.params.n_grid
    L = mcs.capi.Layout(prob.params)
    tabs_c = cons.consumer_tables(prob, 1)
    n_photon = {"synch": 24, "pion": 31, "ic": 40}
    hb.begin_iteration(1)
    hb.write_tallies(*crafted_buffers(L, 1)[0])
    ends = [1, 9, ng // 2, ng + 1]
    obs = {p: tables(p, ng, n_photon[p], BETAS, ends, e_min_mev=cons.photon_e_min(p)) for p in cons.PHOTON_PROCESSES}
    for p in cons.PHOTON_PROCESSES:
        with pytest.raises(RuntimeError, match="no emission of this process"):
            hb.photon_observe(p, **obs[p])
    folds = folds_on(prob, hb, tabs_c, n_photon)
    lit = 0
    for p in cons.PHOTON_PROCESSES:
        E_erg, emis = folds[p]
        kept = hb.photon_observe(p, **obs[p])
        fed = hb.photon_observe(p, emis=emis, **obs[p])
        assert same_words(kept, fed), p
        lit += int((kept > 1e-99).sum())
        with pytest.raises(RuntimeError, match="energies on the context"):
            hb.photon_observe(p, **tables(p, ng, n_photon[p] + 1, BETAS, ends))
    print("lit words of the chain:", lit)
    assert lit > 0
    # an observation of one process leaves the others' emission where it was; the second fold of a process replaces its own
    again = hb.photon_observe("synch", **obs["synch"])
    assert same_words(again, hb.photon_observe("synch", emis=folds["synch"][1], **obs["synch"]))
    hb.write_tally("scalars", np.zeros(4))
    with pytest.raises(RuntimeError, match="no emission of this process"):
        hb.photon_observe("pion", **obs["pion"])
    folds_on(prob, hb, tabs_c, n_photon)
    hb.photon_observe("ic", **obs["ic"])
    hb.begin_species(1, 1, 1.0, 1.0, prob.pmax, 1.0, 1.0)
    for p in cons.PHOTON_PROCESSES:
        with pytest.raises(RuntimeError, match="no emission of this process"):
            hb.photon_observe(p, **obs[p])


def kept_on_device(hb, process, n_shells, n):
    """What the last mcs_photon_observe of `process` left on the context, [n_shells + 1][n]: read through a photons sample of a fresh
    accumulator (one sample: the mean is the sample), the only reader of that buffer.  The sample clears the context's photon flags."""
    words = {p: n if p == process else 5 for p in cons.PHOTON_PROCESSES}
    e = mcs.ensemble.HipEnsemble(hb, 1)
    e.set_photon_layout(cons.PhotonLayout(n_shells, words, {p: 0 for p in cons.PHOTON_PROCESSES}, n))
    try:
        e.add_photons(hb, 0)
        return e.mean(e.photons_slot(0), process)
    finally:
        e.destroy()


def test_refusals_change_nothing(ctx):
    prob, hb = ctx
    ng, n_photon = prob.params.n_grid, 24
    hb.begin_species(1, 1, 1.0, 1.0, prob.pmax, 1.0, 1.0)           # (no observation of another process is left on the context)
    emis, tabs = crafted_case("synch", ng, n_photon)
    before = hb.photon_observe("synch", emis=emis, **tabs)
    out = np.full_like(before, -7.0)

    def call(process="synch", **change):
        kw = dict(tabs, emis=emis); kw.update(change)
        return hb.photon_observe(process, **kw)

    def changed(name, index, value):
        a = np.array(tabs[name], dtype=np.float64); a[index] = value
        return {name: a}

    big = tables("synch", ng, 257, BETAS, tabs["shell_ends"])
    bad_ends = tabs["shell_ends"].copy(); bad_ends[-1] = ng + 2
    neg_ends = tabs["shell_ends"].copy(); neg_ends[1] = -1
    refused = [
        ("n_photon = 257", lambda: hb.photon_observe("synch", emis=np.ones((ng, 257)), **big)),
        ("n_photon = 2", lambda: hb.photon_observe("synch", emis=np.ones((ng, 2)), **tables("synch", ng, 2, BETAS, tabs["shell_ends"]))),
        ("gam_ef", lambda: call(**changed("gam_ef", 3, np.nan))),
        ("gam_ef", lambda: call(**changed("gam_ef", 0, np.inf))),
        ("gam_ef", lambda: call(**changed("gam3_ef", 5, np.inf))),
        ("beta_ef", lambda: call(**changed("beta_ef", 2, np.nan))),
        ("beta_ef", lambda: call(**changed("beta_ef", 2, 1.0))),
        ("beta_ef", lambda: call(**changed("beta_ef", ng - 1, -0.1))),
        ("energy 4", lambda: call(**changed("energy_grid", 4, np.inf))),
        ("energy 0", lambda: call(**changed("energy_div", 0, np.nan))),
        ("energy_grid decreases", lambda: call(**changed("energy_grid", 7, tabs["energy_grid"][5]))),
        ("cos_edge", lambda: call(**changed("cos_edge", 90, np.nan))),
        ("shell_ends", lambda: call(shell_ends=bad_ends)),
        ("shell_ends", lambda: call(shell_ends=neg_ends)),
        ("area", lambda: call(area=0.0)),
        ("dlog", lambda: call(dlog=np.nan)),
        ("last_mid_ratio", lambda: call(last_mid_ratio=0.5)),
        ("no emission of this process", lambda: call(emis=None)),
    ]
    for msg, f in refused:
        with pytest.raises(RuntimeError, match="mcs_photon_observe.*" + msg):
            f()
    # no successful call since `before`: what the device kept is still that result, bit for bit
    assert bits_equal(kept_on_device(hb, "synch", 6, n_photon - 1), before)
    with pytest.raises(RuntimeError, match="mcs_ens_add_photons"):      # (the sample took it)
        kept_on_device(hb, "synch", 6, n_photon - 1)
    assert bits_equal(hb.photon_observe("synch", emis=emis, **tabs), before)
    # null tables and an unknown process, past the wrapper
    lib, dp = hb.lib, lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(mcs.capi.c_double_p)
    ends = np.ascontiguousarray(tabs["shell_ends"], dtype=np.int64)
    keep = [np.ascontiguousarray(emis)] + [np.ascontiguousarray(tabs[k], dtype=np.float64) for k in ("energy_div", "energy_grid", "cos_edge", "gam_ef", "beta_ef", "gam3_ef")]
    ptrs = [dp(a) for a in keep]

    def raw(process, which_null):
        p = list(ptrs)
        if which_null is not None and which_null < 7:
            p[which_null] = None
        e = None if which_null == 7 else ends.ctypes.data_as(mcs.capi.c_int64_p)
        return lib.mcs_photon_observe(hb.h, process, n_photon, p[0], p[1], p[2], tabs["area"], tabs["dlog"], tabs["last_mid_ratio"], p[3], p[4], p[5], p[6],
                                      len(ends) - 1, e, dp(out))
    for which in range(1, 8):
        assert raw(0, which) != 0 and b"null table" in lib.mcs_last_error()
    assert raw(3, None) != 0 and b"process" in lib.mcs_last_error()
    assert raw(-1, None) != 0
    assert np.all(out == -7.0)                      # no refusal wrote the caller's array
    assert bits_equal(kept_on_device(hb, "synch", 6, n_photon - 1), before)      # ... nor the result kept on the device
    assert raw(0, None) == 0 and bits_equal(out, before)


def test_non_finite_emission_has_the_host_bits(ctx):
    """The emission is not checked: a NaN is no flux (every floor test is false for it), an infinity stays one; host and device agree."""
    prob, hb = ctx
    ng, n_photon = prob.params.n_grid, 24
    for process in cons.PHOTON_PROCESSES:
        emis, tabs = crafted_case(process, ng, n_photon)
        emis[1, 3] = np.nan; emis[2, :] = np.nan; emis[7, 6] = np.inf; emis[8, 2] = -np.inf; emis[9, 4] = -1.0
        with np.errstate(all="ignore"):
            want = cons.shell_spectra_host(process, emis, **tabs)
        got = hb.photon_observe(process, emis=emis, **tabs)
        assert same_words(got, want) and np.isinf(want).any() and not np.isnan(want).any(), process
