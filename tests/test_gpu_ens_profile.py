"""The profile sample of the ensemble statistics on the device (mcs_ens_add_profile in csrc/mcs_ensemble.hip, through
ensemble.HipEnsemble) against ensemble.HostEnsemble fed the same ProfileUpdate: count, mean and M2 of four crafted samples word for
word, the merge, the two summaries, a trigger, a comparison of two accumulators, profile_consistency, and the refusals."""
import copy

import numpy as np
import pytest

import ens_compare_common as cmpc
import profile_common as pc
from conftest import mcs, make_problem, hip_backend
from ensemble_common import same_words
from ens_summary_common import as_dict, assert_exact, assert_sums, restate

pytestmark = pytest.mark.gpu

ens = mcs.ensemble
cons = mcs.consumers


def pin_of(c, **kw):
    d = {k: c[k] for k in cons.PROFILE_SETTINGS}
    d.update(hist_q_px=c["hist_q_px"], hist_q_en=c["hist_q_en"], pxx_EM=c["pxx_EM"], en_EM=c["en_EM"], atan_x=c["atan_x"])
    d.update(kw)
    return cons.ProfileIn(**d)


def variant(c0, seed):
    """The base case with other fluxes and another q history: the same settings."""
    c = copy.deepcopy(c0)
    rng = np.random.default_rng(seed)
    c["pxx_flux"] = c["pxx_flux"] * (1 + 1e-3 * rng.standard_normal(c["n_grid"]))
    c["energy_flux"] = c["energy_flux"] * (1 + 1e-3 * rng.standard_normal(c["n_grid"]))
    c["hist_q_px"], c["hist_q_en"] = ((), ()) if seed % 2 else ((0.01 * seed,), (0.02,))
    return c


def update(prob, hb, c, **kw):
    """The case on the context (fluxes and scalars into the tallies, NaN elsewhere) and the device call -> ProfileUpdate."""
    _, i = hb.read_tallies()
    hb.write_tallies(pc.crafted_tallies(hb.layout, c), i)
    pin = pin_of(c, **kw)
    out, diag = hb.profile_update(pin, (c["P_par"], c["P_perp"], c["e_dens"]))
    return cons._profile_from_words(out, diag, prob.n_grid, pin.settings())


@pytest.fixture(scope="module")
def fed():
    """One context, four crafted samples of one setting, and a device and a numpy accumulator that took each."""
    prob = make_problem(64)
    hb = hip_backend(prob)
    hb.begin_iteration(1)
    hb.begin_species(1, 1, 1.0, 1.0, prob.pmax, 1.0, 1.0)
    c0 = pc.make_cases(prob)[0][1]
    e, h = ens.HipEnsemble(hb, 1), ens.HostEnsemble(prob.params, 1)
    ups = []
    for seed in range(4):
        u = update(prob, hb, variant(c0, seed))
        e.add_profile(hb, u)
        h.add_profile(hb, u)
        ups.append(u)
    yield prob, hb, c0, e, h, ups
    e.destroy(); hb.destroy()


def test_count_mean_and_m2(fed):
    prob, hb, c0, e, h, ups = fed
    s = e.profile_slot
    n = prob.n_grid
    total = e.layout.profile_fields()["total"]
    assert e.count(s) == 4 and e.count(0) == 0 and e.count(e.photons_all_slot) == 0 and total == 10 * n + 8 and total % 256 != 0
    for name in ens.PROFILE_NAMES:
        assert same_words(e.mean(s, name), h.mean(s, name)), f"mean of {name}"
        assert same_words(e.m2(s, name), h.m2(s, name)), f"M2 of {name}"
    assert same_words(e._read(s, 0, 0, total), h._read(s, 0, 0, total)) and same_words(e._read(s, 1, 0, total), h._read(s, 1, 0, total))
    mean, err, k = ens.stats_over([u.words() for u in ups])
    assert k == 4 and same_words(e._read(s, 0, 0, total), mean) and same_words(e._read(s, 2, 0, total), err)
    assert h.m2(s, "ux_next").max() > 0 and np.isfinite(h.mean(s, "shift")).all()
    a, b = ens.profile_consistency(e), ens.profile_consistency(h)
    assert a.n == 4 and same_words(a.z, b.z) and a.chi2_upstream == b.chi2_upstream and a.n_upstream == b.n_upstream > 0


def test_merge_summaries_trigger_and_comparison(fed):
    prob, hb, c0, e, h, ups = fed
    s = e.profile_slot
    n = prob.n_grid
    total = e.layout.profile_fields()["total"]
    a, b, c = (ens.HipEnsemble(hb, 1) for _ in range(3))
    ha, hb_ = ens.HostEnsemble(prob.params, 1), ens.HostEnsemble(prob.params, 1)
    try:
        for k in range(4):
            u = update(prob, hb, variant(c0, k))
            (a if k < 2 else b).add_profile(hb, u)
            (ha if k < 2 else hb_).add_profile(hb, u)
        reqs = [ens.Request("ux_next"), ens.Request("shift", (0, prob.params.i_shock), 0.0, 0.5), ens.Request("scalars"), ens.Request("ux_pred", (3, 40), 1e-3, 0.1)]
        merged, hmerged = a.summarize_merged([b], s, reqs), ha.summarize_merged([hb_], s, reqs)
        # a comparison of the two halves, before they are merged
        creqs = [ens.CompareRequest("ux_next", None, 0.0, 2.0), ens.CompareRequest("shift", (0, 30), 0.0, 1.0)]
        ma, qa = a._read(s, 0, 0, total), a._read(s, 1, 0, total)
        mb, qb = b._read(s, 0, 0, total), b._read(s, 1, 0, total)
        diffs, hdiffs = a.compare(b, s, creqs), ha.compare(hb_, s, creqs)
        for q, d, hd in zip(creqs, diffs, hdiffs):
            first, count = a.word_range(s, q.name, q.zones, q.bins)
            sl = slice(first, first + count)
            want = cmpc.restate(ma[sl], qa[sl], 2, mb[sl], qb[sl], 2, q.floor_frac, q.zcut)
            for res in (d, hd):
                cmpc.assert_exact(cmpc.as_dict(res), want, repr(q)); cmpc.assert_sums(cmpc.as_dict(res), want, repr(q))
        ha.merge(hb_)
        a.merge(b)
        c.merge(a)                                     # an accumulator without profile samples takes the source's settings
        assert a.count(s) == 4 and b.count(s) == 2 and c.count(s) == 4
        for acc in (a, c):
            for name in ens.PROFILE_NAMES:
                assert same_words(acc.mean(s, name), ha.mean(s, name)) and same_words(acc.m2(s, name), ha.m2(s, name)), name
        mean, m2 = a._read(s, 0, 0, total), a._read(s, 1, 0, total)
        got, host = a.summarize(s, reqs), ha.summarize(s, reqs)
        for q, r, hr, mr, hmr in zip(reqs, got, host, merged, hmerged):
            first, count = a.word_range(s, q.name, q.zones, q.bins)
            want = restate(mean[first:first + count], m2[first:first + count], 4, q.floor_frac, q.tol)
            for res in (r, hr, mr, hmr):
                assert res.n == 4
                assert_exact(as_dict(res), want, repr(q)); assert_sums(as_dict(res), want, repr(q))
        assert got[1].n_nonfinite == 0 and got[0].n_selected > 10
        loose, tight = (ens.Trigger(s, "ux_next", "max", thr, zones=(0, 40)) for thr in (1.0, 1e-12))
        for acc in (a, ha):
            rows = mcs.driver._check_triggers(acc, [loose, tight])
            assert [r.met for r in rows] == [True, False], [r.value for r in rows]
        c.add_profile(hb, update(prob, hb, variant(c0, 9)))     # ... and goes on sampling with them
        assert c.count(s) == 5
    finally:
        for acc in (a, b, c):
            acc.destroy()


def test_refusals(fed):
    prob, hb, c0, e, h, ups = fed
    s = e.profile_slot
    with pytest.raises(RuntimeError, match="mcs_ens_add_profile: the context needs an mcs_profile_update"):
        e.add_profile(hb)                              # the last result was taken by the fixture's last sample
    u = update(prob, hb, variant(c0, 5))
    _, i = hb.read_tallies()
    hb.write_tallies(pc.crafted_tallies(hb.layout, c0), i)      # a tally write invalidates the result
    with pytest.raises(RuntimeError, match="mcs_ens_add_profile: the context needs an mcs_profile_update"):
        e.add_profile(hb, u)
    update(prob, hb, variant(c0, 5))
    hb.begin_species(1, 1, 1.0, 1.0, prob.pmax, 1.0, 1.0)      # ... and so does the next species
    with pytest.raises(RuntimeError, match="mcs_ens_add_profile: the context needs an mcs_profile_update"):
        e.add_profile(hb, u)
    odd = update(prob, hb, variant(c0, 6), w=float(np.nextafter(c0["w"], 2.0)))      # one bit of one setting
    with pytest.raises(RuntimeError, match="mcs_ens_add_profile: the settings"):
        e.add_profile(hb, odd)
    assert e.count(s) == 4
    other = ens.HipEnsemble(hb, 1)
    fresh = ens.HipEnsemble(hb, 1)
    try:
        other.add_profile(hb, odd)                     # (the refused sample left the result in place)
        other.add_profile(hb, update(prob, hb, variant(c0, 7), w=odd.settings[12]))
        with pytest.raises(RuntimeError, match="mcs_ens_merge: the settings of the accumulators' profile samples differ"):
            e.merge(other)
        with pytest.raises(RuntimeError, match="mcs_ens_summarize_merged: the settings of the accumulators' profile samples differ"):
            e.summarize_merged([other], s, [ens.Request("shift")])
        with pytest.raises(RuntimeError, match="mcs_ens_compare: the settings of the accumulators' profile samples differ"):
            e.compare(other, s, [ens.CompareRequest("shift")])
        with pytest.raises(RuntimeError, match="mcs_ens_read: range outside the slot's sample vector"):
            fresh.mean(s, "shift")                         # (a profile slot that never took a sample has no vector)
        assert fresh.count(s) == 0
        with pytest.raises(ValueError):
            e.compare(other, s, [ens.CompareRequest("shift")], other_slot=0)
    finally:
        other.destroy(); fresh.destroy()
