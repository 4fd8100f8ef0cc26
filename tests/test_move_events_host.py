"""The states of tests/move_common.py and the oracle's side of mcs_eval_move, on the CPU.

orc_eval_move (one pass's Code Block 2 per state: oracle/mcs_oracle.cpp, the function particle_loop itself calls) is checked against the
numpy restatement of move_common, which shares no code with it: the move of a parallel field in plain IEEE operations, the zone search
by np.searchsorted, the shock crossing with its PRP update, `inj`, the time cut, and the exits that downstream_test and a PRP crossing
with vt < u2 decide.  The thresholds' table (np_thresholds) is checked against the events on the same states, and three of its
compares are flipped (the `>=` of the upstream FEB in refresh_thr, the `>=` and `<=` of move_and_detect_thr) to show that the states tell
the difference -- the CPU twin of flipping them in the kernel."""
import functools

import numpy as np
import pytest

from conftest import oracle_backend
import move_common as mv

u64 = mv.u64


@functools.lru_cache(maxsize=None)
def material(name):
    case = mv.make_case(name)
    S = mv.build_states(case)
    x_new, phi_new = mv.first_move(case, S.pop)
    ob = oracle_backend(case.prob)
    case.begin(ob)
    ob.set_retro_cap(mv.RETRO_CAP)
    out, word, log = ob.eval_move(S.pop, mv.I_PCUT)
    found = ob.zone_search(x_new, x_new > S.pop.x_PT_cm, S.pop.grid)
    ob.destroy()
    for a in (x_new, phi_new, out, word, found):
        a.setflags(write=False)
    return case, S, x_new, phi_new, out, word, log, found


@pytest.mark.parametrize("problem", mv.PROBLEMS)
def test_builder(problem):
    case, S, x_new = material(problem)[:3]
    counts = mv.check_states(case, S, x_new)
    print(f"\n{problem}: {S.n} states; class: (states, x_new below / on / above the target)")
    for c, v in counts.items():
        print(f"    {c:12s} {v}")
    assert S.n % 256 != 0 and counts["fuzz"][0] >= mv.N_FUZZ
    # the zone search: moves over 1, 2, 3, 4 and dozens of zones in both directions, all three probes and both ends of the bisection
    xg = mv.tables(case).xg
    ig = S.pop.grid
    found = mv.np_zone_search(xg, x_new, x_new > S.pop.x_PT_cm, ig)
    span = np.where(found >= 0, found - ig, 0)
    for sp in (1, 2, 3, 4, -1, -2, -3, -4):
        assert np.any(span == sp), f"{problem}: no move over {sp} zones"
    assert np.any(span >= 24) and np.any(span <= -24)
    fwd = x_new > S.pop.x_PT_cm
    # (with the oblique field of that problem no momentum outruns the upstream flow: b_cos = cos 0.35 < u_x / c, so nothing moves off
    # the upstream end there)
    assert np.any((found < 0) & fwd) and (np.any((found < 0) & ~fwd) or not mv.parallel(case)), f"{problem}: no move off both ends of the grid"
    assert np.any((found == len(xg) - 2) & fwd & (span > 3)) and np.any((found <= 1) & ~fwd & (span < -3)), f"{problem}: the bisection's ends"
    on_edge = np.isin(x_new, xg)
    assert on_edge.sum() > 100 and np.any(on_edge & fwd) and np.any(on_edge & ~fwd)


@pytest.mark.parametrize("problem", mv.PROBLEMS)
def test_zone_search_against_searchsorted(problem):
    case, S, x_new, _, _, _, _, found = material(problem)
    xg = mv.tables(case).xg
    fwd = x_new > S.pop.x_PT_cm
    assert np.array_equal(found, mv.np_zone_search(xg, x_new, fwd, S.pop.grid))
    # ... and from every zone to every edge, its neighbours, and beyond both ends, in both directions
    ob = oracle_backend(case.prob)
    xs = np.concatenate([xg, np.nextafter(xg, -np.inf), np.nextafter(xg, np.inf), [-np.inf, np.inf, 0.0, -0.0]])
    X, G, F = np.meshgrid(xs, np.arange(len(xg)), [0, 1], indexing="ij")
    got = ob.zone_search(X.ravel(), F.ravel(), G.ravel())
    ob.destroy()
    assert np.array_equal(got, mv.np_zone_search(xg, X.ravel(), F.ravel() != 0, G.ravel()))
    assert (got < 0).sum() > 100


@pytest.mark.parametrize("problem", mv.PROBLEMS)
def test_oracle_move_against_numpy(problem):
    case, S, x_new, phi_new, out, word, log, found = material(problem)
    P, pop = case.prob.params, S.pop
    w = mv.unpack(word)
    d = mv.np_derive(case, pop)
    x_old = pop.x_PT_cm
    ev = mv.np_events(case, pop, x_old, x_new, d)
    # the domain of the bit-for-bit statements: no random number was drawn (no retry of no_DSA_loop, no PRP return decided by a draw)
    calm = w["draws"] == 0
    assert calm.mean() > 0.9, f"{problem}: only {calm.mean():.0%} of the states draw nothing"
    assert np.array_equal(u64(out[:, 1]), u64(x_old))
    if mv.parallel(case):
        assert np.array_equal(u64(out[calm, 0]), u64(x_new[calm])), "the move differs from its numpy restatement"
        assert np.array_equal(u64(out[calm, 2]), u64(phi_new[calm]))
    assert np.array_equal(u64(out[calm, 6]), u64(d["gam"][calm])) and np.array_equal(u64(out[calm, 5]), u64(pop.ptot_pf[calm]))
    # a retry means: x_new <= 0 < x_old, not injected, in a configuration with the loop
    assert np.all(ev["reflect"][~calm & (w["n_retro"] == 0) & (w["end"] != 1) & ~ev["prp"]])
    # zone search, D6
    off = found < 0
    assert np.array_equal(w["end"][calm] == 3, off[calm]), "end code 3 is not 'the zone search ran off the grid'"
    ok = calm & ~off
    assert np.array_equal(w["i_grid"][ok], found[ok]) and np.array_equal(w["i_grid_old"], pop.grid) and np.array_equal(w["ig3"], pop.grid)
    # the shock crossing: downstream, the PRP update, inj
    shock = (x_old < 0) & (x_new >= 0)
    L_shock = P.eta_mfp / 3 * d["grt"] * pop.ptot_pf / (d["m"] * d["gam"] * P.u2)
    down = (pop.downstream != 0) | shock
    inj = (pop.inj != 0) | (down & (x_new < 0))
    assert np.array_equal(w["downstream"][calm], down[calm].astype(np.int64)) and np.array_equal(w["inj"][calm], inj[calm].astype(np.int64))
    assert shock.sum() > 50 and (shock & (L_shock > pop.prp_x_cm)).sum() > 5 and (shock & (L_shock < pop.prp_x_cm)).sum() > 5
    prp_after_shock = np.where(shock & (L_shock > pop.prp_x_cm), L_shock, pop.prp_x_cm)
    quiet = ok & ~ev["stop"] & ~((x_new >= P.x_grid_stop) & bool(case.aa < 1))        # (neither of prob_return's own PRP updates)
    assert np.array_equal(u64(out[quiet, 7]), u64(prp_after_shock[quiet])), "the PRP after the move differs (shock crossing: max(prp, L_diff))"
    # the time cut of the pass
    nt = len(case.prob.tcuts)
    tc_ = np.asarray(case.prob.tcuts, dtype=np.float64)
    cut = (pop.downstream != 0) & bool(P.do_tcuts) & (pop.tcut <= nt) & (pop.acctime_sec >= tc_[np.minimum(pop.tcut, nt) - 1])
    assert np.array_equal(w["tcut"][calm], (pop.tcut + cut)[calm]) and cut.sum() >= 2 * nt
    # the exits: downstream_test, or a PRP crossing with vt < u2 (decided without a draw)
    vt = pop.ptot_pf / (d["gam"] * case.aa * mv.MP)
    prp_no_return = ev["prp"] & ~ev["stop"] & (vt < P.u2)
    want_exit = ev["dtest"] | prp_no_return
    assert np.array_equal(w["end"][ok] == 1, want_exit[ok]), "end code 1 is not 'downstream_test or a PRP crossing with vt < u2'"
    assert np.all(w["end"][ok & ~want_exit] == mv.GOES_ON)
    if not P.feb_downstream > 0:
        assert (prp_no_return & ok).sum() >= 30 and np.any(w["n_retro"] > 10), f"{problem}: no retro walk of more than ten steps"
        print(f"\n{problem}: {int((w['n_retro'] > 0).sum())} PRP returns, retro walks of up to {int(w['n_retro'].max())} steps")
    # the flags of a particle that goes on
    on = ok & (w["end"] == mv.GOES_ON)
    assert np.array_equal(w["crossed"][on], (found != pop.grid)[on].astype(np.int64)) and np.array_equal(w["zone"][on], w["crossed"][on])
    assert np.all(w["b1"][calm] == 0) and np.all(w["b1"][w["n_retro"] == 0] == 0)
    # what all_flux! tallied: left the zone, or an FEB zone, or detectors
    tallied = ~off & ~((found == pop.grid) & (pop.grid > P.i_grid_feb) & (len(case.prob.x_spec) == 0))
    assert np.array_equal(w["npush"][calm], tallied[calm].astype(np.int64))
    # the log names states, and a state that tallied nothing and ended nowhere logs nothing
    lr = log[0]
    silent = calm & ~tallied & ~cut & (w["end"] == mv.GOES_ON)
    assert not np.any(np.isin(lr, np.flatnonzero(silent))) and (silent.sum() > 100 or len(case.prob.x_spec) != 0)


@pytest.mark.parametrize("problem", mv.PROBLEMS)
def test_thresholds_table_misses_nothing(problem):
    """The table above refresh_thr, restated (np_thresholds), against the events due: whatever is due reaches a threshold (or is an
    event of the odd configurations, which the event bit carries); and three compares flipped, one at a time, each miss something."""
    case, S, x_new = material(problem)[:3]
    pop = S.pop
    d = mv.np_derive(case, pop)
    ev = mv.np_events(case, pop, pop.x_PT_cm, x_new, d)
    dom = mv.contract_domain(case, pop, S.x_thr, d)

    def missed(no_xn=False, mutate=None):
        hi, lo, _ = mv.np_thresholds(case, pop, S.x_thr, d, no_xn=no_xn, mutate=mutate)
        up = (x_new > hi) if mutate == "hi_gt" else (x_new >= hi)            # (move_and_detect_thr's own two compares)
        dn = (x_new < lo) if mutate == "lo_lt" else (x_new <= lo)
        return np.flatnonzero(mv.np_due(ev, no_xn) & ~(up | dn | ev["odd"]) & dom)
    for no_xn in (False, True):
        m = missed(no_xn)
        assert len(m) == 0, f"{problem}: the table misses {len(m)} events, first {mv.describe(S, int(m[0]))}"
    P = case.prob.params
    if len(case.prob.x_spec) == 0:      # (with detectors every pass is an event: the thresholds decide nothing)
        # (nothing moves upstream from the FEB in the oblique problem: see test_builder)
        assert len(missed(mutate="feb_gt")) > 0 or not mv.parallel(case), "x_thr == feb_upstream, injected, moving upstream: no state tells `>=` from `>` in refresh_thr"
        m = missed(mutate="hi_gt")
        assert len(m) > 100 and "edge" in set(S.cls[m]) and ("x_grid_stop" in set(S.cls[m]) or case.aa < 1), "x_new ON a zone edge / the grid end: no state tells `>=` from `>`"
        assert len(missed(mutate="lo_lt")) > 0, "x_new ON gyro_rad_tot with coarse steps: no state tells `<=` from `<`"
    # and the stops with nothing due are those the table allows
    hi, lo, _ = mv.np_thresholds(case, pop, S.x_thr, d)
    spurious = ((x_new >= hi) | (x_new <= lo)) & ~mv.np_due(ev) & dom
    cat = mv.np_spurious(case, pop, S.x_thr, x_new, d)
    unexplained = spurious & ~(cat["boundary"] | cat["rearm"] | cat["beyond_dt"] | cat["prp_below"])
    assert not unexplained.any(), f"{problem}: a stop the table does not allow: {mv.describe(S, int(np.flatnonzero(unexplained)[0]))}"
    assert not (spurious & cat["beyond_dt"]).any()        # (x > x_dt is downstream_test's exit itself: always due)
    assert ((spurious & cat["boundary"]).sum() > 0 and (spurious & cat["rearm"]).sum() > 0) or len(case.prob.x_spec) != 0
    print(f"\n{problem}: stops with nothing due (numpy table):", {k: int((spurious & v).sum()) for k, v in cat.items()},
          f"outside the contract: {int((~dom).sum())} of {S.n}")
