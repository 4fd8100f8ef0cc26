"""The references of tests/test_gpu_pass_head.py checked against each other on the CPU: the oracle's pass boundary (orc_eval_pass: the
functions particle_loop itself calls -- code_block_2, code_block_3_head, code_block_3_rest) against the numpy restatement of
tests/pass_common.py, state by state, and the builder's own assertions (below / on / above per class, the share of every crafted class
that reaches the test it aims at, every end of the head present)."""
import functools

import numpy as np
import pytest

from conftest import oracle_backend
import move_common as mv
import pass_common as pc

u64 = pc.u64
COLS = pc.COLS


@functools.lru_cache(maxsize=None)
def material(name):
    case = pc.make_case(name)
    S = pc.build_states(case)
    return pc.reference(case, S)


def first_bad(bad):
    return int(np.flatnonzero(bad)[0])


@pytest.mark.parametrize("problem", pc.PROBLEMS)
def test_states_land_on_their_branches(problem):
    m = material(problem)
    counts = pc.check_states(m["case"], m["S"], m)
    print(f"\n{problem}: {m['S'].n} states; class: (states, below, on, above, share that reached its test)")
    for k, v in counts.items():
        print("   ", k, v)
    assert 5000 <= m["S"].n <= 8500


@pytest.mark.parametrize("problem", pc.PROBLEMS)
def test_oracle_equals_the_restatement(problem):
    m = material(problem)
    S, r, out = m["S"], m["np"], m["out"]
    w = pc.unpack(m["word"])
    cov = r["covered"]
    assert cov.all()          # (the frame change and both energy transfers are restated: every state is classified)
    bad = cov & (r["end"] != w["pre_end"])
    assert not bad.any(), f"{problem}: the head ends {int(w['pre_end'][first_bad(bad)])} in the oracle, {int(r['end'][first_bad(bad)])} in the restatement; {pc.describe(S, first_bad(bad))}"
    # whether the head runs at all is stated for every state
    assert np.array_equal(r["runs"], w["pre_end"] != pc.NOT_RUN)
    past = cov & (r["stage"] > pc.STAGES.index("helix"))          # (the helix cap ends a particle before anything is recomputed)
    alive = past & (w["pre_end"] == pc.GOES_ON)
    assert alive.sum() > 500
    for f, c, mask in (("ptot", "ptot_pf", past), ("gam", "gam_pf", past), ("grt", "gyro_rad_tot", past), ("gr", "gyro_rad", past),
                       ("gd", "gyro_denom", past), ("xn", "xn_per", past), ("pb", "pb_pf", alive), ("pperp", "p_perp", alive), ("phi", "phi", alive)):
        d = (u64(r[f]) != u64(out[:, COLS[c]])) & mask
        assert not d.any(), f"{problem}: {c} of {int(d.sum())} states differs, first {float(r[f][first_bad(d)]).hex()} against the oracle's {float(out[first_bad(d), COLS[c]]).hex()}; {pc.describe(S, first_bad(d))}"
    # dphi and t_step follow the NEW xn_per, and the flags are their predicates, in the oracle's own output
    go = w["pre_end"] == pc.GOES_ON
    assert np.array_equal(u64(out[go, COLS["dphi"]]), u64(pc.TWOPI / out[go, COLS["xn_per"]]))
    assert np.array_equal(u64(out[go, COLS["t_step"]]), u64(out[go, COLS["gyro_period"]] / out[go, COLS["xn_per"]]))
    assert not w["f_save"][go].any() and np.all(w["f_save"][w["pre_end"] == pc.SAVED] == 1)
    # a saved particle has scattered (two draws) and its pass is counted
    sv = w["pre_end"] == pc.SAVED
    if not m["case"].prob.params.dont_scatter:
        assert np.all(w["draws"][sv] >= 2)
    assert np.array_equal(w["helix"][sv], S.helix[sv] + 1) and np.array_equal(w["helix"][go], S.helix[go])


@pytest.mark.parametrize("problem", mv.PROBLEMS)
def test_head_skipped_equals_eval_move(problem):
    """orc_eval_pass with helix = 1 and the head skipped (head = 0: the prologue's gyro period) is orc_eval_move: the same prologue, the
    same one call of code_block_2"""
    m = material(problem)
    case, S = m["case"], m["S"]
    ob = oracle_backend(case.prob)
    case.begin(ob)
    ob.set_retro_cap(mv.RETRO_CAP)
    T0, I0 = ob.read_tallies()
    one = np.ones(S.n, dtype=np.int32)
    po, pw, plog = ob.eval_pass(S.pop, one, pc.I_PCUT, head=0)
    Tp, Ip = ob.read_tallies()
    ob.write_tallies(T0, I0)
    mo, mw, mlog = ob.eval_move(S.pop, pc.I_PCUT)
    Tm, Im = ob.read_tallies()
    ob.destroy()
    mc = {n: i for i, n in enumerate(mv.OUT)}
    for n in mv.OUT:
        if n not in ("t_hi", "t_lo"):
            assert np.array_equal(u64(po[:, COLS[n]]), u64(mo[:, mc[n]])), f"{problem}: {n}"
    a, b = pc.unpack(pw), mv.unpack(mw)
    for n in ("i_grid", "i_grid_old", "ig3", "tcut", "downstream", "inj"):
        assert np.array_equal(a[n], b[n]), f"{problem}: {n}"
    assert np.array_equal(a["post_end"], b["end"]) and np.all(a["pre_end"] == pc.NOT_RUN)
    assert np.array_equal(np.minimum(b["draws"], 7), a["draws"]) and np.array_equal(np.minimum(b["n_retro"], 7), a["n_retro"])
    assert np.array_equal(u64(Tp), u64(Tm)) and np.array_equal(Ip, Im)
    for x, y in zip(plog, mlog):
        assert np.array_equal(x, y)


FLIPS = (("pmax", "> pmax_cutoff"), ("feb_up", "< feb_upstream"), ("age", "> age_max"), ("pcut", "> pcut"), ("dlnp", "> 1e-2"), ("grt", "> gyro_rad_tot"))


@pytest.mark.parametrize("name,text", FLIPS)
def test_each_comparison_is_told_from_its_non_strict_form(name, text):
    """Stating one comparison of the head the other way (`>` as `>=`, `<` as `<=`) changes what the restatement says of at least one
    state: the states sit ON every number the head compares with."""
    hits = {}
    for problem in pc.PROBLEMS:
        m = material(problem)
        case, S = m["case"], m["S"]
        ob = oracle_backend(case.prob)
        case.begin(ob)
        r = pc.np_head(case, ob, S.pop, S.helix, m["pre"], m["wpre"], mutate=name, pool=m["pool"])
        ob.destroy()
        diff = (r["end"] != m["np"]["end"]) | (u64(r["xn"]) != u64(m["np"]["xn"])) | (u64(r["ptot"]) != u64(m["np"]["ptot"]))
        hits[problem] = int(diff.sum())
    print(f"\n`{text}` stated the other way changes", hits)
    assert sum(hits.values()) > 0, f"no state tells `{text}` from its non-strict form"
    # ... in every problem that has the comparison (pcut: where no loss precedes it -- the loss moves a momentum that starts ON pcut off it)
    for problem, h in hits.items():
        P, aa = material(problem)["case"].prob.params, material(problem)["case"].aa
        has = dict(pmax=True, feb_up=True, age=P.age_max > 0, pcut=not (bool(P.do_rad_losses) and aa < 1), dlnp=bool(P.do_rad_losses) and aa < 1, grt=not P.dont_scatter)[name]
        assert h > 0 or not has, f"{problem}: no state tells `{text}` from its non-strict form"


# the largest error of the oracle's transform_p_PSP against 50 digits, measured over the frame changes of the states (ulps of ptot_pf
# for ptot_pf and pb_pf, ulps of pi for phi where p_perp / ptot_pf > 1e-3):
#   parallel field, frame changes at the shock only   12.04, 43.15, 1.95   (the largest over the nine such problems)
#   ramp (frame changes between downstream zones whose u_x differ by 5e-4: two boosts that nearly cancel, on slow particles)   67.76, 124.88, 1.95
#   oblique (the transform sums terms of both signs)   87.58, 345.16, 69.14
# Asserted: twice that (libm differs between machines; the check is for a wrong formula, not a last bit).
PSP_MEASURED = dict(shock=(12.04, 43.15, 1.95), ramp=(67.76, 124.88, 1.95), oblique=(87.58, 345.16, 69.14))


@pytest.mark.parametrize("problem", pc.PROBLEMS)
def test_frame_change_against_mpmath(problem):
    import math
    m = material(problem)
    case = m["case"]
    cases = pc.psp_cases(case, m["S"], m["pre"], m["wpre"])
    assert len(cases) > 500
    ob = oracle_backend(case.prob)
    case.begin(ob)
    e, n_phi = [0.0, 0.0, 0.0], 0
    for c in cases:
        o, r = pc.psp_oracle(case, ob, *c), pc.psp_mp(case.aa, *c)
        u = math.ulp(o[0])
        e[0], e[1] = max(e[0], abs(float((r[0] - o[0]) / u))), max(e[1], abs(float((r[1] - o[1]) / u)))
        if r[2] > 1e-3:
            n_phi += 1
            e[2] = max(e[2], abs(float((r[3] - o[4]) / math.ulp(math.pi))))
    ob.destroy()
    print(f"\n{problem}: {len(cases)} frame changes, {n_phi} with p_perp / ptot > 1e-3; largest error in ulps: ptot {e[0]:.2f}, pb {e[1]:.2f}, phi {e[2]:.2f}")
    bound = tuple(2 * v for v in PSP_MEASURED["oblique" if not mv.parallel(case) else ("ramp" if problem == "ramp" else "shock")])
    assert n_phi > 400 and all(a <= b for a, b in zip(e, bound)), f"{problem}: errors {e} against the bounds {bound}"
