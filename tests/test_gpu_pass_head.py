"""The head of a pass of the transport kernel -- everything between the end of one move and the next scatter -- state by state, on a
real MI355X.

mcs_eval_pass (include/mcs.h) runs one state per thread through the kernel's own load_particle, move_and_detect, slow_post and then
slow_pre (form 0) or the LOSSY kernel's in-line radiative loss (form 1), in the translation unit they ship in.  Before the move the
derived quantities and the flags are those the previous slow_pre left, so slow_pre recomputes only what a flag raised since then asks
for: a flag that a branch forgets to raise leaves a stale value in the output.  The references are orc_eval_pass -- the functions the
oracle's particle_loop calls once per pass, which recompute everything --, its deposit log, and the from-scratch statements of
tests/pass_common.py and tests/move_common.py.  The states: pass_common.build_states.

Every comparison is bit equality, except the tally cells with several terms (tally_common.check_launch: the a-priori bound of a sum in
any order) and the two refined reciprocals the oracle does not have (1/ptot_pf and 1/(gam_pf m): within one ulp of the quotient, which
two Newton steps on the hardware's estimate guarantee).  A state outside an assertion's domain is named by a mask whose size is
asserted.

Regression cases found with these tests keep their states in REGRESSIONS below (none so far)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import mcs, oracle_backend
import move_common as mv
import pass_common as pc
import tally_common as tc

pytestmark = pytest.mark.gpu

u64 = pc.u64
COLS = pc.COLS
COUNTS = {}
REGRESSIONS = {}             # name -> (problem, {field: [hex floats / ints]}, helix): states that once differed


@functools.lru_cache(maxsize=None)
def material(name):
    """The states of one problem and every reference, built once and never changed."""
    case = pc.make_case(name)
    S = pc.build_states(case)
    return pc.reference(case, S)


@pytest.fixture(scope="module")
def contexts():
    """One context per problem, holding the problem's states as its population, shared by the tests of the module."""
    from mcs_amd import hip_backend as hbm
    made, runs = {}, {}

    def get(name):
        if name not in made:
            m = material(name)
            be = hbm.HipBackend(0)
            be.create(m["case"].prob)
            be.set_retro_cap(mv.RETRO_CAP)
            m["case"].begin(be)
            be.set_population(m["S"].pop)
            made[name] = be
        return made[name]

    def run(name, form):
        """-> (out, word, T1, I1) of one launch from the problem's starting tallies; cached"""
        if (name, form) not in runs:
            m, hb = material(name), get(name)
            hb.write_tallies(*m["start"])
            out, word = hb.eval_pass(form, m["S"].helix, pc.I_PCUT)
            T1, I1 = hb.read_tallies()
            runs[(name, form)] = (out, word, T1, I1)
        return runs[(name, form)]
    yield get, run
    for be in made.values():
        be.destroy()
    print("\npass head run; per problem:")
    for key, v in COUNTS.items():
        print("   ", key, v)


def first_bad(bad):
    return int(np.flatnonzero(bad)[0])


def assert_bits(got, want, what, S, mask=None):
    bad = u64(got) != u64(want)
    if mask is not None:
        bad &= mask
    if bad.any():
        k = first_bad(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} states differ, first got {float(got[k]).hex()} want {float(want[k]).hex()}; {pc.describe(S, k)}")


def launch_of(m, name):
    """The oracle's log as a tally_common.Launch (one pass, one record per state) for the per-cell rule"""
    S, p = m["S"], m["S"].pop
    rec = np.zeros((1, S.n, 8))
    rec[0, :, 0], rec[0, :, 2], rec[0, :, 4], rec[0, :, 5], rec[0, :, 6] = p.pb_pf, p.ptot_pf, p.phi_rad, p.weight, p.x_PT_cm
    word = (p.grid.astype(np.uint64) * np.uint64(0x010101) | (p.inj.astype(np.uint64) << np.uint64(24)) | np.uint64(1 << 40)).reshape(1, -1)
    return tc.Launch(name, rec, word, np.arange(S.n).reshape(1, -1), log=m["log"])


def np_L_diff(case, ptot, gam, grt, gd):
    """particle_loop.jl:595-637: the diffusion length of downstream_test, from the given quantities"""
    P = case.prob.params
    m = case.aa * pc.MP
    v_fac = grt * ptot / (m * gam * P.u2)
    if case.aa < 1:
        v_fac = np.where(ptot < P.pe_crit, (P.pe_crit * pc.CC * gd) * P.pe_crit / (m * P.game_crit * P.u2), v_fac)
    return P.eta_mfp / 3 * v_fac


def within_one_ulp(got, x):
    """got is 1/x to within one ulp"""
    q = 1.0 / x
    return (got >= np.nextafter(q, -np.inf)) & (got <= np.nextafter(q, np.inf))


# ---- 1. form 0 against the oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", pc.PROBLEMS)
def test_form0_against_the_oracle(contexts, problem):
    get, run = contexts
    m = material(problem)
    S = m["S"]
    out, word, T1, I1 = run(problem, 0)
    what = f"{problem}, slow_pre"
    for n in pc.OUT:
        if n not in pc.DEVICE_ONLY:
            assert_bits(out[:, COLS[n]], m["out"][:, COLS[n]], f"{what}: {n}", S)
    assert not out[:, COLS["t_hi"]].any() and not out[:, COLS["t_lo"]].any()
    bad = (word & ~pc.DEVICE_BITS) != m["word"]
    assert not bad.any(), (f"{what}: the packed word of {int(bad.sum())} states differs, first {pc.unpack(word[bad][:1])} against the oracle's "
                           f"{pc.unpack(m['word'][bad][:1])}; {pc.describe(S, first_bad(bad))}")
    T0, I0 = m["start"]
    assert np.array_equal(I1, m["end_tallies"][1]), f"{what}: the int64 counters differ from the oracle's"
    e, b = tc.check_launch(get(problem).layout, launch_of(m, what), T0, I0, T1, I1, what)
    w = pc.unpack(m["word"])
    COUNTS[(problem, "form 0")] = dict(states=S.n, ends={int(k): int((w["pre_end"] == k).sum()) for k in np.unique(w["pre_end"])},
                                       histogram_deposits_bit_exact=e, bounded=b)


# ---- 2. laziness: every derived quantity equals the value computed from scratch from the output's own state ---------------------------
@pytest.mark.parametrize("problem", pc.PROBLEMS)
def test_derived_quantities_are_fresh(contexts, problem):
    get, run = contexts
    m = material(problem)
    S, case = m["S"], m["case"]
    P = case.prob.params
    out, word = run(problem, 0)[:2]
    w = pc.unpack(word)
    col = lambda n: out[:, COLS[n]]
    go, sv = w["pre_end"] == pc.GOES_ON, w["pre_end"] == pc.SAVED
    done = go | sv          # the head ran to its end: everything it is lazy about must be up to date
    assert go.sum() > 500 and sv.sum() > 20
    what = f"{problem}, from scratch"
    mass = case.aa * pc.MP
    # the scatter's quantities: orc_eval_scatter's columns on the output's own momenta and field, with the OLD xn_per
    if not P.dont_scatter:
        st = np.zeros((S.n, 10))
        st[:, 2], st[:, 3], st[:, 4], st[:, 5], st[:, 6] = case.aa, col("gyro_denom"), col("ptot_pf"), col("gam_pf"), S.pop.xn_per
        st[:, 7], st[:, 8], st[:, 9] = col("pb_pf"), col("p_perp"), col("phi")
        ob = oracle_backend(case.prob)
        case.begin(ob)
        sc = ob.eval_scatter(st)
        ob.destroy()
        assert_bits(col("gyro_period"), sc[:, 3], f"{what}: gyro_period", S, mask=done)
        assert_bits(col("cm_val"), sc[:, 4], f"{what}: cos_max (with the old xn_per)", S, mask=done)
        ok = within_one_ulp(col("rp_val"), col("ptot_pf"))
        assert ok[done].all(), f"{what}: 1/ptot_pf is stale; {pc.describe(S, first_bad(done & ~ok))}"
    # the move's quantities, with the NEW xn_per
    assert_bits(col("dphi"), pc.TWOPI / col("xn_per"), f"{what}: dphi", S, mask=go)
    assert_bits(col("t_step"), col("gyro_period") / col("xn_per"), f"{what}: t_step", S, mask=go)
    ok = within_one_ulp(col("rg_val"), col("gam_pf") * mass)
    assert ok[go].all(), f"{what}: 1/(gam_pf m) is stale; {pc.describe(S, first_bad(go & ~ok))}"
    want_xn = np.where(col("x") > col("gyro_rad_tot"), P.xn_per_coarse, P.xn_per_fine)
    assert_bits(col("xn_per"), want_xn, f"{what}: xn_per", S, mask=go)
    # downstream_test's threshold, F_SAVE, F_NEARP
    x_dt = mv.np_x_dt(case, col("prp"), np_L_diff(case, col("ptot_pf"), col("gam_pf"), col("gyro_rad_tot"), col("gyro_denom")))
    assert_bits(col("x_dt"), x_dt, f"{what}: x_dt", S, mask=done)
    f_save = (w["downstream"] != 0) & (col("ptot_pf") > case.prob.pcuts[pc.I_PCUT - 1])
    f_nearp = col("ptot_pf") > pc.pmax_of(case)
    assert np.array_equal((w["f_save"] != 0)[done], f_save[done]), f"{what}: F_SAVE is not its predicate"
    assert np.array_equal((w["f_nearp"] != 0)[done], f_nearp[done]), f"{what}: F_NEARP is not its predicate"
    # the gyroradii, where the head changed the momentum through its loss or its frame change (the reference recomputes them there;
    # a change of the field alone, or an energy transfer, leaves them as they are in the reference too)
    lossy = bool(P.do_rad_losses) and case.aa < 1
    changed = done if lossy else done & (u64(col("ptot_pf")) != u64(m["pre"][:, COLS["ptot_pf"]])) & ~m["np"]["etf"]
    assert changed.sum() > 100
    assert_bits(col("gyro_rad_tot"), col("ptot_pf") * pc.CC * col("gyro_denom"), f"{what}: gyro_rad_tot", S, mask=changed)
    assert_bits(col("gyro_rad"), col("p_perp") * pc.CC * col("gyro_denom"), f"{what}: gyro_rad", S, mask=changed & go)
    gd, _ = pc.np_gyro_denom(case, w["i_grid"], col("x"))
    assert_bits(col("gyro_denom"), gd, f"{what}: gyro_denom", S, mask=done)
    # the zone cache is the table's entry of the zone the particle is in
    tb = mv.tables(case)
    for n, tab in (("z_lo", tb.xg[w["i_grid"]]), ("z_hi", tb.xg[w["i_grid"] + 1]), ("z_ux", tb.ux[w["i_grid"]]), ("z_gsf", tb.gsf[w["i_grid"]]),
                   ("z_gef", tb.gef[w["i_grid"]])):
        assert_bits(col(n), tab, f"{what}: {n}", S, mask=done)
    assert np.array_equal(w["ig3"][done], w["i_grid"][done])
    COUNTS[(problem, "fresh")] = dict(went_on=int(go.sum()), saved=int(sv.sum()), momentum_changed=int(changed.sum()), near_pmax=int(f_nearp[done].sum()))


# ---- 3. the LOSSY kernel's in-line loss against slow_pre ---------------------------------------------------------------------------
@pytest.mark.parametrize("problem", pc.LOSSY)
def test_inline_loss_against_slow_pre(contexts, problem):
    get, run = contexts
    m = material(problem)
    S, pop, case = m["S"], m["S"].pop, m["case"]
    P = case.prob.params
    out0, word0 = run(problem, 0)[:2]
    out1, word1 = run(problem, 1)[:2]
    w0, w1 = pc.unpack(word0), pc.unpack(word1)
    # what the in-line path is entitled to: the move left nothing due (no position event but the fine / coarse switch, which that kernel
    # decides in line; no clock event; not the cap) and no flag is pending (not near p_max, not to be saved, no inj check)
    d = mv.np_derive(case, pop)
    gam_in = d["gam"]
    d["period"] = pc.np_period(case, np.asarray(pop.ptot_pf), gam_in, d["gd"])
    ev = mv.np_events(case, pop, out0[:, COLS["x_old"]], out0[:, COLS["x"]], d)
    nt = len(case.prob.tcuts)
    t_next = np.where(pop.tcut <= nt, np.asarray(case.prob.tcuts)[np.minimum(pop.tcut, nt) - 1], np.inf) if nt else np.full(S.n, np.inf)
    t_ev = np.minimum(t_next, P.age_max) if P.age_max > 0 else t_next
    clock = (pop.downstream != 0) & (pop.acctime_sec >= t_ev)
    flags = (pop.ptot_pf > pc.pmax_of(case)) | ((pop.downstream != 0) & (pop.ptot_pf > case.prob.pcuts[pc.I_PCUT - 1]))
    flags |= (pop.downstream != 0) & (pop.inj == 0) & (pop.x_PT_cm < 0)
    calm = ~mv.np_due(ev, no_xn=True) & ~clock & ~flags & (S.helix < pc.HELIX_CAP) & (w0["post_end"] == 7) & (w0["pre_end"] != pc.NOT_RUN)
    calm &= w0["draws"] == 0
    # (and the reference lets the particle go on: an input the head ends with nothing due after its move -- injected and already beyond
    # the upstream FEB, or older than age_max upstream -- is no state a live lane holds)
    calm &= pc.unpack(m["word"])["pre_end"] == pc.GOES_ON
    loss = S.cls == "loss"
    assert calm[loss].mean() >= 0.5, f"{problem}: the in-line path is entitled to {calm[loss].mean():.0%} of the loss class"
    assert calm.sum() > 1500
    what = f"{problem}, in-line loss against slow_pre"
    for n in pc.OUT:
        if n not in ("t_hi", "t_lo"):
            assert_bits(out1[:, COLS[n]], out0[:, COLS[n]], f"{what}: {n}", S, mask=calm)
    bad = calm & (word1 != word0)
    assert not bad.any(), f"{what}: the packed word differs: {pc.unpack(word1[bad][:1])} against {pc.unpack(word0[bad][:1])}; {pc.describe(S, first_bad(bad))}"
    assert np.all(w0["pre_end"][calm] == pc.GOES_ON)
    # the thresholds it leaves are the table's, for the state it leaves
    col = lambda n: out1[:, COLS[n]]
    after = SimpleNamespace(n=S.n, grid=w1["i_grid"], prp_x_cm=col("prp"), inj=w1["inj"], xn_per=col("xn_per"))
    d1 = dict(L_diff=np_L_diff(case, col("ptot_pf"), col("gam_pf"), col("gyro_rad_tot"), col("gyro_denom")), grt=col("gyro_rad_tot"))
    hi, lo, _ = mv.np_thresholds(case, after, col("x"), d1, no_xn=True)
    assert_bits(col("t_hi"), hi, f"{what}: t_hi", S, mask=calm)
    assert_bits(col("t_lo"), lo, f"{what}: t_lo", S, mask=calm)
    COUNTS[(problem, "form 1")] = dict(entitled=int(calm.sum()), of_the_loss_class=f"{calm[loss].mean():.0%}",
                                       dlnp_above=int((calm & (m["np"]["dlnp"] > 1e-2)).sum()), dlnp_below=int((calm & (m["np"]["dlnp"] <= 1e-2)).sum()))
    assert (calm & (m["np"]["dlnp"] > 1e-2)).sum() > 5 and (calm & (m["np"]["dlnp"] <= 1e-2)).sum() > 5


# ---- 4. read-only inputs, refusals --------------------------------------------------------------------------------------------------
def test_inputs_are_only_read_and_refusals(contexts):
    get, run = contexts
    hb = get("electrons")
    m = material("electrons")
    S = m["S"]
    saved0, l_save0 = hb.get_saved()
    before = [run("electrons", f) for f in (0, 1)]
    pop_after = hb.get_population()
    for f in pop_after.fields():
        assert np.array_equal(getattr(pop_after, f), getattr(S.pop, f)), f"the population's {f} was written"
    saved1, l_save1 = hb.get_saved()
    assert np.array_equal(l_save0, l_save1)
    for f in saved1.fields():
        assert np.array_equal(u64(getattr(saved0, f)) if getattr(saved0, f).dtype == np.float64 else getattr(saved0, f),
                              u64(getattr(saved1, f)) if getattr(saved1, f).dtype == np.float64 else getattr(saved1, f)), f"the saved array {f} was written"
    hx = np.array(S.helix)
    for form, i_pcut, msg in ((2, 1, "unknown form"), (-1, 1, "unknown form"), (0, 0, "i_pcut outside"), (0, len(m["case"].prob.pcuts) + 1, "i_pcut outside")):
        with pytest.raises(RuntimeError, match=msg):
            hb.eval_pass(form, hx, i_pcut)
    for v in (0, -1, 16001):
        bad = hx.copy(); bad[S.n // 2] = v
        with pytest.raises(RuntimeError, match="helix"):
            hb.eval_pass(0, bad, 1)
    with pytest.raises(RuntimeError, match="form 1 is the LOSSY kernel's"):
        get("protons").eval_pass(1, np.array(material("protons")["S"].helix), 1)
    with pytest.raises(RuntimeError, match="form 1 is the LOSSY kernel's"):
        get("electrons_epsB").eval_pass(1, np.array(material("electrons_epsB")["S"].helix), 1)
    # ... and after all the refused calls the context computes as before
    hb.write_tallies(*m["start"])
    out, word = hb.eval_pass(0, S.helix, pc.I_PCUT)
    T1, I1 = hb.read_tallies()
    assert np.array_equal(u64(out), u64(before[0][0])) and np.array_equal(word, before[0][1]) and np.array_equal(I1, before[0][3])


def test_regressions(contexts):
    for name, (problem, fields, helix) in REGRESSIONS.items():
        case = material(problem)["case"]
        n = len(helix)
        pop = mcs.capi.Population(n)
        for f, vals in fields.items():
            getattr(pop, f)[:] = [float.fromhex(v) if isinstance(v, str) else v for v in vals]
        S = pc.States(pop, np.array(helix, dtype=np.int32), np.full(n, "regression"), np.full(n, np.nan))
        m = pc.reference(case, S)
        from mcs_amd import hip_backend as hbm
        hb = hbm.HipBackend(0)
        hb.create(case.prob)
        hb.set_retro_cap(mv.RETRO_CAP)
        case.begin(hb)
        hb.set_population(pop)
        hb.write_tallies(*m["start"])
        out, word = hb.eval_pass(0, S.helix, pc.I_PCUT)
        for c in pc.OUT:
            if c not in pc.DEVICE_ONLY:
                assert_bits(out[:, COLS[c]], m["out"][:, COLS[c]], f"regression '{name}': {c}", S)
        assert np.array_equal(word & ~pc.DEVICE_BITS, m["word"])
        hb.destroy()
