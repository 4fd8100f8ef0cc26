"""The move of Code Block 2 and the decision what that move triggers, state by state, on a real MI355X.

mcs_eval_move (include/mcs.h) runs one state per thread through the transport kernel's own load_particle, refresh_move / refresh_time /
refresh_dtest, one of the four spellings of the move (move_and_detect; refresh_thr + move_and_detect_thr; the same with the tail loop's
literals; the lossy kernel's thresholds) and then slow_post or plain_crossing, in the translation unit they ship in.  The references
are orc_eval_move -- the oracle's Code Block 2, the function its particle_loop calls -- with its deposit log, and the numpy
restatement of tests/move_common.py (the events due, the zone search, the table of the thresholds), which the host tests check
against each other.  The states put x_new within an ulp of every zone edge, of x_grid_stop, the PRP, 1.1 prp, 6.91 L_diff, the
downstream FEB, gyro_rad_tot and the upstream FEB, and on them; see move_common for the classes.

Every comparison is bit equality, except the tally cells with several terms (tally_common.check_launch: the a-priori bound of a sum
in any order).  Nothing is filtered out of an assertion: a state outside an assertion's domain is named by a mask whose size is
asserted.  Outside this test: the inline dispatch of the rare region (full / light path / waiting) in transport_body,
mcs_transport_ws.inc and the tail loop (calling it from a test kernel needs a refactor of the body: a pull request of its own, with a
bench), the fp32 kernels, and the electrons' helix_count % 1000 branch of prob_return (a state is a particle's first pass).

Regression cases found with these tests keep their states in REGRESSIONS below (none so far)."""
import ctypes as ct
import functools

import numpy as np
import pytest

from conftest import mcs, oracle_backend
import move_common as mv
import tally_common as tc

pytestmark = pytest.mark.gpu

u64 = mv.u64
COUNTS = {}
REGRESSIONS = {}             # name -> (problem, {field: [hex floats / ints]}, x_thr as hex floats): states that once differed, run by test_regressions
COLS = {n: i for i, n in enumerate(mv.OUT)}
STATE = [COLS[n] for n in mv.OUT if n not in ("t_hi", "t_lo")]        # what the oracle has too


@functools.lru_cache(maxsize=None)
def material(name):
    """The states of one problem and every reference, built once and never changed."""
    case = mv.make_case(name)
    S = mv.build_states(case)
    return reference(case, S)


def reference(case, S):
    x_new, phi_new = mv.first_move(case, S.pop)
    ob = oracle_backend(case.prob)
    case.begin(ob)
    ob.set_retro_cap(mv.RETRO_CAP)
    start = ob.read_tallies()              # a fresh context after begin_iteration / begin_species: where every launch starts
    out, word, log = ob.eval_move(S.pop, mv.I_PCUT)
    ob.destroy()
    d = mv.np_derive(case, S.pop)
    ev = mv.np_events(case, S.pop, S.pop.x_PT_cm, x_new, d)
    m = dict(case=case, S=S, x_new=x_new, phi_new=phi_new, out=out, word=word, log=log, d=d, ev=ev, start=start,
             found=mv.np_zone_search(mv.tables(case).xg, x_new, x_new > S.pop.x_PT_cm, S.pop.grid))
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return m


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

    def run(name, form, post, own_thr=False):
        """-> (out, word, T1, I1) of one launch from the fresh tallies; cached.  own_thr: x_thr = x for every state."""
        key = (name, form, post, own_thr)
        if key not in runs:
            m, hb = material(name), get(name)
            T0, I0 = m["start"]
            hb.write_tallies(T0, I0)
            out, word = hb.eval_move(form, post, mv.I_PCUT, None if form == 0 else (m["S"].pop.x_PT_cm if own_thr else m["S"].x_thr))
            T1, I1 = hb.read_tallies()
            runs[key] = (out, word, T1, I1)
        return runs[key]
    yield get, run
    for be in made.values():
        be.destroy()
    print("\nmove events run; per problem: states per class, and the stops of forms 1-3 with nothing due, by the table's reason:")
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
        raise AssertionError(f"{what}: {int(bad.sum())} states differ, first got {float(got[k]).hex()} want {float(want[k]).hex()}; {mv.describe(S, k)}")


def launch_of(m, log, name):
    """The oracle's log as a tally_common.Launch (one pass, one record per state) for the per-cell rule"""
    S, p = m["S"], m["S"].pop
    rec = np.zeros((1, S.n, 8))
    rec[0, :, 0], rec[0, :, 2], rec[0, :, 4], rec[0, :, 5], rec[0, :, 6] = p.pb_pf, p.ptot_pf, p.phi_rad, p.weight, p.x_PT_cm
    word = (p.grid.astype(np.uint64) * np.uint64(0x010101) | (p.inj.astype(np.uint64) << np.uint64(24)) | np.uint64(1 << 40)).reshape(1, -1)
    return tc.Launch(name, rec, word, np.arange(S.n).reshape(1, -1), log=log)


# ---- 1. the move -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", mv.PROBLEMS)
def test_the_four_spellings_of_the_move(contexts, problem):
    get, run = contexts
    m = material(problem)
    S, pop, case = m["S"], m["S"].pop, m["case"]
    P = case.prob.params
    assert np.all(np.abs(pop.phi_rad + mv.TWOPI / pop.xn_per) < 1e5)            # the domain of mod2pi_k: all of the inputs
    T0, I0 = m["start"]
    for form in (0, 1, 2, 3):
        out, word, T1, I1 = run(problem, form, 0)
        what = f"{problem}, form {form}"
        assert_bits(out[:, COLS["x"]], m["x_new"], what + ": x", S)
        assert_bits(out[:, COLS["x_old"]], pop.x_PT_cm, what + ": x_old", S)
        assert_bits(out[:, COLS["phi"]], m["phi_new"], what + ": phi", S)
        assert_bits(out[:, COLS["gam_pf"]], m["d"]["gam"], what + ": gam_pf", S)
        assert np.array_equal(u64(T1), u64(T0)) and np.array_equal(I1, I0), what + ": a move alone changed a tally"
        w = mv.unpack(word)
        assert np.all(w["end"] == mv.GOES_ON) and not w["npush"].any() and not w["draws"].any() and not w["plain"].any()
        # the thresholds and x_dt against the table, bit for bit
        x_dt = mv.np_x_dt(case, pop.prp_x_cm, m["d"]["L_diff"])
        assert_bits(out[:, COLS["x_dt"]], x_dt, what + ": x_dt", S)
        if form:
            hi, lo, _ = mv.np_thresholds(case, pop, S.x_thr, m["d"], no_xn=form == 3)
            assert_bits(out[:, COLS["t_hi"]], hi, what + ": t_hi", S)
            assert_bits(out[:, COLS["t_lo"]], lo, what + ": t_lo", S)
    # against the oracle: its x is the first move's wherever it drew no random number (no retry of no_DSA_loop, no PRP return)
    wo = mv.unpack(m["word"])
    calm = wo["draws"] == 0
    assert calm.mean() > 0.9
    out0 = run(problem, 0, 0)[0]
    for n in ("x", "x_old", "phi"):
        assert_bits(out0[:, COLS[n]], m["out"][:, COLS[n]], f"{problem}: {n} against the oracle", S, mask=calm if n != "x_old" else None)


# ---- 2. nothing is missed, 3. nothing spurious beyond the contract ------------------------------------------------------------------
@pytest.mark.parametrize("problem", mv.PROBLEMS)
def test_nothing_due_is_missed(contexts, problem):
    get, run = contexts
    m = material(problem)
    S, ev = m["S"], m["ev"]
    # form 0, the exact one: ev | ev_cross is the numpy statement, ev_cross is "left the zone"
    w = mv.unpack(run(problem, 0, 0)[1])
    exact = ev["left"] | ev["stop"] | ev["prp"] | ev["dtest"] | ev["xn"] | ev["odd"]
    got = (w["ev"] | w["ev_cross"]) != 0
    assert np.array_equal(w["ev_cross"] != 0, ev["left"]), f"{problem}: ev_cross of move_and_detect is not 'left the zone'; {mv.describe(S, first_bad((w['ev_cross'] != 0) != ev['left']))}"
    assert np.array_equal(got, exact), f"{problem}: move_and_detect reports {int((got & ~exact).sum())} events that are not due and misses {int((exact & ~got).sum())}; {mv.describe(S, first_bad(got != exact))}"
    for name in ("left", "stop", "prp", "dtest", "xn"):
        assert ev[name].sum() > 20, f"{problem}: only {int(ev[name].sum())} states with the event '{name}'"
    assert ev["feb"].sum() > 5
    # forms 1-3: whatever is due is reported, by a threshold or by the event bit
    for form in (1, 2, 3):
        for own in (False, True):
            w = mv.unpack(run(problem, form, 0, own)[1])
            # (the thresholds promise nothing for a position no lane leaves the rare region alive at -- an injected particle beyond the
            # upstream FEB, a position beyond x_dt, the other step size: the contract's domain, whose size is asserted)
            dom = mv.contract_domain(m["case"], S.pop, S.pop.x_PT_cm if own else S.x_thr, m["d"])
            assert (~dom).sum() < 0.1 * S.n
            due = mv.np_due(ev, no_xn=form == 3) & dom
            missed = due & ((w["ev"] | w["ev_cross"]) == 0)
            assert not missed.any(), f"{problem}, form {form}: {int(missed.sum())} events missed, first {mv.describe(S, first_bad(missed))}"
            assert np.array_equal(w["ev"] != 0, ev["odd"]), f"{problem}, form {form}: the event bit is not the odd configurations' own"


@pytest.mark.parametrize("problem", mv.PROBLEMS)
def test_nothing_spurious_beyond_the_contract(contexts, problem):
    get, run = contexts
    m = material(problem)
    S, ev, case = m["S"], m["ev"], m["case"]
    dom = mv.contract_domain(case, S.pop, S.x_thr, m["d"])
    crafted = S.cls != "fuzz"
    assert dom[crafted].mean() >= 0.9 and (~dom).sum() < 0.1 * S.n, f"{problem}: {int((~dom).sum())} of {S.n} states outside the thresholds' contract"
    counts = {c: int((S.cls == c).sum()) for c in np.unique(S.cls)}
    for form in (1, 2, 3):
        w = mv.unpack(run(problem, form, 0)[1])
        no_xn = form == 3
        spurious = (w["ev_cross"] != 0) & ~mv.np_due(ev, no_xn) & dom
        cat = mv.np_spurious(case, S.pop, S.x_thr, m["x_new"], m["d"], no_xn)
        allowed = cat["boundary"] | cat["rearm"] | cat["beyond_dt"] | cat["prp_below"]
        assert not (spurious & ~allowed).any(), f"{problem}, form {form}: a stop with nothing due that the table does not allow: {mv.describe(S, first_bad(spurious & ~allowed))}"
        assert sum(int((spurious & v).sum()) for v in cat.values()) == int(spurious.sum())          # exactly one reason each
        counts[f"form {form} stops with nothing due"] = {k: int((spurious & v).sum()) for k, v in cat.items()}
    COUNTS[problem] = counts


# ---- 4. slow_post -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("post", (1, 2))
@pytest.mark.parametrize("problem", mv.PROBLEMS)
def test_slow_post_against_the_oracle(contexts, problem, post):
    get, run = contexts
    m = material(problem)
    S = m["S"]
    out, word, T1, I1 = run(problem, 0, post)
    what = f"{problem}, slow_post<{'true' if post == 2 else 'false'}>"
    for n in mv.OUT:
        if n not in ("t_hi", "t_lo"):
            assert_bits(out[:, COLS[n]], m["out"][:, COLS[n]], f"{what}: {n}", S)
    keep = ~(mv.DEVICE_BITS | (mv.NPUSH_BITS if post == 2 else np.uint64(0)))
    bad = (word & keep) != (m["word"] & keep)
    assert not bad.any(), (f"{what}: the packed word of {int(bad.sum())} states differs, first {mv.unpack(word[bad][:1])} against the oracle's "
                           f"{mv.unpack(m['word'][bad][:1])}; {mv.describe(S, first_bad(bad))}")
    if post == 2:
        assert not mv.unpack(word)["npush"].any()
    T0, I0 = m["start"]
    e, b = tc.check_launch(get(problem).layout, launch_of(m, m["log"], what), T0, I0, T1, I1, what)
    wo = mv.unpack(m["word"])
    assert (wo["end"] == 1).sum() > 50 and (wo["end"] == 3).sum() >= 1 and (wo["n_retro"] > 0).sum() >= (0 if m["case"].prob.params.feb_downstream > 0 else 20)
    COUNTS[(problem, f"post {post}")] = dict(histogram_deposits_bit_exact=e, bounded=b, ended=int((wo["end"] != mv.GOES_ON).sum()),
                                             prp_returns=int((wo["n_retro"] > 0).sum()))


@pytest.mark.parametrize("problem", mv.PROBLEMS)
def test_pushed_and_direct_slow_post_agree(contexts, problem):
    get, run = contexts
    S = material(problem)["S"]
    a, b = run(problem, 0, 1), run(problem, 0, 2)
    for n in mv.OUT:
        assert_bits(a[0][:, COLS[n]], b[0][:, COLS[n]], f"{problem}: {n} of slow_post<false> against slow_post<true>", S)
    assert np.array_equal(a[1] & ~mv.NPUSH_BITS, b[1] & ~mv.NPUSH_BITS)
    assert np.array_equal(a[3], b[3])


# ---- 5. plain_crossing --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("post", (3, 4))
@pytest.mark.parametrize("problem", mv.PROBLEMS)
def test_plain_crossing(contexts, problem, post):
    get, run = contexts
    m = material(problem)
    S, pop, case, ev, found = m["S"], m["S"].pop, m["case"], m["ev"], m["found"]
    P, tb = case.prob.params, mv.tables(case)
    out, word, T1, I1 = run(problem, 0, post)
    out0, word0 = run(problem, 0, 0)[:2]
    what = f"{problem}, plain_crossing<{'true' if post == 4 else 'false'}>"
    w = mv.unpack(word)
    # the numpy predicate.  plain_crossing is called for a move that left its zone: that is its domain (of a move that stayed it says
    # "crossed into the neighbour", by construction: it looks at the neighbour's FAR edge only)
    x_old, x_new = pop.x_PT_cm, m["x_new"]
    left = ev["left"]
    assert 0.3 * S.n < left.sum() < 0.9 * S.n
    shock = (x_old < 0) & (x_new >= 0)
    tgt = np.maximum(found, 0)
    gd_tgt = 1 / (case.zz * mv.QCGS * tb.bt[tgt])
    want = left & ~shock & (found >= 0) & (found > P.i_grid_feb) & (tb.ux[tgt] == tb.ux[pop.grid]) & (gd_tgt == m["d"]["gd"])
    got = w["plain"] != 0
    bad = left & (got != want)
    assert not bad.any(), f"{what}: returns {bool(got[first_bad(bad)])} where the predicate says {bool(want[first_bad(bad)])}; {mv.describe(S, first_bad(bad))}"
    assert (want & left).sum() > 100 and (left & ~want).sum() > 100
    if problem == "oblique":
        assert (left & ~shock & (found > P.i_grid_feb) & (tb.ux[tgt] != tb.ux[pop.grid])).sum() > 20        # refused for the flow speed alone
    if problem == "epsB":
        assert (left & ~shock & (found > P.i_grid_feb) & (tb.ux[tgt] == tb.ux[pop.grid]) & (gd_tgt != m["d"]["gd"])).sum() > 0        # ... for the field alone
    # where false (or outside the domain and false): nothing changed
    same = ~got
    for n in mv.OUT:
        assert_bits(out[:, COLS[n]], out0[:, COLS[n]], f"{what} returned false: {n}", S, mask=same)
    plain_bits = np.uint64(1 << 42) | mv.NPUSH_BITS
    assert np.array_equal((word & ~plain_bits)[same], (word0 & ~plain_bits)[same]) and not w["npush"][same].any()
    # where true, inside the domain: what slow_post does, followed by the zone reload of the next Code Block 3
    yes = got & left
    w1 = mv.unpack(run(problem, 0, 1)[1])
    # (a retry of no_DSA_loop moves the particle again, and slow_post's zone is then another: a move from a downstream zone onto
    # x = 0 exactly, not injected, where inj_frac < 1 -- a handful of states)
    again = yes & ev["reflect"]
    assert again.sum() <= 10
    for n in ("i_grid", "i_grid_old", "inj"):
        assert np.array_equal(w[n][yes & ~again], w1[n][yes & ~again]), f"{what}: {n} differs from slow_post's"
    assert np.array_equal(w["inj"][yes] != 0, ((pop.inj != 0) | ((pop.downstream != 0) & (x_new < 0)))[yes])
    assert np.array_equal(w["ig3"][yes], w["i_grid"][yes]) and np.array_equal(w["i_grid"][yes], found[yes])
    new = w["i_grid"]
    for n, tab in (("z_lo", tb.xg[new]), ("z_hi", tb.xg[new + 1]), ("z_ux", tb.ux[new]), ("z_gsf", tb.gsf[new]), ("z_gef", tb.gef[new])):
        assert_bits(out[:, COLS[n]], tab, f"{what} returned true: {n} is not the table's value at the new zone", S, mask=yes)
    z_bcos_of = {}
    out1 = run(problem, 0, 0)[0]                      # (the kernel's own cos theta_B per zone: every zone is some state's ig3)
    for g, c in zip(pop.grid, out1[:, COLS["z_bcos"]]):
        z_bcos_of.setdefault(int(g), c)
    have = yes & np.isin(new, list(z_bcos_of))
    assert have.sum() >= 0.9 * yes.sum()
    assert_bits(out[:, COLS["z_bcos"]], np.array([z_bcos_of.get(int(g), np.nan) for g in new]), f"{what} returned true: z_bcos", S, mask=have)
    for n in ("x", "x_old", "phi", "pb_pf", "p_perp", "ptot_pf", "gam_pf", "prp", "acctime", "x_dt"):
        assert_bits(out[:, COLS[n]], out0[:, COLS[n]], f"{what} returned true: {n} changed", S, mask=yes)
    assert np.array_equal(w["npush"][yes], np.full(int(yes.sum()), 1 if post == 3 else 0))
    # its record is slow_post's: the state the move left, the zones (i_grid_old, found], inj as above -- walked through the oracle's
    # all_flux! tally (orc_eval_tally: the reference of test_gpu_tally_records.py), and the per-cell rule over the whole buffers
    rec = np.zeros((1, S.n, 8))
    for j, n in enumerate(("pb_pf", "p_perp", "ptot_pf", "gam_pf", "phi")):
        rec[0, :, j] = out0[:, COLS[n]]
    rec[0, :, 5], rec[0, :, 6], rec[0, :, 7] = pop.weight, x_new, x_old
    # (every state it returned true for, those outside its domain too: the whole buffers are compared, and there it "crossed" into
    # the neighbour -- the zone its word names)
    wordr = np.where(got, w["i_grid"].astype(np.uint64) | (pop.grid.astype(np.uint64) << np.uint64(8)) | (pop.grid.astype(np.uint64) << np.uint64(16))
                     | (w["inj"].astype(np.uint64) << np.uint64(24)) | np.uint64(tc.KIND_CROSS << 40), np.uint64(0)).reshape(1, -1)
    ob = oracle_backend(case.prob)
    case.begin(ob)
    log = ob.eval_tally(rec, wordr)
    ob.destroy()
    T0, I0 = m["start"]
    tc.check_launch(get(problem).layout, tc.Launch(what, rec, wordr, np.arange(S.n).reshape(1, -1), log=log), T0, I0, T1, I1, what)
    COUNTS[(problem, f"post {post}")] = dict(left=int(left.sum()), plain=int(yes.sum()), refused=int((left & ~got).sum()), outside_domain=int((~left).sum()))


# ---- refusals, regressions ----------------------------------------------------------------------------------------------------------
def test_refusals(contexts):
    """Everything mcs_eval_move refuses, with its message, and the context afterwards computes what it computed before."""
    get, run = contexts
    hb = get("protons")
    m = material("protons")
    n = m["S"].n
    before = run("protons", 0, 1)
    thr = np.ascontiguousarray(m["S"].x_thr)
    for form, post, i_pcut, msg in ((4, 0, 1, "unknown form"), (-1, 0, 1, "unknown form"), (0, 5, 1, "unknown post"), (0, -1, 1, "unknown post"),
                                    (0, 0, 0, "i_pcut outside"), (0, 0, len(m["case"].prob.pcuts) + 1, "i_pcut outside")):
        with pytest.raises(RuntimeError, match=msg):
            hb.eval_move(form, post, i_pcut, thr)
    bad = thr.copy(); bad[n // 2] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        hb.eval_move(1, 0, 1, bad)
    dp, up64 = ct.POINTER(ct.c_double), ct.POINTER(ct.c_uint64)
    out, word = np.zeros((n, 18)), np.zeros(n, dtype=np.uint64)
    o, wd, t = out.ctypes.data_as(dp), word.ctypes.data_as(up64), thr.ctypes.data_as(dp)
    lib = hb.lib
    assert lib.mcs_eval_move(hb.h, 0, 0, 1, n, t, None, wd) != 0 and b"null argument" in lib.mcs_last_error()
    assert lib.mcs_eval_move(hb.h, 0, 0, 1, n, t, o, None) != 0 and b"null argument" in lib.mcs_last_error()
    assert lib.mcs_eval_move(hb.h, 1, 0, 1, n, None, o, wd) != 0 and b"null argument" in lib.mcs_last_error()
    assert lib.mcs_eval_move(hb.h, 0, 0, 1, -1, t, o, wd) != 0 and b"negative" in lib.mcs_last_error()
    assert lib.mcs_eval_move(hb.h, 0, 0, 1, n - 1, t, o, wd) != 0 and b"not the size" in lib.mcs_last_error()
    assert lib.mcs_eval_move(None, 0, 0, 1, n, t, o, wd) != 0 and b"null context" in lib.mcs_last_error()
    assert not out.any() and not word.any()
    from mcs_amd import hip_backend as hbm
    f32 = hbm.HipBackend(0)
    f32.create(mcs.inputs.build_problem(mcs.inputs.Config(N_PTS_INJ=64, N_PTS_PCUT=64, N_PTS_PCUT_HI=64, state_fp32=True)))
    m["case"].begin(f32)
    with pytest.raises(RuntimeError, match="fp32 state"):
        f32.eval_move(0, 0, 1)
    f32.destroy()
    # ... and after all the refused calls the context computes as before
    T0, I0 = m["start"]
    hb.write_tallies(T0, I0)
    out, word = hb.eval_move(0, 1, mv.I_PCUT)
    T1, I1 = hb.read_tallies()
    assert np.array_equal(u64(out), u64(before[0])) and np.array_equal(word, before[1]) and np.array_equal(I1, before[3])
    pop_after = hb.get_population()
    for f in pop_after.fields():
        assert np.array_equal(getattr(pop_after, f), getattr(m["S"].pop, f)), f"the population's {f} was written"


def test_regressions(contexts):
    get, run = contexts
    for name, (problem, fields, thr) in REGRESSIONS.items():
        case = material(problem)["case"]
        n = len(thr)
        pop = mcs.capi.Population(n)
        for f, vals in fields.items():
            getattr(pop, f)[:] = [float.fromhex(v) if isinstance(v, str) else v for v in vals]
        S = mv.States(pop, np.array([float.fromhex(v) for v in thr]), np.full(n, "regression"), np.full(n, np.nan))
        m = reference(case, S)
        from mcs_amd import hip_backend as hbm
        hb = hbm.HipBackend(0)
        hb.create(case.prob)
        hb.set_retro_cap(mv.RETRO_CAP)
        case.begin(hb)
        hb.set_population(pop)
        for post in (1, 2):
            hb.write_tallies(*m["start"])
            out, word = hb.eval_move(0, post, mv.I_PCUT)
            for c in STATE:
                assert_bits(out[:, c], m["out"][:, c], f"regression '{name}', post {post}: {mv.OUT[c]}", S)
            keep = ~(mv.DEVICE_BITS | (mv.NPUSH_BITS if post == 2 else np.uint64(0)))
            assert np.array_equal(word & keep, m["word"] & keep)
        hb.destroy()
