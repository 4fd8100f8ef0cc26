"""States for mcs_eval_move / orc_eval_move: one move of Code Block 2 per state, and what that move triggers.

A state is a row of a population as the move sees it, AFTER the scatter and the clock of a pass: weight, ptot_pf, pb_pf, x, xn_per, prp,
acctime, phi, grid, tcut, downstream, inj; and x_thr, the position at which forms 1-3 of mcs_eval_move compute the two thresholds of the
common pass (x_thr = x: the ordinary case).  build_states() crafts them, per problem, around every number a move can reach:

    edge          every zone edge x_grid[1 .. n_grid]; the sentinels x_grid[0] and x_grid[n_grid + 1] are the `off_grid` class
    x_grid_stop, prp_lo / prp_hi (the PRP below and above x_grid_stop), prp11 (1.1 prp), ldiff (6.91 L_diff), feb_down (where set),
    grt_fine / grt_coarse (gyro_rad_tot with either step size), feb_up (zones up to i_grid_feb, with and without inj),
    shock         0 from both sides, x exactly +-0.0, and x_old > 0 >= x with inj clear (the retry loop of no_DSA_loop where inj_frac < 1)
    jump          moves over 1, 2, 3, 4 and dozens of zones in both directions, landing inside a zone and exactly on an edge
    off_grid      moves beyond either end of the grid (end code 3), and onto the sentinels themselves
    rearm_down / rearm_up   x_thr on one side of x_grid_stop / prp / gyro_rad_tot, x between x_thr and the boundary (strictly inside
                  the thresholds of x_thr), the move across the boundary
    prp_return    PRP crossings beyond x_grid_stop with vt < u2, vt just above u2, and momenta whose returns start the retro walk
    tcut          acctime one ulp below, on and one ulp above the next cut, the index beyond the last cut, age_max
    fuzz          2000 states of conftest.fuzz_population as background

For a target T the builder wants x_new = x + dx on T: for a parallel field dx = gsf (pb t_step / (gam m) b_cos + ux t_step) does not
depend on x, so x = T - dx, corrected once by the first move's own error and then walked over +-3 ulps; pb_pf is either a plain
fraction of ptot_pf (both signs) or solved so that |dx| is an eighth of |T|, which keeps x in T's binade and lets x_new land ON T.
Classification always uses the computed x_new (first_move), never the intended one, and check_states() asserts that every target
class has states below, on and above its target.

np_* below are a numpy restatement of the reference's statements (particle_loop.jl prologue and Code Block 2, all_flux.jl:64-82,
particle_loop.jl:595-637, prob_return.jl:73,89) and of the table in the comment above refresh_thr (csrc/mcs_transport.hip); they share
no code with oracle/mcs_oracle.cpp (gam_pf and mod2pi come through orc_eval_fn).  The move itself is restated for parallel fields
only: with an oblique field the gyro term needs the library's cos, and first_move() then asks the oracle.

Not reached here, on purpose: prob_return's `helix_count % 1000 == 0` branch of the electrons (a state is a particle's first pass,
helix_count 1: mcs_eval_pass takes the count from the caller, and tests/pass_common.py builds electrons beyond x_grid_stop with 999, 1000 and
2000 passes behind them), and the inline dispatch of the rare region (full / light path / waiting) in transport_body, mcs_transport_ws.inc and the tail loop -- calling that from a test kernel needs a refactor of the body, which is a
pull request of its own, with a bench.  The fp32 kernels keep their whole-run check.
"""
import ctypes as ct
from dataclasses import dataclass

import numpy as np

from conftest import mcs, make_problem, fuzz_problem, fuzz_population
import orc
import tally_common as tc

MP, CC, QCGS = tc.MP, tc.CC, tc.QCGS
TWOPI = 6.283185307179586
PROBLEMS = ("protons", "general", "electrons", "oblique", "epsB", "xspec")
I_PCUT = 3                   # the launch constants are those of this pcut: pcut_prev = pcuts[1]
RETRO_CAP = 20000            # both backends: bounds the retro walk of a fuzzed state
N_FUZZ = 2000
OUT = ("x", "x_old", "phi", "pb_pf", "p_perp", "ptot_pf", "gam_pf", "prp", "acctime", "t_hi", "t_lo", "x_dt", "z_lo", "z_hi", "z_ux",
       "z_gsf", "z_bcos", "z_gef")
# classes whose states aim at a number: check_states() asserts below / on / above for each
TARGET_CLASSES = ("edge", "x_grid_stop", "prp_lo", "prp_hi", "prp11", "ldiff", "feb_down", "grt_fine", "grt_coarse", "feb_up", "shock")


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_LIB = None


def oev(fn, a):
    """orc_eval_fn: the oracle's own hypot1 / mod2pi, the two functions of the move that are no IEEE operation"""
    global _LIB
    if _LIB is None:
        _LIB = orc.load("det", mcs.capi)
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.zeros_like(a)
    dp = ct.POINTER(ct.c_double)
    assert _LIB.orc_eval_fn(mcs.capi.FN[fn], len(a), a.ctypes.data_as(dp), a.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    return out


def make_case(name):
    if name in ("protons", "general", "electrons", "oblique"):
        prob, aa = fuzz_problem(name, 64)
        return tc.Case(name, prob, 1, aa, 1.0)
    if name == "epsB":
        return tc.Case(name, make_problem(64, use_custom_epsB=True), 1, 1.0, 1.0)
    if name == "xspec":
        rg0 = make_problem(64).rg0
        prob = make_problem(64, XSPEC=tuple(x * rg0 for x in (-0.5, 0.05, 2.0)))
        assert len(prob.x_spec) == 3
        return tc.Case(name, prob, 1, 1.0, 1.0)
    raise KeyError(name)


def parallel(case):
    return not np.any(case.prob.theta)


@dataclass
class Tables:
    xg: np.ndarray
    ux: np.ndarray
    gsf: np.ndarray
    gef: np.ndarray
    bt: np.ndarray
    th: np.ndarray


def tables(case):
    t = [np.ascontiguousarray(v, dtype=np.float64) for v in case.prob.grid_tables()]     # x, ux, uz, ut, gsf, gef, bef, bt, th
    return Tables(t[0], t[1], t[4], t[5], t[7], t[8])


def zone_of(xg, x):
    return np.clip(np.searchsorted(xg, x, side="right") - 1, 0, len(xg) - 2)


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------
def np_derive(case, pop):
    """The prologue of particle_loop in plain IEEE operations, in the reference's order -> dict of arrays"""
    P, tb = case.prob.params, tables(case)
    m = case.aa * MP
    mc = m * CC
    zzq = case.zz * QCGS
    ig = pop.grid
    gam = oev("hypot1", pop.ptot_pf / mc)
    gd = 1 / (zzq * tb.bt[ig])
    if P.use_custom_epsB:
        with np.errstate(invalid="ignore"):
            gd = np.where(pop.x_PT_cm > P.x_grid_stop, gd * np.sqrt(pop.x_PT_cm / P.x_grid_stop), gd)
    grt = pop.ptot_pf * CC * gd
    period = TWOPI * gam * m * CC * gd
    if case.aa < 1:
        v_fac = np.where(pop.ptot_pf < P.pe_crit, (P.pe_crit * CC * gd) * P.pe_crit / (m * P.game_crit * P.u2),
                         grt * pop.ptot_pf / (m * gam * P.u2))
    else:
        v_fac = grt * pop.ptot_pf / (m * gam * P.u2)
    L_diff = P.eta_mfp / 3 * v_fac
    return dict(m=m, gam=gam, gd=gd, grt=grt, period=period, L_diff=L_diff)


def np_x_dt(case, prp, L_diff):
    """downstream_test's threshold: the particle ends iff x > feb_downstream (when set) or (x > 1.1 prp and x > 6.91 L_diff)"""
    P = case.prob.params
    t = np.maximum(1.1 * prp, 6.91 * L_diff)
    return np.where((P.feb_downstream > 0) & (P.feb_downstream < t), P.feb_downstream, t)


def np_move(case, pop, d=None):
    """Code Block 2's move for a PARALLEL field (b_sin = 0: the gyro term is exactly 0, b_cos = cos(0) = 1) -> (x_new, phi_new)"""
    assert parallel(case)
    tb = tables(case)
    d = d or np_derive(case, pop)
    ig = pop.grid
    t_step = d["period"] / pop.xn_per
    x_move = pop.pb_pf * t_step / (d["gam"] * d["m"])
    dx = tb.gsf[ig] * (x_move * 1.0 - 0.0 + tb.ux[ig] * t_step)
    return pop.x_PT_cm + dx, oev("mod2pi", pop.phi_rad + TWOPI / pop.xn_per)


def np_zone_search(xg, x, fwd, ig):
    """all_flux.jl:68-72 by searchsorted: forward findnext(>(x), x_grid, ig + 1) - 1, backward findprev(<=(x), x_grid, ig); -1 off the grid"""
    ne = len(xg)
    first_gt = np.searchsorted(xg, x, side="right")             # first j with xg[j] > x (ne if none)
    f = np.maximum(first_gt, ig + 1)                            # ... at or after ig + 1 (the grid increases)
    fw = np.where(f >= ne, -1, f - 1)
    last_le = first_gt - 1                                      # last j with xg[j] <= x (-1 if none)
    bw = np.minimum(last_le, ig)
    return np.where(fwd, fw, bw).astype(np.int64)


def np_events(case, pop, x_old, x_new, d):
    """The events due after a move, as the reference states them on (x_old, x_new) -> dict of bool arrays"""
    P, tb = case.prob.params, tables(case)
    ig = pop.grid
    fwd = x_new > x_old
    same = np.where(fwd, tb.xg[ig + 1] > x_new, tb.xg[ig] <= x_new)
    xgs, prp = P.x_grid_stop, pop.prp_x_cm
    coarse = pop.xn_per == P.xn_per_coarse
    ev = dict(left=~same,
              stop=(x_old < xgs) & (xgs <= x_new),
              prp=(x_new >= xgs) & (x_old < prp) & (prp <= x_new),
              dtest=((P.feb_downstream > 0) & (x_new > P.feb_downstream)) | ((x_new > 1.1 * prp) & (x_new > 6.91 * d["L_diff"])),
              xn=(x_new > d["grt"]) != coarse,
              feb=(ig <= P.i_grid_feb) & (pop.inj != 0) & (x_new < P.feb_upstream))
    inj_frac = float(case.prob.inj_fracs[case.i_ion - 1])
    # what the odd configurations add to a pass (the exact move reports them in its event bit): the retry loop of no_DSA_loop, the
    # electrons' PRP logic beyond x_grid_stop (prob_return.jl:100-121), the detectors of all_flux!
    ev["reflect"] = (x_new <= 0) & (x_old > 0) & (pop.inj == 0) & bool(P.dont_DSA or inj_frac < 1)
    ev["odd"] = ev["reflect"] | ((x_new >= xgs) & bool(case.aa < 1)) | bool(len(case.prob.x_spec) != 0)
    ev["odd"] = ev["odd"] | ((P.feb_downstream > 0) & (x_new > P.feb_downstream))       # (the downstream FEB: also part of `dtest`)
    return ev


def np_thresholds(case, pop, x_thr, d, no_xn=False, mutate=None):
    """The two thresholds of the common pass as the table above refresh_thr states them, for a lane that left the rare region at x_thr.
    mutate = "feb_gt": the one non-strict compare of the table whose strict form loses an event (x_thr > feb_upstream for >=: an
    injected particle exactly on the upstream FEB gets no threshold there) -- the host test shows that the states tell the two apart.
    (The other compares of the table only decide on which side a boundary is armed for a lane that sits exactly on it: with `<=` for `<`
    at the grid end, the PRP or gyro_rad_tot the thresholds are more eager, never blind.)"""
    P, tb = case.prob.params, tables(case)
    ig = pop.grid
    inf = np.inf
    hi, lo = tb.xg[ig + 1].copy(), tb.xg[ig].copy()
    for T in (np.full(pop.n, P.x_grid_stop), pop.prp_x_cm):
        up = x_thr < T
        hi = np.where(up & (T < hi), T, hi)
        lo = np.where(~up & (T > lo), T, lo)
    near_feb = (ig <= P.i_grid_feb) & (pop.inj != 0) & ((x_thr > P.feb_upstream) if mutate == "feb_gt" else (x_thr >= P.feb_upstream))
    lo = np.where(near_feb & (P.feb_upstream > lo), P.feb_upstream, lo)
    x_dt = np_x_dt(case, pop.prp_x_cm, d["L_diff"])
    hi = np.minimum(x_dt, hi)
    hi = np.where(x_thr > x_dt, -inf, hi)
    if not no_xn:
        g = d["grt"]
        coarse = pop.xn_per == P.xn_per_coarse
        above = x_thr > g
        hi = np.where(coarse, hi, np.where(above, -inf, np.minimum(g, hi)))
        lo = np.where(coarse, np.where(above, np.maximum(g, lo), inf), lo)
    return hi, lo, x_dt


def contract_domain(case, pop, x_thr, d):
    """Where the thresholds' contract speaks: x_thr is a position a lane can leave the rare region ALIVE at -- inside its zone, the
    step size decided there (coarse iff x_thr > gyro_rad_tot), not beyond x_dt (downstream_test would have ended it), not an injected
    particle beyond the upstream FEB (Code Block 3 would have) --, and x has not reached a threshold since."""
    P, tb = case.prob.params, tables(case)
    ig = pop.grid
    hi, lo, x_dt = np_thresholds(case, pop, x_thr, d)
    coarse = pop.xn_per == P.xn_per_coarse
    ok = (tb.xg[ig] <= x_thr) & (x_thr < tb.xg[ig + 1]) & (coarse == (x_thr > d["grt"])) & (x_thr <= x_dt)
    ok &= ~((ig <= P.i_grid_feb) & (pop.inj != 0) & (x_thr < P.feb_upstream))
    x = pop.x_PT_cm
    ok &= np.where(x == x_thr, True, (lo < x) & (x < hi))
    return ok


# ---- the states ------------------------------------------------------------------------------------------------------------------
@dataclass
class States:
    pop: object
    x_thr: np.ndarray
    cls: np.ndarray          # class name per state
    target: np.ndarray       # the number the state aims at (nan: none)

    @property
    def n(self):
        return self.pop.n


class _Rows:
    FIELDS = ("weight", "ptot", "pb", "x", "xn", "prp", "acc", "phi", "tcut", "down", "inj", "thr", "target", "walk")

    def __init__(self):
        self.r = {k: [] for k in self.FIELDS}
        self.cls = []

    def add(self, cls, **kw):
        for k in self.FIELDS:
            self.r[k].append(kw[k])
        self.cls.append(cls)


def _pop_of(case, r, x):
    n = len(x)
    pop = mcs.capi.Population(n)
    pop.weight[:] = r["weight"]; pop.ptot_pf[:] = r["ptot"]; pop.pb_pf[:] = r["pb"]; pop.x_PT_cm[:] = x; pop.xn_per[:] = r["xn"]
    pop.prp_x_cm[:] = r["prp"]; pop.acctime_sec[:] = r["acc"]; pop.phi_rad[:] = r["phi"]; pop.tcut[:] = r["tcut"]
    pop.downstream[:] = r["down"]; pop.inj[:] = r["inj"]
    pop.grid[:] = zone_of(tables(case).xg, pop.x_PT_cm)
    return pop


def first_move(case, pop):
    """(x_new, phi_new) of the FIRST move of Code Block 2 (before any retry of no_DSA_loop): the numpy restatement for a parallel field;
    with an oblique field the oracle's (whose configuration here has no retry loop: inj_frac = 1, DSA on)"""
    if parallel(case):
        return np_move(case, pop)
    P = case.prob.params
    assert not P.dont_DSA and float(case.prob.inj_fracs[case.i_ion - 1]) == 1.0
    from conftest import oracle_backend
    ob = oracle_backend(case.prob)
    case.begin(ob)
    ob.set_retro_cap(RETRO_CAP)
    # (with the PRP out of reach: a PRP return would put the particle back on the PRP and draw a new phase; nothing else of Code Block 2
    # touches x or phi after the move in this configuration)
    far = mcs.capi.Population(pop.n)
    for f in pop.fields():
        getattr(far, f)[:] = getattr(pop, f)
    far.prp_x_cm[:] = 1e300
    out, word, _ = ob.eval_move(far, I_PCUT, log=False)
    ob.destroy()
    assert not unpack(word)["draws"].any()
    return out[:, 0], out[:, 2]


def _dx_parts(case, tb, ig, ptot, xn, x):
    """t_step and the factor of pb_pf in dx, for placement (double precision is ample: the placement is corrected afterwards)"""
    P = case.prob.params
    m = case.aa * MP
    gam = float(oev("hypot1", np.array([ptot / (m * CC)]))[0])
    gd = 1 / (case.zz * QCGS * tb.bt[ig])
    if P.use_custom_epsB and x > P.x_grid_stop:
        gd *= np.sqrt(x / P.x_grid_stop)
    t_step = TWOPI * gam * m * CC * gd / xn
    return t_step, t_step / (gam * m) * np.cos(tb.th[ig]), gam, gd


PTOTS = (3.0, 20.0, 1e3, 1e6, 1e9, 1e12, 1e17, 1e24, 1e34, 1e40, 1e45)       # in m c


def build_states(case, seed=11):
    P, tb = case.prob.params, tables(case)
    prob = case.prob
    rg0, xgs, ng = prob.rg0, P.x_grid_stop, P.n_grid
    xg = tb.xg
    mc = case.aa * MP * CC
    rng = np.random.default_rng(seed)
    R = _Rows()
    nt = len(prob.tcuts)
    PRP_FAR = 4.0 * xgs
    oblique = not parallel(case)
    base = dict(weight=1.0 / 4096, prp=PRP_FAR, acc=0.0, phi=1.0, tcut=1, down=0, inj=0, thr=np.nan, target=np.nan, walk=0)

    def aim(cls, T, dx=None, frac=None, ptots=PTOTS, xns=None, walk=3, start=None, target=None, **kw):
        """A state whose move ends on T: pb_pf solved for the wanted dx over the momenta `ptots` (the first that can), or the plain
        fraction `frac` of ptot_pf.  start: the state starts THERE and T is ignored (x_old on a boundary).  xns None: the step size
        the rare region would have left at the state's position (coarse iff x > gyro_rad_tot), else the one given."""
        done = False
        for xn in (xns or (P.xn_per_coarse, P.xn_per_fine)):
            if done:
                break
            for pm in ptots:
                ptot = pm * mc
                x_guess = (T - dx) if dx is not None else T
                if start is not None:
                    x_guess = start
                phi = kw.get("phi", base["phi"])
                for _ in range(3):
                    ig = int(zone_of(xg, x_guess))
                    t_step, k1, _, gd_ = _dx_parts(case, tb, ig, ptot, xn, x_guess)

                    def dx_of(pb):      # (with the gyro term of an oblique field)
                        gyr = 0.0
                        if oblique:
                            gyr = np.sqrt(max(ptot * ptot - pb * pb, 0.0)) * CC * gd_ * np.sin(tb.th[ig]) * (np.cos(phi + TWOPI / xn) - np.cos(phi))
                        return tb.gsf[ig] * (pb * k1 - gyr + tb.ux[ig] * t_step)
                    if dx is None:
                        pb = frac * ptot
                    elif not oblique:
                        pb = (dx / tb.gsf[ig] - tb.ux[ig] * t_step) / k1
                    else:
                        lo_, hi_ = -0.999 * ptot, 0.999 * ptot
                        pb = np.inf
                        if (dx_of(lo_) - dx) * (dx_of(hi_) - dx) <= 0:
                            for _b in range(80):
                                mid = 0.5 * (lo_ + hi_)
                                if (dx_of(lo_) - dx) * (dx_of(mid) - dx) <= 0:
                                    hi_ = mid
                                else:
                                    lo_ = mid
                            pb = 0.5 * (lo_ + hi_)
                    dxa = dx_of(pb) if np.isfinite(pb) else 0.0
                    if start is None:
                        x_guess = T - dxa
                if abs(pb) > 0.999 * ptot or not np.isfinite(pb):
                    continue
                _, _, _, gd = _dx_parts(case, tb, ig, ptot, xn, x_guess)
                if xns is None and xn == P.xn_per_coarse and not x_guess > ptot * CC * gd:
                    break          # (coarse steps below a gyroradius: try the fine ones)
                done = True
                row = dict(base); row.update(kw)
                row.update(ptot=ptot, pb=pb, x=x_guess, xn=xn, target=T if target is None else target, walk=0 if start is not None else walk)
                R.add(cls, **row)
                break

    def around(cls, T, **kw):
        """T approached from below and from above (`sides`) with |dx| an eighth of |T| (or `s`), with plain pitch fractions (`fracs`),
        and left from T itself in both directions"""
        s = kw.pop("s", abs(T) / 8)
        sides, fracs, starts = kw.pop("sides", (1.0, -1.0)), kw.pop("fracs", (0.5, -0.5)), kw.pop("starts", (1.0, -1.0))
        for sg in sides:
            aim(cls, T, dx=sg * s, **kw)
        for sg in starts:
            if kw.get("ptots") is not None and len(kw["ptots"]) == 1:      # (one momentum: its own step, not a solved one)
                aim(cls, T, frac=0.9 * sg, start=T, **kw)
            else:
                aim(cls, T, dx=sg * s / 64, start=T, **kw)      # (a small step: no other boundary is within reach)
        for fr in fracs:
            aim(cls, T, frac=fr, **dict(dict(ptots=(3.0,)), **kw))

    # every zone edge; the grid end; the PRP on either side of it, 1.1 prp, 6.91 L_diff, the downstream FEB
    for j in range(1, ng + 1):
        if xg[j] != 0.0:
            around("edge", xg[j], down=int(xg[j] > 0))
    # (a position beyond x_dt is none a live particle holds: where a class aims at x_dt itself, or beyond the downstream FEB, the
    # states come from below only)
    feb = P.feb_downstream > 0
    below = dict(sides=(1.0,), fracs=(0.5,))
    around("x_grid_stop", xgs, down=1, **(below if feb and P.feb_downstream <= xgs else {}))
    for cls, prp in (("prp_lo", 0.5 * xgs), ("prp_hi", 2.0 * xgs)):
        if feb and prp >= P.feb_downstream:
            continue
        around(cls, prp, prp=prp, down=1, s=prp / 16)
        around("prp11", 1.1 * prp, prp=prp, down=1, ptots=(3.0, 20.0), **below)
    for pm in (20.0, 1e3):
        ig = int(zone_of(xg, 2 * xgs))
        _, _, gam, gd = _dx_parts(case, tb, ig, pm * mc, P.xn_per_coarse, 2 * xgs)
        T = 6.91 * (P.eta_mfp / 3 * ((pm * mc * CC * gd) * (pm * mc) / (case.aa * MP * gam * P.u2)))
        if not (P.feb_downstream > 0 and T > P.feb_downstream) and not P.use_custom_epsB and not (case.aa < 1 and pm * mc < P.pe_crit):
            around("ldiff", T, prp=0.01 * rg0, down=1, ptots=(pm,), **below)
    if feb:
        around("feb_down", P.feb_downstream, down=1, prp=PRP_FAR, **below)
    # gyro_rad_tot with fine and coarse steps (downstream, where x > 0 can be a gyroradius): fine steps from below, coarse ones from
    # above (the step size the rare region leaves is coarse iff x > gyro_rad_tot; x = gyro_rad_tot itself belongs to the fine ones)
    def grt_of(pm):
        ig = int(zone_of(xg, pm * rg0 / 5))
        for _ in range(6):
            g = pm * mc * CC * _dx_parts(case, tb, ig, pm * mc, P.xn_per_coarse, 0.0)[3]
            ig = int(zone_of(xg, g))
        return g
    for pm in (3.0, 20.0, 1e3):
        g = grt_of(pm)
        if feb and 1.2 * g > P.feb_downstream:
            continue
        around("grt_fine", g, ptots=(pm,), xns=(P.xn_per_fine,), down=1, sides=(), fracs=(0.5, 0.9), phi=1.0)
        around("grt_coarse", g, ptots=(pm,), xns=(P.xn_per_coarse,), down=1, sides=(), fracs=(-0.9, -0.6), starts=(), phi=4.0)
    # the upstream FEB, in the zones up to i_grid_feb, with and without inj
    around("feb_up", P.feb_upstream, inj=0, down=0)
    around("feb_up", P.feb_upstream, inj=1, down=1, sides=(-1.0,), fracs=())      # (injected and beyond it: Code Block 3 has ended it)
    # the shock: from both sides, x exactly +-0.0, and x_old > 0 >= x with inj clear / set
    for s in (1e-8 * rg0, 1e-3 * rg0, 0.3 * rg0):
        for inj in (0, 1):
            around("shock", 0.0, s=s, inj=inj, down=inj)
    for z in (0.0, -0.0):
        for sg in (1.0, -1.0):
            for inj in (0, 1):
                aim("shock", 0.0, dx=sg * 1e-3 * rg0, start=z, inj=inj, down=inj)
    # multi-zone moves in both directions: inside the target zone and exactly on its near edge
    i0 = int(np.searchsorted(xg, 0.0))
    for a, spans in ((i0 + 1, (1, 2, 3, 4, 5, 9, 17, ng - i0 - 1)), (ng - 9, (-1, -2, -3, -4, -5, -9, -(ng - 9 - i0 - 1), -(ng - 9 - i0 + 2), -40, -(ng - 10))),
                     (30, (-1, -2, -3, -4, -12, 1, 2, 3, 4, 20, 40, 60))):
        xa = 0.5 * (xg[a] + xg[a + 1]) if a < ng else 2 * xg[ng]
        for sp in spans:
            b = a + sp
            if not 1 <= b <= ng:
                continue
            xb = 0.5 * (xg[b] + xg[b + 1]) if b < ng else 2 * xg[ng]
            aim("jump", xb, dx=xb - xa, down=int(xa > 0), walk=0)
            edge = xg[b] if sp > 0 else xg[b + 1]
            if b + (sp < 0) <= ng:
                aim("jump", edge, dx=edge - xa, down=int(xa > 0), walk=1)
    # off either end of the grid, and onto the sentinels
    x_lo, x_hi = 0.5 * (xg[1] + xg[2]), 0.5 * (xg[ng - 1] + xg[ng])
    aim("off_grid", 4 * xg[ng + 1], dx=4 * xg[ng + 1] - x_hi, start=x_hi, down=1)
    aim("off_grid", xg[ng + 1], dx=xg[ng + 1] - x_hi, start=x_hi, down=1)
    aim("off_grid", 4 * xg[0], dx=4 * xg[0] - x_lo, start=x_lo)
    aim("off_grid", xg[0], dx=xg[0] - x_lo, start=x_lo)
    # re-arming: the thresholds of x_thr, x between x_thr and the boundary T (all in one zone), the move across T
    def rearm(T, **kw):
        for cls, sg in (("rearm_down", 1.0), ("rearm_up", -1.0)):
            z = int(zone_of(xg, np.nextafter(T, sg * np.inf)))
            room = (xg[z + 1] - T) if sg > 0 else (T - xg[z])
            dl = 0.5 * min(room, abs(T) / 16)
            if feb and T + sg * dl > P.feb_downstream:
                continue
            aim(cls, T - sg * dl / 2, dx=-sg * dl, start=T + sg * dl / 2, thr=T + sg * dl, down=1, target=T, **kw)
    rearm(xgs, prp=PRP_FAR)
    rearm(2.0 * xgs, prp=2.0 * xgs)
    rearm(0.5 * xgs, prp=0.5 * xgs)
    for pm in (20.0, 1e3):
        rearm(grt_of(pm), ptots=(pm,))
    # PRP crossings beyond x_grid_stop: vt < u2, vt just above u2, and momenta whose returns start the retro walk
    beta2 = P.u2 / CC
    for pm in (() if feb else (0.5 * beta2, beta2 / np.sqrt(1 - beta2 ** 2) * (1 + 1e-3), 3.0, 1e3)):
        for _ in range(37 if pm < 1 else 97):
            aim("prp_return", 2.0 * xgs * (1 + 1 / 256), frac=0.6, start=2.0 * xgs * (1 - 2.0 ** -30), prp=2.0 * xgs, down=1, ptots=(pm,), target=2.0 * xgs)
    # time cuts: acctime on either side of, and on, the next cut; the index beyond the last cut; age_max
    for j in range(nt):
        for acc in (np.nextafter(prob.tcuts[j], 0.0), prob.tcuts[j], np.nextafter(prob.tcuts[j], np.inf)):
            aim("tcut", 0.5 * rg0, frac=0.3, start=0.5 * rg0, ptots=(3.0,), down=1, acc=acc, tcut=j + 1)
    for acc in (0.0, 1e300):
        aim("tcut", 0.5 * rg0, frac=0.3, start=0.5 * rg0, ptots=(3.0,), down=1, acc=acc, tcut=nt + 1)
    if P.age_max > 0:
        for acc in (np.nextafter(P.age_max, 0.0), P.age_max, np.nextafter(P.age_max, np.inf)):
            aim("tcut", 0.5 * rg0, frac=0.3, start=0.5 * rg0, ptots=(3.0,), down=1, acc=acc, tcut=nt + 1)

    # ---- correct the aimed states by the first move's own error, then walk them over +- `walk` ulps
    r = {k: np.array(v, dtype=np.float64) for k, v in R.r.items()}
    cls = np.array(R.cls)
    x = r["x"].copy()
    aimed = r["walk"] > 0
    x_new, _ = first_move(case, _pop_of(case, r, x))
    with np.errstate(invalid="ignore", over="ignore"):
        x_fix = x + (r["target"] - x_new)
    keep_zone = zone_of(xg, x_fix) == zone_of(xg, x)
    x = np.where(aimed & keep_zone & np.isfinite(x_fix), x_fix, x)
    reps = (2 * r["walk"] + 1).astype(np.int64)
    idx = np.repeat(np.arange(len(x)), reps)
    step = np.concatenate([np.arange(-w, w + 1) for w in r["walk"].astype(np.int64)])
    xs = x[idx]
    for k in range(1, 4):
        xs = np.where(step >= k, np.nextafter(xs, np.inf), np.where(step <= -k, np.nextafter(xs, -np.inf), xs))
    r = {k: v[idx] for k, v in r.items()}
    cls = cls[idx]
    crafted = _pop_of(case, r, xs)
    thr = np.where(np.isnan(r["thr"]), xs, r["thr"])

    # ---- the fuzzed background: the step size of nine states in ten is the one the rare region would have left (coarse iff x > gyro_rad_tot)
    fz = fuzz_population(prob, N_FUZZ, seed, case.aa)
    dz = np_derive(case, fz)
    fix = rng.random(N_FUZZ) < 0.9
    fz.xn_per[:] = np.where(fix, np.where(fz.x_PT_cm > dz["grt"], P.xn_per_coarse, P.xn_per_fine), fz.xn_per)
    n = crafted.n + N_FUZZ
    pad = 1 if n % 256 == 0 else 0
    pop = mcs.capi.Population(n + pad)
    for f in pop.fields():
        a = getattr(pop, f)
        a[:crafted.n] = getattr(crafted, f)
        a[crafted.n:n] = getattr(fz, f)
        if pad:
            a[n:] = getattr(fz, f)[:1]
    S = States(pop, np.concatenate([thr, fz.x_PT_cm, fz.x_PT_cm[:pad]]), np.concatenate([cls, np.full(N_FUZZ + pad, "fuzz")]),
               np.concatenate([r["target"], np.full(N_FUZZ + pad, np.nan)]))
    assert S.n % 256 != 0
    for f in pop.fields():
        getattr(pop, f).setflags(write=False)
    S.x_thr.setflags(write=False)
    return S


def check_states(case, S, x_new):
    """The builder's own assertions, on the computed x_new -> {class: (states, below, on, above)}"""
    counts = {}
    d = np_derive(case, S.pop)
    dom = contract_domain(case, S.pop, S.x_thr, d)
    for c in np.unique(S.cls):
        sel = S.cls == c
        T = S.target[sel]
        with np.errstate(invalid="ignore"):
            below, on, above = int((x_new[sel] < T).sum()), int((x_new[sel] == T).sum()), int((x_new[sel] > T).sum())
        counts[str(c)] = (int(sel.sum()), below, on, above)
        if c in TARGET_CLASSES:
            assert below > 0 and on > 0 and above > 0, f"{case.name}: class {c} has {below} states below, {on} on and {above} above its target"
        if c != "fuzz":
            assert dom[sel].mean() >= 0.9, f"{case.name}: only {dom[sel].mean():.0%} of class {c} is inside the thresholds' contract"
    P = case.prob.params
    feb = P.feb_downstream > 0
    absent = set(TARGET_CLASSES) - set(counts)
    allowed = ({"prp_hi", "ldiff"} if feb else {"feb_down"}) | ({"ldiff"} if P.use_custom_epsB else set())
    assert absent <= allowed, f"{case.name}: no states for {sorted(absent - allowed)}"
    # re-arming: x strictly inside the thresholds of x_thr, x_thr on the other side of x from the boundary
    hi, lo, _ = np_thresholds(case, S.pop, S.x_thr, d)
    x = S.pop.x_PT_cm
    for c, sign in (("rearm_down", 1), ("rearm_up", -1)):
        sel = S.cls == c
        assert sel.sum() >= 2, f"{case.name}: {int(sel.sum())} {c} states"
        assert np.all((lo[sel] < x[sel]) & (x[sel] < hi[sel])), f"{case.name}: a {c} state has left the thresholds of its x_thr"
        assert np.all(sign * (S.x_thr[sel] - x[sel]) > 0) and np.all(sign * (x[sel] - S.target[sel]) > 0)
        assert np.all(sign * (S.target[sel] - x_new[sel]) >= 0), f"{case.name}: a {c} move does not reach its boundary"
    return counts


def np_due(ev, no_xn=False):
    """every event of np_events that the thresholds (or the event bit) of forms 1-3 must not miss"""
    due = ev["left"] | ev["stop"] | ev["prp"] | ev["dtest"] | ev["feb"] | ev["odd"]
    return due if no_xn else due | ev["xn"]


def np_spurious(case, pop, x_thr, x_new, d, no_xn=False):
    """The stops of the thresholds with nothing due, by the table above refresh_thr -> dict of bool arrays, tried in this order:
      boundary    x_new EQUALS a boundary the thresholds were folded from (zone edge, grid end, PRP, upstream FEB, gyro_rad_tot, x_dt)
      rearm       x_new came down to x_grid_stop or the PRP from an x_thr at or above it: the visit that makes it an upward threshold again
      beyond_dt   x_new > x_dt
      prp_below   x_new came up to a PRP that lies below x_grid_stop (prob_return asks for x >= x_grid_stop: nothing is due there, and the
                  table folds the PRP without looking at x_grid_stop)"""
    P, tb = case.prob.params, tables(case)
    ig = pop.grid
    x_dt = np_x_dt(case, pop.prp_x_cm, d["L_diff"])
    bnd = (x_new == tb.xg[ig]) | (x_new == tb.xg[ig + 1]) | (x_new == P.x_grid_stop) | (x_new == pop.prp_x_cm) | (x_new == x_dt)
    bnd |= (x_new == P.feb_upstream) & (ig <= P.i_grid_feb) & (pop.inj != 0)
    if not no_xn:
        bnd |= x_new == d["grt"]
    rearm = np.zeros(pop.n, dtype=bool)
    for T in (np.full(pop.n, P.x_grid_stop), pop.prp_x_cm):
        rearm |= (x_thr >= T) & (x_new < T)
    return dict(boundary=bnd, rearm=rearm & ~bnd, beyond_dt=(x_new > x_dt) & ~bnd & ~rearm,
                prp_below=(x_thr < pop.prp_x_cm) & (x_new > pop.prp_x_cm) & (pop.prp_x_cm < P.x_grid_stop) & ~bnd & ~rearm & ~(x_new > x_dt))


# ---- the packed word of mcs_eval_move (include/mcs.h) ------------------------------------------------------------------------------
def unpack(word):
    w = np.asarray(word, dtype=np.uint64)

    def f(sh, bits):
        return ((w >> np.uint64(sh)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    return dict(i_grid=f(0, 8), i_grid_old=f(8, 8), ig3=f(16, 8), tcut=f(24, 8), downstream=f(32, 1), inj=f(33, 1), end=f(34, 3), b1=f(37, 1),
                crossed=f(38, 1), zone=f(39, 1), ev=f(40, 1), ev_cross=f(41, 1), plain=f(42, 1), npush=f(43, 2), n_retro=f(45, 9), draws=f(54, 10))


DEVICE_BITS = np.uint64(7 << 40)          # the move's event bit, ev_cross, plain_crossing's return value: the oracle has none
NPUSH_BITS = np.uint64(3 << 43)
GOES_ON = 7


def describe(S, k):
    p = S.pop
    return (f"state {k} ({S.cls[k]}, target {float(S.target[k]).hex()}): x {float(p.x_PT_cm[k]).hex()} x_thr {float(S.x_thr[k]).hex()} ptot "
            f"{float(p.ptot_pf[k]).hex()} pb {float(p.pb_pf[k]).hex()} xn {p.xn_per[k]:g} prp {float(p.prp_x_cm[k]).hex()} acctime "
            f"{float(p.acctime_sec[k]).hex()} phi {float(p.phi_rad[k]).hex()} weight {float(p.weight[k]).hex()} grid {int(p.grid[k])} tcut "
            f"{int(p.tcut[k])} downstream {int(p.downstream[k])} inj {int(p.inj[k])}")
