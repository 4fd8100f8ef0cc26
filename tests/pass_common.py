"""States for mcs_eval_pass / orc_eval_pass: one pass boundary per state -- the move of Code Block 2 with what it triggers, then the head
of Code Block 3 (slow_pre in csrc/mcs_transport.hip): helix cap, zone reload, frame change, energy transfer, the exit tests, the
electrons' radiative loss, the save for the next pcut, the fine / coarse step.

A state is a row of move_common (the population AFTER the scatter and the clock of the pass that moves) plus `helix`, the count of that
pass.  build_states() takes move_common's states of the problem -- they already put the move's end within an ulp of every zone edge
(frame change: crossings into zones of equal and of different u_x, jumps over 2, 3 and dozens of zones, the shock in both directions, the
oblique field; energy transfer: x_old < 0, x_old = +-0.0, x_old > 0, inj set and clear, from i_grid_old = 0 ... across the shock), of the
upstream FEB with inj set and clear, and acctime within an ulp of every time cut and of age_max -- and adds, per problem:

    helix         helix = cap - 1, cap; for electrons 999, 1000, 2000 beyond x_grid_stop with ptot_pf < pcut_prev (prob_return's % 1000 branch)
    pmax_pf       ptot_pf one ulp below, on and one ulp above pmax_cutoff, four pitches, upstream and downstream
    pmax_sk       ptot_pf above pmax_cutoff by 1e-6 .. 5e-2, 41 pitches: the shock-frame momentum on both sides of pmax_cutoff; and ptot_pf
                  below it with pitches whose shock-frame momentum is above (no exit: the reference's own rule)
    save          ptot_pf one ulp below, on and one ulp above pcut, downstream and upstream; saves whose clock reaches the next time
                  cut, and with the time-cut index beyond the last cut
    loss          (electrons with losses) ptot_pf solved for dlnp = 1e-2 and walked over +-3 ulps, momenta from 1e-3 to 1e6 m c (1 - dlnp
                  rounds to 1 at the low end), ptot_pf from pe_crit upwards in steps from one ulp to 1e-3 (the loss takes it across);
                  with custom eps_B also beyond x_grid_stop
    step          momenta at or below this launch's pcut (a particle above it downstream is saved before the choice): x after the move
                  within +-3 ulps of the gyro_rad_tot that the pass head leaves (after its loss); counted at the fine / coarse choice
    step_frame    (the ramp problem, whose flow still slows down behind the shock) a move across a downstream zone edge into a zone of
                  another u_x, x after it within +-3 ulps of the gyro_rad_tot that the frame change leaves
    dont_scatter  (no-scatter problem) x after the move within +-3 ulps of 10 gyro_rad
    frame         the shock crossed in both directions with p_perp = 0, |pb_pf| one ulp below ptot_pf, and phi on and beside 0, pi/2, 2 pi
    etf           (problems with energy transfer) not yet injected, across the last upstream zones and the shock, 270 momenta 1.8 % apart
                  around pcut and pmax_cutoff, and for the receiver momenta below them by steps of 1e-4 and 1e-14
    feb_up        move_common's injected states at the upstream FEB, aimed again with the pass's own move
    fuzz          move_common's 2000 fuzzed states, with random helix counts

`step` and `dont_scatter` aim at a number the head itself computes: the builder asks the oracle for it (it does not depend on x inside a
zone for a parallel field), moves x by the difference and walks over +-3 ulps.  check_states() classifies every state from the
reference's output and the numpy restatement below, never from the intent.

np_head() restates, in plain IEEE operations from the Julia text (particle_loop.jl:158-165, 251-326, 361-385, 578-592), the exit tests in
their order, radiation_loss with what hangs on the momentum, the save predicate and the fine / coarse choice, for the states it covers:
every state: np_psp restates the frame change in the reference's order of operations, and the donor's and the receiver's energy
transfer are restated in np_head itself.  It shares no code with oracle/mcs_oracle.cpp; hypot1 comes through
orc_eval_fn and the shock-frame momentum of the p_max test through orc_transform_p_PS.

Not built here, and said so in DESIGN.md: for the oblique problem states with ptot_sk within ulps of pmax_cutoff (the pitch is solved for the
parallel fields, swept for all), and transfers that take ptot_pf across pcut (across pmax_cutoff: the donor's only).
"""
import ctypes as ct
from dataclasses import dataclass

import numpy as np

from conftest import mcs, make_problem, oracle_backend
import move_common as mv
import tally_common as tc

MP, CC, QCGS, TWOPI = mv.MP, mv.CC, mv.QCGS, mv.TWOPI
ME_MP = mcs.constants.ME / mcs.constants.MP
PROBLEMS = mv.PROBLEMS + ("electrons_epsB", "etf_recv", "etf_donor", "ramp", "no_scatter")
LOSSY = ("electrons", "etf_recv")  # the problems inside the LOSSY kernel's domain (form 1)
I_PCUT = mv.I_PCUT
HELIX_CAP = 10000
RAD_LOSS_FAC = (4.0 / 3.0) * CC * mcs.constants.SIGMA_T / (CC * CC * CC * mcs.constants.ME * mcs.constants.ME * 8.0 * 3.141592653589793)
OUT = ("pb_pf", "p_perp", "ptot_pf", "gam_pf", "phi", "x", "x_old", "prp", "acctime", "gyro_denom", "gyro_rad", "gyro_rad_tot", "gyro_period",
       "cm_val", "rp_val", "xn_per", "dphi", "t_step", "rg_val", "x_dt", "t_hi", "t_lo", "z_lo", "z_hi", "z_ux", "z_gsf", "z_bcos", "z_gef")
COLS = {n: i for i, n in enumerate(OUT)}
DEVICE_ONLY = ("rp_val", "rg_val", "t_hi", "t_lo")          # the oracle has none
DEVICE_BITS = np.uint64(3 << 62)                            # the move's event bit and ev_cross
# the head's end as the word holds it (end code + 1; 7: the head did not run)
GOES_ON, SAVED, NOT_RUN = 0, 1, 7
# how far a state gets in the head: what a class aims at
STAGES = ("not_run", "helix", "dont_scatter", "pmax", "feb_up", "age", "loss", "save", "step")
CLASS_STAGE = dict(helix="helix", pmax_pf="pmax", pmax_sk="pmax", save="save", loss="loss", step="step", dont_scatter="dont_scatter")
u64 = mv.u64


def make_case(name):
    if name in mv.PROBLEMS:
        return mv.make_case(name)
    if name == "electrons_epsB":      # the loss beyond x_grid_stop with the field of use_custom_epsB; no CMB term
        prob = make_problem(64, species=[mcs.inputs.Species(ME_MP, -1.0, 1e6, 1.0)], radiation_losses=True, B_mag_upstream=3.0,
                            b_field_turbulence=1.0, electron_energy_mfp_threshold=1e4, B_CMBz=0.0, use_custom_epsB=True)
        return tc.Case(name, prob, 1, ME_MP, 1.0)
    if name == "etf_recv":            # proton donor + electron receiver; the electron is the species under test
        prob = make_problem(64, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(ME_MP, -1.0, 1e6, 1.0)],
                            energy_transfer_frac=0.1)
        return tc.Case(name, prob, 2, ME_MP, 1.0)
    if name == "etf_donor":           # a proton donor whose target rises through the precursor: transfers at zone crossings far from the
        prob = make_problem(64, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(ME_MP, -1.0, 1e6, 1.0)],
                            energy_transfer_frac=0.1)      # shock, where no frame change and no change of the field raises a flag
        sh = prob.params.i_shock
        eps = np.array(prob.eps_target, dtype=np.float64)
        for i in range(sh // 2, sh):          # zones i_shock / 2 .. i_shock - 1: every other zone none, then rising to the shock's own
            eps[i - 1] = 0.0 if i % 4 == 0 else 0.08 * (i - sh // 2 + 1) / (sh - sh // 2)
        prob.eps_target = eps
        return tc.Case(name, prob, 1, 1.0, 1.0)
    if name == "ramp":                # protons in a profile whose flow still slows down behind the shock (a smoothed shock): frame changes at
        prob = make_problem(64)       # x > 0, where x can exceed a gyroradius -- the fine / coarse choice after a transform
        xg = prob.x_grid_cm
        i0 = int(np.searchsorted(xg, 0.0))
        ux = np.array(prob.ux, dtype=np.float64)
        for z in range(i0, i0 + 25):
            ux[z] = ux[i0 + 25] * (1 + 5e-4 * (i0 + 25 - z))
        prob.ux = ux
        prob.utot = np.hypot(prob.ux, prob.uz)
        prob.gam_sf = 1 / np.sqrt(1 - (prob.utot / mcs.constants.C) ** 2)
        return tc.Case(name, prob, 1, 1.0, 1.0)
    if name == "no_scatter":
        return tc.Case(name, make_problem(64, no_scatter=True), 1, 1.0, 1.0)
    raise KeyError(name)


def pmax_of(case):
    sp = case.prob.cfg.species[case.i_ion - 1]
    return float(mcs.inputs.get_pmax_cutoff(case.prob.Emax_keV, case.prob.Emax_per_aa_keV, case.prob.pmax, sp.aa))


def seed_pool(case, be, T, I):
    """The receivers' energy pool for the etf_recv problem: zero in the zones far upstream, every third zone non-zero in the middle of the
    precursor, every zone non-zero up to the shock -- so that the ranges the states cross hold none, one or only non-zero entries.
    -> (T, I) to start every launch from."""
    T = T.copy()
    if case.name == "etf_recv":
        P = case.prob.params
        pool = be.layout.view(T, "energy_recv_pool")
        e0 = case.aa * MP * CC * CC
        for i in range(1, P.n_grid + 1):
            if i > P.i_shock // 3:
                pool[i - 1] = (0.25 + i / 64.0) * e0 if (i > 2 * P.i_shock // 3 or i % 3 == 0) else 0.0
    return T, I


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------
def np_gyro_denom(case, ig, x):
    """particle_loop.jl:195-211: 1 / (zz e B) with the field of the zone, or of use_custom_epsB beyond x_grid_stop"""
    P, tb = case.prob.params, mv.tables(case)
    bmag = tb.bt[ig].copy()
    if P.use_custom_epsB:
        with np.errstate(invalid="ignore", divide="ignore"):
            bmag = np.where(x > P.x_grid_stop, tb.bt[P.n_grid] * np.sqrt(P.x_grid_stop / x), bmag)
    return 1 / (case.zz * QCGS * bmag), bmag


def np_period(case, ptot, gam, gd):
    """scattering.jl:39-50: the gyro period the scatter leaves"""
    P = case.prob.params
    mc = case.aa * MP * CC
    if case.aa < 1:
        return np.where(ptot < P.pe_crit, TWOPI * P.game_crit * mc * gd, TWOPI * gam * mc * gd)
    return TWOPI * gam * mc * gd


def oev2(fn, a, b):
    """orc_eval_fn with two arguments (atan2)"""
    mv.oev("cos", np.zeros(1))          # (loads the library)
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    out = np.zeros_like(a)
    dp = ct.POINTER(ct.c_double)
    assert mv._LIB.orc_eval_fn(mcs.capi.FN[fn], len(a), a.ctypes.data_as(dp), b.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    return out


def np_psp(case, pb, pperp, gam, phi, io, ig):
    """transform_p_PSP (transformers.jl:523-607) in the reference's order of operations: the plasma frame of zone io -> the shock frame
    -> the plasma frame of zone ig.  cos, sin, atan2 and hypot1 are the oracle's functions (orc_eval_fn); everything else is an IEEE
    operation.  -> (ptot, pb, pperp, gam, phi, clamped)"""
    pr = case.prob
    f = lambda a: np.asarray(a, dtype=np.float64)
    m = case.aa * MP
    mc = m * CC
    PI = 3.141592653589793
    cs, sn = mv.oev("cos", f(pr.theta)), mv.oev("sin", f(pr.theta))
    uxo, uzo, uto, gso, bco, bso = f(pr.ux)[io], f(pr.uz)[io], f(pr.utot)[io], f(pr.gam_sf)[io], cs[io], sn[io]
    ux, uz, ut, gs, bc, bs = f(pr.ux)[ig], f(pr.uz)[ig], f(pr.utot)[ig], f(pr.gam_sf)[ig], cs[ig], sn[ig]
    phi_p = phi + PI / 2
    ppc = pperp * mv.oev("cos", phi_p)
    x, y, z = pb * bco - ppc * bso, pperp * mv.oev("sin", phi_p), pb * bso + ppc * bco
    qx, qz = uxo / uto, uzo / uto
    sx = ((gso - 1) * (qx * qx) + 1) * x + (gso - 1) * (uxo * uzo / (uto * uto)) * z + gso * gam * m * uxo
    sz = (gso - 1) * (uxo * uzo / (uto * uto)) * x + ((gso - 1) * (qz * qz) + 1) * z + gso * gam * m * uzo
    psk = np.sqrt(sx * sx + y * y + sz * sz)
    pbsk = sx * bc + sz * bs
    clamped = psk < np.abs(pbsk)
    gsk = mv.oev("hypot1", psk / mc)
    qx, qz = ux / ut, uz / ut
    px = ((gs - 1) * (qx * qx) + 1) * sx + (gs - 1) * (ux * uz / (ut * ut)) * sz - gs * gsk * m * ux
    pz = (gs - 1) * (ux * uz / (ut * ut)) * sx + ((gs - 1) * (qz * qz) + 1) * sz - gs * gsk * m * uz
    ptot = np.sqrt(px * px + y * y + pz * pz)
    pbn = px * bc + pz * bs
    cl2 = ptot < np.abs(pbn)
    with np.errstate(invalid="ignore"):
        pp_c = 1.0e-6 * ptot
        pperp_n = np.where(cl2, pp_c, np.sqrt(ptot * ptot - pbn * pbn))
        pbn = np.where(cl2, np.copysign(np.sqrt(ptot * ptot - pp_c * pp_c), pbn), pbn)
    gam_n = mv.oev("hypot1", ptot / mc)
    phi_n = oev2("atan2", y, -px * bs + pz * bc) - PI / 2
    return ptot, pbn, pperp_n, gam_n, phi_n, clamped.astype(np.int64) + cl2.astype(np.int64)


def np_head(case, ob, pop, helix, pre, wpre, mutate=None, pool=None):
    """The head of the pass that follows the move, from the state the move left (`pre`, `wpre`: orc_eval_pass's rows and words with the
    head skipped, i.e. the state after Code Block 2) -> dict: end (the word's code: 0 goes on, 1 saved, 2..5 i_reason 1..4, 7 not run),
    stage (index into STAGES: the last test the state reached), ptot / gam / pb / pperp / grt / gr / xn after the head, dlnp, covered.
    mutate: the name of one comparison to state the other way (">" <-> ">=", "<" <-> "<="), for the host test that shows that the states
    tell the two apart: pmax, feb_up, age, pcut, dlnp, grt."""
    P, tb = case.prob.params, mv.tables(case)
    n = pop.n
    m = case.aa * MP
    mc = m * CC
    w = unpack(wpre)
    ig, ig_in = w["i_grid"], np.asarray(pop.grid, dtype=np.int64)
    x, ptot, pb, pperp, gam, phi, acc = (pre[:, COLS[k]].copy() for k in ("x", "ptot_pf", "pb_pf", "p_perp", "gam_pf", "phi", "acctime"))
    gr, grt = pre[:, COLS["gyro_rad"]].copy(), pre[:, COLS["gyro_rad_tot"]].copy()
    inj, down = w["inj"] != 0, w["downstream"] != 0
    runs = (w["post_end"] == 7) & (w["n_retro"] == 0) & ~prp_return(case, pop, pre)
    etf = bool(P.energy_transfer_frac > 0) & ~inj & (pre[:, COLS["x_old"]] <= 0) & (w["i_grid_old"] != ig)
    covered = np.ones(n, dtype=bool)          # (every state: the frame change and the energy transfers are restated below)
    end = np.full(n, NOT_RUN)
    stage = np.zeros(n, dtype=np.int64)
    live = runs.copy()

    def leave(cond, code, st):
        hit = live & cond
        end[hit] = code
        stage[live] = st
        live[hit] = False

    def cmp(name, a, b, strict_gt=True):
        """a > b (or a < b), or the other strictness under `mutate`"""
        flip = mutate == name
        if strict_gt:
            return (a >= b) if flip else (a > b)
        return (a <= b) if flip else (a < b)

    leave(helix + 1 > HELIX_CAP, 2, STAGES.index("helix"))
    gd, bmag = np_gyro_denom(case, ig, x)
    # the frame change into a zone of another u_x (particle_loop.jl:214-233); the gyroradii follow with the new field
    psp = live & (tb.ux[ig] != tb.ux[ig_in])
    n_clamp = np.zeros(n, dtype=np.int64)
    if psp.any():
        k = np.flatnonzero(psp)
        ptot[k], pb[k], pperp[k], gam[k], phi[k], n_clamp[k] = np_psp(case, pb[k], pperp[k], gam[k], phi[k], ig_in[k], ig[k])
        gr[k] = pperp[k] * CC * gd[k]
        grt[k] = ptot[k] * CC * gd[k]
    # energy transfer (particle_loop.jl:235-249 -> :652-723): the donor (aa >= 1) gives up the share eps_target of its kinetic energy over
    # the zones it crossed, the receiver takes what the pool of those zones holds; the momenta are scaled, the gyroradii stay
    ptot_before_etf = ptot.copy()
    did_etf = np.zeros(n, dtype=bool)
    if P.energy_transfer_frac > 0:
        eps = np.asarray(case.prob.eps_target, dtype=np.float64)
        pl = np.zeros(P.n_grid) if pool is None else np.asarray(pool, dtype=np.float64)
        E0 = m * (CC * CC)
        for k in np.flatnonzero(live & etf & covered):
            i_start, i_stop = int(w["i_grid_old"][k]), int(min(ig[k], P.i_shock))
            zones = [i for i in range(i_start + 1, i_stop + 1) if 1 <= i <= P.n_grid]
            eps_max = max([eps[i - 1] for i in zones], default=-1e300)
            recv_max = max([pl[i - 1] for i in zones] + [0.0])
            gam_i = float(mv.oev("hypot1", np.array([ptot[k] / mc]))[0])
            if case.aa >= 1 and eps_max > 0:
                eps_start = eps[i_start - 1] if i_start >= 1 else 0.0
                gam_f = 1 + (gam_i - 1) * (1 - eps[i_stop - 1]) / (1 - eps_start)
            elif recv_max > 0:
                tot = 0.0
                for i in range(i_start + 1, i_stop + 1):
                    tot += pl[i - 1]
                gam_f = gam_i + tot * 1.0 / E0          # (ewf = 1: Case.begin)
            else:
                continue
            pf = mc * np.sqrt(gam_f * gam_f - 1)
            sc = pf / ptot[k]
            pb[k] *= sc; pperp[k] *= sc; ptot[k] = pf; gam[k] = gam_f
            did_etf[k] = True
    if P.dont_scatter:
        leave(x > 10 * gr, 2, STAGES.index("dont_scatter"))
    near = cmp("pmax", ptot, pmax_of(case))
    psk = np.zeros(n)
    sel = np.flatnonzero(live & near)
    if len(sel):
        psk[sel] = ptot_sk_of(case, ob, pb[sel], pperp[sel], gam[sel], phi[sel], ig[sel])
    leave(near & cmp("pmax", psk, pmax_of(case)), 3, STAGES.index("pmax"))
    leave(inj & cmp("feb_up", x, P.feb_upstream, strict_gt=False), 3, STAGES.index("feb_up"))
    leave(bool(P.age_max > 0) & cmp("age", acc, P.age_max), 4, STAGES.index("age"))
    dlnp = np.zeros(n)
    if P.do_rad_losses and case.aa < 1:
        # t_step of the move: the period the scatter left over the state's xn_per
        gam_in = mv.oev("hypot1", pop.ptot_pf / mc)
        gd_in = mv.np_derive(case, pop)["gd"]
        t_step = np_period(case, pop.ptot_pf, gam_in, gd_in) / pop.xn_per
        B_CMB_loc = P.B_CMBz * tb.gef[ig]
        dlnp = RAD_LOSS_FAC * (bmag * bmag + B_CMB_loc * B_CMB_loc) * ptot * t_step
        pn = np.where(cmp("dlnp", dlnp, 1.0e-2), ptot / (1 + dlnp), ptot * (1 - dlnp))
        leave(pn <= 0, 5, STAGES.index("loss"))
        gam_n = mv.oev("hypot1", pn / mc)
        upd = live.copy()
        pb = np.where(upd, pb * (pn / ptot), pb)
        pperp = np.where(upd, pperp * (pn / ptot), pperp)
        grt = np.where(upd, pn * CC * gd, grt)
        gam = np.where(upd, gam_n, gam)
        ptot = np.where(upd, pn, ptot)
        gr = np.where(upd, pperp * CC * gd, gr)
    stage[live] = STAGES.index("save")
    saved = live & down & cmp("pcut", ptot, case.prob.pcuts[I_PCUT - 1])
    end[saved] = SAVED
    end[live & ~saved] = GOES_ON
    stage[live & ~saved] = STAGES.index("step")          # (only a particle that is not saved comes to the fine / coarse choice)
    xn = np.where(live & ~saved, np.where(cmp("grt", x, grt), P.xn_per_coarse, P.xn_per_fine), pop.xn_per)
    return dict(end=end, stage=stage, ptot=ptot, gam=gam, pb=pb, pperp=pperp, grt=grt, gr=gr, gd=gd, xn=xn, dlnp=dlnp, covered=covered,
                runs=runs, etf=etf, psk=psk, did_etf=did_etf, ptot_before_etf=ptot_before_etf, psp=psp, n_clamp=n_clamp, phi=phi)


def ptot_sk_of(case, ob, pb, pperp, gam, phi, ig):
    """the shock-frame momentum of the p_max test (particle_loop.jl:264): the oracle's transform_p_PS, state by state"""
    pr = case.prob
    cs, sn = mv.oev("cos", np.asarray(pr.theta, dtype=np.float64)), mv.oev("sin", np.asarray(pr.theta, dtype=np.float64))
    o = np.zeros(5)
    op = o.ctypes.data_as(ct.POINTER(ct.c_double))
    res = np.zeros(len(pb))
    for k in range(len(pb)):
        z = int(ig[k])
        ob.lib.orc_transform_p_PS(case.aa, float(pb[k]), float(pperp[k]), float(gam[k]), float(phi[k]), float(pr.ux[z]), float(pr.uz[z]),
                                  float(pr.utot[z]), float(pr.gam_sf[z]), float(cs[z]), float(sn[z]), op)
        res[k] = o[0]
    return res


def prp_return(case, pop, pre):
    """a PRP return (prob_return.jl:89-100, i_return = 1): the next pass is a Code Block 1 pass and no head runs.  Recognised by its effect:
    the particle sits ON its PRP beyond x_grid_stop after a move that started below it"""
    P = case.prob.params
    x, prp = pre[:, COLS["x"]], pre[:, COLS["prp"]]
    return (x == prp) & (x >= P.x_grid_stop) & (pre[:, COLS["x_old"]] < prp)


# ---- the packed word of mcs_eval_pass (include/mcs.h) ------------------------------------------------------------------------------
def unpack(word):
    w = np.asarray(word, dtype=np.uint64)

    def f(sh, bits):
        return ((w >> np.uint64(sh)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    return dict(i_grid=f(0, 8), i_grid_old=f(8, 8), ig3=f(16, 8), tcut=f(24, 8), downstream=f(32, 1), inj=f(33, 1), post_end=f(34, 3),
                pre_end=f(37, 3), f_save=f(40, 1), f_nearp=f(41, 1), helix=f(42, 14), draws=f(56, 3), n_retro=f(59, 3), ev=f(62, 1),
                ev_cross=f(63, 1))


# ---- the states ------------------------------------------------------------------------------------------------------------------
@dataclass
class States:
    pop: object
    helix: np.ndarray
    cls: np.ndarray          # class name per state
    target: np.ndarray       # the number the state aims at (nan: none)

    @property
    def n(self):
        return self.pop.n


FIELDS = ("weight", "ptot_pf", "pb_pf", "x_PT_cm", "xn_per", "prp_x_cm", "acctime_sec", "phi_rad", "tcut", "downstream", "inj")


class _Rows:
    def __init__(self, case):
        self.case, self.r, self.cls, self.target, self.helix = case, {k: [] for k in FIELDS}, [], [], []

    def add(self, cls, target=np.nan, helix=1, **kw):
        P = self.case.prob.params
        row = dict(weight=1.0 / 4096, prp_x_cm=4.0 * P.x_grid_stop, acctime_sec=0.0, phi_rad=1.0, tcut=1, downstream=0, inj=0, xn_per=None)
        row.update(kw)
        if row["xn_per"] is None:      # the step size the head would have left at the state's position
            gd = 1 / (self.case.zz * QCGS * mv.tables(self.case).bt[int(mv.zone_of(mv.tables(self.case).xg, row["x_PT_cm"]))])
            row["xn_per"] = P.xn_per_coarse if row["x_PT_cm"] > row["ptot_pf"] * CC * gd else P.xn_per_fine
        for k in FIELDS:
            self.r[k].append(row[k])
        self.cls.append(cls); self.target.append(target); self.helix.append(helix)

    def pop(self, sel=None):
        n = len(self.cls)
        sel = np.arange(n) if sel is None else sel
        pop = mcs.capi.Population(len(sel))
        for k in FIELDS:
            getattr(pop, k)[:] = np.array(self.r[k], dtype=np.float64)[sel]
        pop.grid[:] = mv.zone_of(mv.tables(self.case).xg, pop.x_PT_cm)
        return pop


def walk(v, steps=3):
    out = [v]
    lo = hi = v
    for _ in range(steps):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def _oracle(case):
    ob = oracle_backend(case.prob)
    case.begin(ob)
    ob.set_retro_cap(mv.RETRO_CAP)
    T, I = ob.read_tallies()
    T, I = seed_pool(case, ob, T, I)
    ob.write_tallies(T, I)
    return ob, (T, I)


def build_states(case, seed=11):
    P, tb, prob = case.prob.params, mv.tables(case), case.prob
    base = mv.build_states(case, seed)
    rng = np.random.default_rng(seed + 1)
    xg, xgs, ng, rg0 = tb.xg, P.x_grid_stop, P.n_grid, prob.rg0
    mc = case.aa * MP * CC
    pmax, pcut = pmax_of(case), float(prob.pcuts[I_PCUT - 1])
    nt = len(prob.tcuts)
    i0 = int(np.searchsorted(xg, 0.0))
    x_up, x_dn, x_far = 0.5 * (xg[30] + xg[31]), 0.5 * (xg[i0 + 2] + xg[i0 + 3]), 2.0 * xgs
    # (beyond the downstream FEB nothing goes on, and without scattering nothing does ten gyroradii downstream)
    spots = ((x_up, 0), (x_dn, 1)) + (() if (0 < P.feb_downstream < 1.2 * x_far or P.dont_scatter) else ((x_far, 1),))
    R = _Rows(case)
    ulp3 = lambda v: (np.nextafter(v, 0.0), v, np.nextafter(v, np.inf))

    # helix: the cap, and the electrons' % 1000 branch of prob_return beyond x_grid_stop
    for hx in (HELIX_CAP - 1, HELIX_CAP):
        for x, dn in spots:
            for fr in (-0.5, 0.5):
                R.add("helix", target=HELIX_CAP, helix=hx, ptot_pf=20.0 * mc, pb_pf=fr * 20.0 * mc, x_PT_cm=x, downstream=dn)
    if case.aa < 1:
        for hx in (999, 1000, 1001, 2000):
            for pm in (0.3, 3.0, 30.0):
                for xm in (1.5, 3.0, 3.9):
                    R.add("helix", helix=hx, ptot_pf=pm * mc, pb_pf=0.3 * pm * mc, x_PT_cm=xm * xgs, downstream=1)
    # pmax: ptot_pf around pmax_cutoff; the shock-frame momentum on both sides of it
    for pt in ulp3(pmax):
        for x, dn in spots[:2]:      # (from beyond x_grid_stop a move of such a momentum crosses the PRP logic first)
            for fr in (-0.9, -0.3, 0.3, 0.9):
                R.add("pmax_pf", target=pmax, ptot_pf=pt, pb_pf=fr * pt, x_PT_cm=x, downstream=dn, prp_x_cm=1e6 * xgs, xn_per=P.xn_per_fine)
    for eps in (-5e-2, -1e-2, -1e-3, -1e-6, 1e-6, 1e-3, 1e-2, 5e-2):
        for x, dn in ((x_up, 0), (x_dn, 1)):
            for fr in np.linspace(-0.999, 0.999, 41):
                R.add("pmax_sk", target=pmax, ptot_pf=pmax * (1 + eps), pb_pf=fr * pmax * (1 + eps), x_PT_cm=x, downstream=dn, prp_x_cm=1e6 * xgs,
                      xn_per=P.xn_per_fine)
    # ... and the pitch solved by bisection on the doubles for ptot_sk = pmax_cutoff (the restatement's ptot_sk on the state the oracle's
    # move leaves), walked over +-3 ulps: the shock-frame momentum within ulps of the cutoff on both sides
    cands = [(x, dn, pmax * (1 + eps)) for x, dn in ((x_up, 0), (x_dn, 1)) for eps in (1e-3, 1e-2)]
    ob, _ = _oracle(case)

    def psk_of(pbs):
        Q = _Rows(case)
        for (x, dn, pt), v in zip(cands, pbs):
            Q.add("pmax_sk", ptot_pf=pt, pb_pf=float(v), x_PT_cm=x, downstream=dn, prp_x_cm=1e6 * xgs, xn_per=P.xn_per_fine)
        pop = Q.pop()
        hx = np.ones(pop.n, dtype=np.int32)
        pre, wpre, _ = ob.eval_pass(pop, hx, I_PCUT, head=2, log=False)
        return np_head(case, ob, pop, hx, pre, wpre)["psk"]
    lo, hi = np.array([-0.999 * c[2] for c in cands]), np.array([0.999 * c[2] for c in cands])
    plo, phi_ = psk_of(lo), psk_of(hi)
    rising = plo <= phi_          # (with an oblique field the shock-frame momentum can fall with the pitch)
    ok = (plo > 0) & (phi_ > 0) & ((plo <= pmax) != (phi_ <= pmax))
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        up = (psk_of(mid) <= pmax) == rising
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    ob.destroy()
    for (x, dn, pt), v, good in zip(cands, hi, ok):
        if good:
            for pbv in walk(float(v)):
                R.add("pmax_sk", target=pmax, ptot_pf=pt, pb_pf=pbv, x_PT_cm=x, downstream=dn, prp_x_cm=1e6 * xgs, xn_per=P.xn_per_fine)
    # save: ptot_pf around pcut downstream and upstream; the save's clock and the time cuts
    for pt in ulp3(pcut):
        for x, dn in spots:
            for fr in (-0.9, -0.3, 0.3, 0.9):
                R.add("save", target=pcut, ptot_pf=pt, pb_pf=fr * pt, x_PT_cm=x, downstream=dn)
    for j in range(nt):
        for acc in (np.nextafter(prob.tcuts[j], 0.0), 0.5 * prob.tcuts[j]):
            R.add("save", target=pcut, ptot_pf=np.nextafter(pcut, np.inf), pb_pf=0.3 * pcut, x_PT_cm=x_dn, downstream=1, acctime_sec=acc, tcut=j + 1)
    R.add("save", target=pcut, ptot_pf=np.nextafter(pcut, np.inf), pb_pf=0.3 * pcut, x_PT_cm=x_dn, downstream=1, acctime_sec=1.0, tcut=nt + 1)
    # loss: dlnp around 1e-2, tiny and large dlnp, ptot_pf across pe_crit
    lossy = bool(P.do_rad_losses) and case.aa < 1
    if lossy:
        # (mostly upstream in the wide zones far from the shock, where a move of such a momentum stays in its zone and nothing is saved:
        # the states the LOSSY kernel's in-line path is entitled to)
        mid = lambda z: 0.5 * (xg[z] + xg[z + 1])
        places = [(mid(10), 0), (mid(20), 0), (x_up, 0), (x_dn, 1)] + ([(3.0 * xgs, 1), (30.0 * xgs, 1)] if P.use_custom_epsB else [])

        # ptot_pf solved for dlnp = 1e-2 by bisection on the doubles.  dlnp is the restatement's, on the state the oracle's move leaves
        # (the field is that of the zone, or of the position beyond x_grid_stop, the move ENDS in)
        cands = [(x, dn, xn, fr) for x, dn in places for xn in (P.xn_per_fine, P.xn_per_coarse) for fr in ((0.2, 0.6) if dn else (-0.6, 0.4))]
        ob, _ = _oracle(case)      # (downstream: away from the shock, or the move ends far upstream)

        def dlnp_of(pt):
            Q = _Rows(case)
            for (x, dn, xn, fr), v in zip(cands, pt):
                Q.add("loss", ptot_pf=float(v), pb_pf=fr * float(v), x_PT_cm=x, downstream=dn, xn_per=xn, prp_x_cm=1e6 * xgs)
            pop = Q.pop()
            hx = np.ones(pop.n, dtype=np.int32)
            pre, wpre, _ = ob.eval_pass(pop, hx, I_PCUT, head=2, log=False)
            return np_head(case, ob, pop, hx, pre, wpre)["dlnp"]
        lo, hi = np.full(len(cands), 1e-3 * mc), np.full(len(cands), 1e12 * mc)
        ok = (dlnp_of(lo) < 1e-2) & (dlnp_of(hi) > 1e-2)
        for _ in range(120):
            mid = np.sqrt(lo * hi)
            mid = np.where((mid > lo) & (mid < hi), mid, np.nextafter(lo, np.inf))
            up = dlnp_of(mid) < 1e-2
            lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
            if np.all(np.nextafter(lo, np.inf) >= hi):
                break
        ob.destroy()
        for (x, dn, xn, fr), v, good in zip(cands, hi, ok):
            if good:
                for pt in walk(float(v)):
                    R.add("loss", target=1e-2, ptot_pf=pt, pb_pf=fr * pt, x_PT_cm=x, downstream=dn, xn_per=xn, prp_x_cm=1e6 * xgs)
        for x, dn in places:
            for pm in 10 ** np.linspace(-3, 6, 19):
                R.add("loss", ptot_pf=pm * mc, pb_pf=0.4 * pm * mc, x_PT_cm=x, downstream=dn, prp_x_cm=1e6 * xgs)
            pc = P.pe_crit
            for pt in [pc, np.nextafter(pc, np.inf), np.nextafter(pc, 0.0)] + [pc * (1 + d) for d in 10 ** np.linspace(-15, -3, 13)]:
                R.add("loss", ptot_pf=pt, pb_pf=-0.4 * pt, x_PT_cm=x, downstream=dn, prp_x_cm=1e6 * xgs)
    # step / dont_scatter: x after the move on the number the head leaves.  Candidates downstream, near a gyroradius; aimed below.
    aim_cls = "dont_scatter" if P.dont_scatter else "step"
    fac = 10.0 if P.dont_scatter else 1.0
    # (step: momenta at or below this launch's pcut -- a particle above it downstream is saved before the fine / coarse choice)
    for pm in ((3.0, 20.0, 1e3) if P.dont_scatter else tuple(f * pcut / mc for f in (0.05, 0.25, 0.6, 0.95, 1.0))):
        gd = 1 / (case.zz * QCGS * tb.bt[i0 + 2])
        for fr, xn, off in ((0.5, P.xn_per_fine, 0.9), (0.9, P.xn_per_fine, 0.95), (-0.6, P.xn_per_coarse, 1.1), (-0.9, P.xn_per_coarse, 1.05)):
            g = fac * (np.sqrt(1 - fr * fr) if P.dont_scatter else 1.0) * pm * mc * CC * gd
            if P.feb_downstream > 0 and 1.3 * g > P.feb_downstream:
                continue
            R.add(aim_cls, ptot_pf=pm * mc, pb_pf=fr * pm * mc, x_PT_cm=off * g, downstream=1, xn_per=xn, prp_x_cm=1e6 * xgs, phi_rad=1.0 if fr > 0 else 4.0)

    # step_frame: (the ramp problem) a move across a downstream zone edge into a zone of another u_x, x after it on the gyro_rad_tot that
    # the frame change leaves; momenta below pcut, so that the particle goes on to the fine / coarse choice
    if case.name == "ramp":
        for j in range(i0 + 3, i0 + 16):
            gd = 1 / (case.zz * QCGS * tb.bt[j])
            pt = xg[j] * (1 + 1e-3) / (CC * gd)
            if pt <= 0.95 * pcut:
                for fr in (0.9, 0.6):
                    R.add("step_frame", ptot_pf=pt, pb_pf=fr * pt, x_PT_cm=xg[j] * (1 + 1e-3) * (1 - 4e-3), downstream=1, inj=1, xn_per=P.xn_per_fine,
                          prp_x_cm=1e6 * xgs)
    # frame: the shock crossed in both directions with p_perp = 0, |pb_pf| one ulp below ptot_pf (the clamp of transform_p_PSP and its
    # counter), and phi near 0, pi/2 and 2 pi (the result is atan2 - pi/2, not reduced)
    HALFPI = 1.5707963267948966
    for pm in (3.0, 20.0, 1e3):
        rg = pm * mc * CC / (case.zz * QCGS * tb.bt[i0])          # (a fine step is about 3e-3 gyroradii long: the move crosses the shock)
        for x, sg, inj, dn in ((-5e-5 * rg, 1.0, 0, 0), (5e-5 * rg, -1.0, 1, 1)):
            pt = pm * mc
            for pbv in (sg * pt, sg * np.nextafter(pt, 0.0), sg * pt * (1 - 1e-13)):
                R.add("frame", ptot_pf=pt, pb_pf=pbv, x_PT_cm=x, downstream=dn, inj=inj, xn_per=P.xn_per_fine)
            for ph in (0.0, 1e-300, 1e-9, np.nextafter(HALFPI, 0.0), HALFPI, np.nextafter(HALFPI, 4.0), TWOPI - 1e-9, np.nextafter(TWOPI, 0.0)):
                R.add("frame", ptot_pf=pt, pb_pf=sg * 0.9 * pt, x_PT_cm=x, downstream=dn, inj=inj, phi_rad=ph, xn_per=P.xn_per_fine)
    # etf: crossings of the last upstream zones and the shock by a particle not yet injected, with ptot_pf on either side of pcut and
    # pmax_cutoff by 1e-9 .. 0.3: transfers that take it across
    if P.energy_transfer_frac > 0:
        for T in (pcut, pmax):
            for dl in (1e-15, 1e-13, 1e-12, 1e-9, 1e-6, 1e-4, 1e-2, 0.05, 0.1, 0.3):
                for sgn in (1.0, -1.0):
                    pt = T * (1 + sgn * dl)
                    rg = pt * CC / (case.zz * QCGS * tb.bt[i0 - 1])          # (a fine step is about 3e-3 gyroradii long)
                    for x in (-2e-4 * rg, xg[i0 - 1] - 2e-4 * rg, xg[i0 - 2] - 2e-4 * rg, xg[3 * i0 // 4] - 2e-4 * rg, xg[i0 // 2 + 1] - 2e-4 * rg):      # (into the shock, into the last upstream zones, into wide zones of the precursor)
                        R.add("etf", ptot_pf=pt, pb_pf=0.6 * pt, x_PT_cm=x, downstream=0, inj=0, xn_per=P.xn_per_fine, prp_x_cm=1e6 * xgs)
        # (the frame change at the shock and the donor's transfer change ptot_pf by per cents: momenta 1.8 % apart straddle the cut after
        # them; the receiver gains a few m c^2 over a crossing: momenta below the cut by steps of 1e-4 and 1e-14)
        for T in (pcut, pmax):
            for ratio in np.geomspace(0.02, 2.5, 270):
                pt = T * ratio
                rg = pt * CC / (case.zz * QCGS * tb.bt[i0 - 1])
                R.add("etf", ptot_pf=pt, pb_pf=0.6 * pt, x_PT_cm=-2e-4 * rg, downstream=0, inj=0, xn_per=P.xn_per_fine, prp_x_cm=1e6 * xgs)
            if case.aa < 1:
                for j in range(1, 21):
                    for pt in (T * (1 - j * 1e-4), T * (1 - j * 1e-14)):
                        rg = pt * CC / (case.zz * QCGS * tb.bt[i0 - 1])
                        R.add("etf", ptot_pf=pt, pb_pf=0.6 * pt, x_PT_cm=xg[i0 - 1] - 2e-4 * rg, downstream=0, inj=0, xn_per=P.xn_per_fine, prp_x_cm=1e6 * xgs)
    # ---- aim the step / dont_scatter candidates with the oracle's own numbers, then walk them
    # feb_up: move_common's injected states at the upstream FEB, aimed again: the pass's own move is made with the scatter's gyro
    # period, whose last bit can differ from the prologue's that move_common aims with
    bsel = np.flatnonzero((base.cls == "feb_up") & (np.asarray(base.pop.inj) != 0))[::7]
    for k in bsel:
        R.add("feb_up", target=P.feb_upstream, **{f: (float if f not in ("tcut", "downstream", "inj") else int)(getattr(base.pop, f)[k]) for f in FIELDS})
    cls = np.array(R.cls)
    col = COLS["gyro_rad"] if P.dont_scatter else COLS["gyro_rad_tot"]
    for this_cls in (aim_cls, "feb_up", "step_frame"):
      sel = np.flatnonzero(cls == this_cls)
      if len(sel):
          ob, _ = _oracle(case)
          xs = np.array(R.r["x_PT_cm"], dtype=np.float64)
          for _ in range(3):
              for k, v in zip(sel, xs[sel]):
                  R.r["x_PT_cm"][k] = float(v)
              pop = R.pop(sel)
              out, word, _ = ob.eval_pass(pop, np.ones(len(sel), dtype=np.int32), I_PCUT, log=False)
              T = np.full(len(sel), P.feb_upstream) if this_cls == "feb_up" else (fac if this_cls == aim_cls else 1.0) * out[:, col]
              x_fix = xs[sel] + (T - out[:, COLS["x"]])
              ok = np.isfinite(x_fix) & (mv.zone_of(xg, x_fix) == pop.grid) & ((x_fix > 0) == (xs[sel] > 0))
              xs[sel] = np.where(ok, x_fix, xs[sel])
          ob.destroy()
          for k in sel:
              row = {f: R.r[f][k] for f in FIELDS}
              for v in walk(float(xs[k]))[1:]:
                  R.add(this_cls, target=(P.feb_upstream if this_cls == "feb_up" else np.nan), **dict(row, x_PT_cm=float(v)))
              R.r["x_PT_cm"][k] = float(xs[k])

    extra = R.pop()
    # ---- helix of move_common's states: the first pass for the crafted ones, anything up to the cap for the fuzzed ones
    hx0 = np.ones(base.n, dtype=np.int32)
    fz = base.cls == "fuzz"
    hx0[fz] = rng.integers(1, HELIX_CAP + 1, int(fz.sum()))
    hx0[fz & (rng.random(base.n) < 0.02)] = HELIX_CAP
    n = base.n + extra.n
    pad = 1 if n % 256 == 0 else 0
    pop = mcs.capi.Population(n + pad)
    for f in pop.fields():
        a = getattr(pop, f)
        a[:base.n] = getattr(base.pop, f)
        a[base.n:n] = getattr(extra, f)
        if pad:
            a[n:] = getattr(base.pop, f)[:1]
    S = States(pop, np.concatenate([hx0, np.array(R.helix, dtype=np.int32), hx0[:pad]]).astype(np.int32),
               np.concatenate([base.cls, np.array(R.cls), base.cls[:pad]]), np.concatenate([base.target, np.array(R.target, dtype=np.float64), base.target[:pad]]))
    assert S.n % 256 != 0
    for f in pop.fields():
        getattr(pop, f).setflags(write=False)
    S.helix.setflags(write=False)
    return S


def reference(case, S):
    """The oracle's pass (with the deposit log), the state the move left (head skipped), and the numpy restatement -> dict"""
    ob, start = _oracle(case)
    pre, wpre, _ = ob.eval_pass(S.pop, S.helix, I_PCUT, head=2, log=False)
    ob.write_tallies(*start)
    out, word, log = ob.eval_pass(S.pop, S.helix, I_PCUT)
    T1, I1 = ob.read_tallies()
    pool = np.array(ob.layout.view(start[0], "energy_recv_pool"))
    np_ = np_head(case, ob, S.pop, S.helix, pre, wpre, pool=pool)
    m = dict(pool=pool, case=case, S=S, out=out, word=word, log=log, pre=pre, wpre=wpre, np=np_, start=start, end_tallies=(T1, I1), layout=ob.layout)
    ob.destroy()
    for v in list(m.values()) + list(np_.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return m


def wp_inj(m):
    return unpack(m["wpre"])["inj"]


def check_states(case, S, m):
    """The builder's own assertions, from the reference alone -> {class: (states, below, on, above, share that reached its branch)}"""
    P = case.prob.params
    r, w = m["np"], unpack(m["word"])
    out = m["out"]
    probe = dict(helix=S.helix.astype(np.float64), pmax_pf=np.asarray(S.pop.ptot_pf), pmax_sk=r["psk"], save=np.asarray(S.pop.ptot_pf), loss=r["dlnp"],
                 step=out[:, COLS["x"]] - out[:, COLS["gyro_rad_tot"]], dont_scatter=out[:, COLS["x"]] - 10 * out[:, COLS["gyro_rad"]],
                 feb_up=out[:, COLS["x"]], tcut=np.asarray(S.pop.acctime_sec))
    counts = {}
    for c in np.unique(S.cls):
        sel = S.cls == c
        T = S.target[sel]
        if c in ("step", "dont_scatter"):
            T = np.zeros(int(sel.sum()))
        v = probe[c][sel] if c in probe else np.full(int(sel.sum()), np.nan)
        if c == "step":          # (below / on / above among the states that take the branch)
            went = w["pre_end"][sel] == GOES_ON
            T, v = T[went], v[went]
        with np.errstate(invalid="ignore"):
            below, on, above = int((v < T).sum()), int((v == T).sum()), int((v > T).sum())
        reach = 1.0
        if c in CLASS_STAGE:
            reach = float((r["stage"][sel] >= STAGES.index(CLASS_STAGE[c])).mean())
            assert reach >= 0.9, f"{case.name}: only {reach:.0%} of class {c} reaches the {CLASS_STAGE[c]} test"
            need_on = c not in ("loss", "pmax_sk")      # (computed numbers: no double need sit ON 1e-2 or on pmax_cutoff)
            if c == "helix":      # (a count above the cap is no state: the pass that would carry it never starts)
                assert below > 0 and on > 0, f"{case.name}: class helix has {below} states below the cap and {on} on it"
            elif not np.all(np.isnan(S.target[sel])) or c in ("step", "dont_scatter"):
                assert below > 0 and above > 0 and (on > 0 or not need_on), f"{case.name}: class {c} has {below} states below, {on} on and {above} above"
        counts[str(c)] = (int(sel.sum()), below, on, above, round(reach, 3))
    want = {"helix", "pmax_pf", "pmax_sk", "save"} | ({"loss"} if (P.do_rad_losses and case.aa < 1) else set()) | ({"dont_scatter"} if P.dont_scatter else {"step"})
    assert want <= set(counts), f"{case.name}: no states for {sorted(want - set(counts))}"
    # helix: the electrons' `% 1000` branch of prob_return moves the PRP for counts 1000 and 2000, and leaves it for 999 and 1001
    if case.aa < 1:
        hx_cls = (S.cls == "helix") & (np.asarray(S.pop.x_PT_cm) >= P.x_grid_stop)
        prp_moved = out[:, COLS["prp"]] != np.asarray(S.pop.prp_x_cm)
        on = hx_cls & np.isin(S.helix, (1000, 2000))
        off = hx_cls & np.isin(S.helix, (999, 1001))
        assert (on & prp_moved).sum() >= 2 and not (off & prp_moved).any() and off.sum() >= 6, \
            f"{case.name}: prp moved in {int((on & prp_moved).sum())} of {int(on.sum())} states with helix 1000 / 2000 and in {int((off & prp_moved).sum())} with 999 / 1001"
        counts["helix_mod_1000"] = (int((on & prp_moved).sum()), int(on.sum()))
    # pmax_sk: the shock-frame momentum within 4 ulps of pmax_cutoff on either side, among the states that reach the comparison
    pm_ = pmax_of(case)
    sk = r["psk"][(S.cls == "pmax_sk") & (r["psk"] > 0)]
    near_sk = (int(((sk <= pm_) & (sk >= pm_ - 4 * np.spacing(pm_))).sum()), int(((sk > pm_) & (sk <= pm_ + 4 * np.spacing(pm_))).sum()))
    # (oblique field: the bisection on the pitch does not converge to the cutoff -- the move and the phase change with it; reported only)
    assert all(near_sk) or not mv.parallel(case), f"{case.name}: states with ptot_sk within 4 ulps of pmax_cutoff at or below / above it: {near_sk}"
    counts["pmax_sk_within_4_ulps"] = near_sk
    # age: acctime one ulp below, on and one ulp above age_max among the states that reach the comparison (the clock of the pass that
    # follows has not run yet)
    if P.age_max > 0:
        at = r["stage"] >= STAGES.index("age")
        acc = m["pre"][:, COLS["acctime"]]
        age = tuple(int((at & (acc == v)).sum()) for v in (np.nextafter(P.age_max, 0.0), P.age_max, np.nextafter(P.age_max, np.inf)))
        assert all(age), f"{case.name}: states one ulp below / on / one ulp above age_max at the comparison: {age}"
        counts["age"] = age
    # step_frame: the fine / coarse choice after a frame change, among the states that go on
    if case.name == "ramp":
        sf = (S.cls == "step_frame") & r["psp"] & (w["pre_end"] == GOES_ON)
        dx_ = out[:, COLS["x"]] - out[:, COLS["gyro_rad_tot"]]
        moved = u64(out[:, COLS["gyro_rad_tot"]]) != u64(m["pre"][:, COLS["gyro_rad_tot"]])
        step_frame = (int((S.cls == "step_frame").sum()), int((sf & moved & (dx_ < 0)).sum()), int((sf & moved & (dx_ == 0)).sum()), int((sf & moved & (dx_ > 0)).sum()))
        assert step_frame[1] > 0 and step_frame[2] > 0 and step_frame[3] > 0 and sf.sum() >= 0.9 * step_frame[0], f"ramp: step_frame {step_frame}"
        counts["step_frame"] = step_frame
    # feb_up: x one ulp below, on and one ulp above feb_upstream among the injected states that reach the comparison
    at = (r["stage"] >= STAGES.index("feb_up")) & (wp_inj(m) != 0)
    xs = m["pre"][:, COLS["x"]]
    feb = tuple(int((at & (xs == v)).sum()) for v in (np.nextafter(P.feb_upstream, -np.inf), P.feb_upstream, np.nextafter(P.feb_upstream, np.inf)))
    assert all(feb), f"{case.name}: injected states one ulp below / on / one ulp above feb_upstream at the comparison: {feb}"
    counts["feb_up_inj"] = feb
    # frame: heads with a frame change -- over 1, 2, 3 and dozens of zones, the shock both ways, phi near 0, pi/2, 2 pi, p_perp = 0
    tb = mv.tables(case)
    wp = unpack(m["wpre"])
    fr = r["psp"]
    span = np.abs(wp["i_grid"] - np.asarray(S.pop.grid, dtype=np.int64))
    xo, xn_ = m["pre"][:, COLS["x_old"]], m["pre"][:, COLS["x"]]
    sel = S.cls == "frame"
    frame = dict(heads=int(fr.sum()), zones_2=int((fr & (span == 2)).sum()), zones_3=int((fr & (span == 3)).sum()), zones_12_up=int((fr & (span >= 12)).sum()),
                 shock_down=int((fr & (xo < 0) & (xn_ >= 0)).sum()), shock_up=int((fr & (xo > 0) & (xn_ < 0)).sum()),
                 p_perp_0=int((fr & sel & (np.abs(S.pop.pb_pf) == S.pop.ptot_pf)).sum()), clamps=int(r["n_clamp"].sum()),
                 reach=round(float(fr[sel].mean()), 3))
    assert frame["heads"] > 100 and frame["shock_down"] > 20 and frame["shock_up"] > 10 and frame["p_perp_0"] >= 4, f"{case.name}: frame {frame}"
    assert frame["reach"] >= 0.9, f"{case.name}: only {frame['reach']:.0%} of class frame changes frame"
    if len(np.unique(tb.ux[:len(tb.xg) - 1][tb.xg[:-1] < 0])) > 2:          # (a precursor: frame changes upstream too)
        assert frame["zones_2"] > 0 and frame["zones_3"] > 0 and frame["zones_12_up"] > 0, f"{case.name}: frame {frame}"
    for ph in (0.0, 1.5707963267948966, np.nextafter(TWOPI, 0.0)):
        assert (fr & sel & (S.pop.phi_rad == ph)).sum() >= 2, f"{case.name}: no frame change with phi = {ph}"
    counts["frame"] = frame
    # etf: transfers made, those that take ptot_pf across pcut and pmax_cutoff, and for the receiver the three kinds of range
    if P.energy_transfer_frac > 0:
        d, a, b = r["did_etf"], r["ptot_before_etf"], r["ptot"]
        pcut, pmax = float(case.prob.pcuts[I_PCUT - 1]), pmax_of(case)
        sel = S.cls == "etf"
        due = r["etf"] & r["runs"]
        etf = dict(due=int(due.sum()), made=int(d.sum()), across_pcut=int((d & ((a > pcut) != (b > pcut))).sum()),
                   across_pmax=int((d & ((a > pmax) != (b > pmax))).sum()), reach=round(float(due[sel].mean()), 3),
                   x_old_neg=int((due & (xo < 0)).sum()), x_old_zero=int((due & (xo == 0)).sum()), from_zone_0=int((due & (wp["i_grid_old"] == 0)).sum()),
                   over_shock=int((due & (wp["i_grid"] > P.i_shock)).sum()), upstream_ward=int((due & (wp["i_grid"] < wp["i_grid_old"])).sum()))
        if case.aa < 1:
            kinds = [0, 0, 0]
            for k in np.flatnonzero(due):
                z = [m["pool"][i - 1] > 0 for i in range(int(wp["i_grid_old"][k]) + 1, int(min(wp["i_grid"][k], P.i_shock)) + 1) if 1 <= i <= P.n_grid]
                if z:
                    kinds[0 if not any(z) else (2 if all(z) else 1)] += 1
            etf["pool_none_some_all"] = tuple(kinds)
            assert all(kinds), f"{case.name}: receiver ranges with no / some / only non-zero pool entries: {kinds}"
        # (across pcut: the etf_donor problem's, whose transfers far from the shock come without the frame change that lifts a crossing
        # particle above this launch's pcut; across pmax_cutoff: the donors', whose transfer is per cents -- the receiver's gain of a few
        # m c^2 at pmax_cutoff is below the spacing of the scan.  Both counts are reported.)
        assert etf["made"] > 20 and etf["reach"] >= 0.9 and (case.aa < 1 or etf["across_pmax"] > 0), f"{case.name}: etf {etf}"
        etf["without_frame_change"] = int((d & ~r["psp"]).sum())
        if case.name == "etf_recv":
            assert etf["across_pcut"] > 0 and etf["across_pmax"] > 0, f"{case.name}: etf {etf}"
        if case.name == "etf_donor":          # (transfers far from the shock: no frame change raises the refresh flags for them; and across pcut)
            assert etf["without_frame_change"] > 100 and etf["across_pcut"] > 0, f"{case.name}: etf {etf}"
        assert etf["x_old_neg"] > 100 and etf["x_old_zero"] > 0 and etf["upstream_ward"] > 0 and etf["over_shock"] > 0, f"{case.name}: etf {etf}"
        counts["etf"] = etf
    # every end the head has, by the reference: saved, the four reasons where the problem can produce them
    ends = {int(e): int((w["pre_end"] == e).sum()) for e in np.unique(w["pre_end"])}
    assert ends.get(GOES_ON, 0) > 500 and ends.get(SAVED, 0) > 20 and ends.get(2, 0) >= 6 and ends.get(3, 0) > 20, f"{case.name}: ends {ends}"
    if P.age_max > 0:
        assert ends.get(4, 0) >= 1, f"{case.name}: no state aged out in the head: {ends}"
    counts["ends"] = ends
    return counts


def describe(S, k):
    p = S.pop
    return (f"state {k} ({S.cls[k]}, target {float(S.target[k]).hex()}, helix {int(S.helix[k])}): x {float(p.x_PT_cm[k]).hex()} ptot "
            f"{float(p.ptot_pf[k]).hex()} pb {float(p.pb_pf[k]).hex()} xn {p.xn_per[k]:g} prp {float(p.prp_x_cm[k]).hex()} acctime "
            f"{float(p.acctime_sec[k]).hex()} phi {float(p.phi_rad[k]).hex()} weight {float(p.weight[k]).hex()} grid {int(p.grid[k])} tcut "
            f"{int(p.tcut[k])} downstream {int(p.downstream[k])} inj {int(p.inj[k])}")


# ---- transform_p_PSP at 50 digits ----------------------------------------------------------------------------------------------------
def psp_cases(case, S, pre, wpre, limit=700):
    """The frame changes the states of a problem make: (pb, p_perp, gam, phi) after the move, the zone left and the zone entered, for
    every state whose head transforms (another zone with another u_x) -> list of (pb, pperp, gam, phi, old6, new6); old6 / new6 are
    (ux, uz, utot, gam_sf, cos theta_B, sin theta_B) as doubles."""
    pr = case.prob
    w = unpack(wpre)
    ig, io = w["i_grid"], np.asarray(S.pop.grid, dtype=np.int64)
    cs, sn = mv.oev("cos", np.asarray(pr.theta, dtype=np.float64)), mv.oev("sin", np.asarray(pr.theta, dtype=np.float64))
    sel = np.flatnonzero((w["post_end"] == 7) & (np.asarray(pr.ux)[ig] != np.asarray(pr.ux)[io]))
    if len(sel) > limit:
        sel = sel[np.linspace(0, len(sel) - 1, limit).astype(np.int64)]
    six = lambda z: tuple(float(v) for v in (pr.ux[z], pr.uz[z], pr.utot[z], pr.gam_sf[z], cs[z], sn[z]))
    return [(float(pre[k, COLS["pb_pf"]]), float(pre[k, COLS["p_perp"]]), float(pre[k, COLS["gam_pf"]]), float(pre[k, COLS["phi"]]), six(io[k]), six(ig[k]))
            for k in sel]


def psp_oracle(case, ob, pb, pperp, gam, phi, old6, new6):
    """the oracle's transform_p_PSP -> (ptot_pf, pb_pf, p_perp, gam_pf, phi)"""
    dp = ct.POINTER(ct.c_double)
    o, n, out = np.array(old6), np.array(new6), np.zeros(6)
    ob.lib.orc_transform_p_PSP(ob.h, case.aa, pb, pperp, gam, phi, o.ctypes.data_as(dp), n.ctypes.data_as(dp), out.ctypes.data_as(dp))
    return tuple(float(v) for v in out[:5])


def psp_mp(aa, pb, pperp, gam, phi, old6, new6):
    """transformers.jl:523-607 at 50 digits, from the same double inputs: plasma frame of the zone left -> shock frame -> plasma frame
    of the zone entered -> (ptot_pf, pb_pf, p_perp / ptot_pf, phi) as mpf.  (The clamp of |pb| > ptot is rounding's and has no place here.)"""
    import mpmath as mp
    mp.mp.dps = 50
    f = mp.mpf
    m = f(aa) * f(MP)
    mc = m * f(CC)
    pb, pperp, gam, phi = f(pb), f(pperp), f(gam), f(phi)
    uxo, uzo, uto, gso, bco, bso = (f(v) for v in old6)
    ux, uz, ut, gs, bc, bs = (f(v) for v in new6)
    phi_p = phi + mp.pi / 2
    ppc = pperp * mp.cos(phi_p)
    x, y, z = pb * bco - ppc * bso, pperp * mp.sin(phi_p), pb * bso + ppc * bco
    sx = ((gso - 1) * (uxo / uto) ** 2 + 1) * x + (gso - 1) * (uxo * uzo / uto ** 2) * z + gso * gam * m * uxo
    sz = (gso - 1) * (uxo * uzo / uto ** 2) * x + ((gso - 1) * (uzo / uto) ** 2 + 1) * z + gso * gam * m * uzo
    psk = mp.sqrt(sx * sx + y * y + sz * sz)
    gsk = mp.sqrt(1 + (psk / mc) ** 2)
    px = ((gs - 1) * (ux / ut) ** 2 + 1) * sx + (gs - 1) * (ux * uz / ut ** 2) * sz - gs * gsk * m * ux
    pz = (gs - 1) * (ux * uz / ut ** 2) * sx + ((gs - 1) * (uz / ut) ** 2 + 1) * sz - gs * gsk * m * uz
    ptot = mp.sqrt(px * px + y * y + pz * pz)
    pbn = px * bc + pz * bs
    phin = mp.atan2(y, -px * bs + pz * bc) - mp.pi / 2
    return ptot, pbn, mp.sqrt(max(ptot * ptot - pbn * pbn, 0)) / ptot, phin
