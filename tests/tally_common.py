"""Tally records for mcs_eval_tally / orc_eval_tally: the problems, the record sets, and the expected buffers from the oracle's log.

A record is what the transport kernel hands to its tally code: eight doubles (pb_pf, p_perp, ptot_pf, gam_pf, phi, weight, x, x_old) and
a packed word (i_grid | i_grid_old << 8 | ig3 << 16 | inj << 24 | aux << 32 | kind << 40; include/mcs.h).  The oracle walks the same
records serially and logs every deposit (record, buffer, offset, value), so for every cell of the fp64 and int64 tallies the list of
terms and the records behind them are known.  expected() turns that into the per-cell rule of the GPU test:

    no term        the cell keeps its bits
    one term       fl(before + term), bit for bit
    k > 1 terms    |device - sum| <= (K - 1) u S / (1 - (K - 1) u),  u = 2^-53, K the number of non-zero summands (the terms, and the
                   cell's value before the launch where that is not zero), S the sum of their magnitudes, `sum` the exact sum of the
                   logged terms, correctly rounded.

The bound is the classical a-priori one for a sum of K floating-point numbers taken in ANY order and ANY grouping (Higham, Accuracy
and Stability of Numerical Algorithms, 2nd ed., section 4.2: every partial sum commits one rounding error of relative size at most u,
and a term passes through at most K - 1 of them: gamma_{K-1} times the sum of magnitudes).  It is derived, not measured, and it covers
the wave butterfly of drain_events, the LDS staging and its flush, the replicas and their fold, and the order of the atomics.
It is a statement about a floating-point sum and the EXACT one.  Two floating-point sums of the same terms, the device's and the
oracle's serial one, may differ by twice as much, and do: on the MI355X pxx_flux[16] of the "general2" problem (its value before
and three terms, K = 4) came out 2 ulp = 0x1p-45 from the serial sum, with the bound at 0x1.d0fa93153865ep-46, while both lie within
the bound of the exact sum.  So the reference of a cell with several terms is the exact sum of the logged terms (math.fsum); a cell
with one term needs no such care, fl(before + term) being the serial sum and the exact one rounded at once.

So that most histogram deposits are in the bit-exact class, split() deals the records of a set into launches in which no cell of the
histograms (HIST) receives two deposits; the crafted stack shapes (same-bin batches) are exempt by design.
"""
import ctypes as ct
import math
from dataclasses import dataclass, field

import numpy as np

from conftest import mcs, make_problem, fuzz_problem, oracle_backend

U = 2.0 ** -53
KIND_IDLE, KIND_CROSS, KIND_FINISH, KIND_TCUT = 0, 1, 2, 3
HIST = ("psd", "therm_sf", "therm_pf", "esc_psd_up", "esc_psd_down", "spectra_sf", "spectra_pf", "spectra_coupled")
MP, ME, CC, QCGS = mcs.constants.MP, mcs.constants.ME, mcs.constants.C, 4.803204712570263e-10
SPIKE_AWAY, E_REL_PT, PSD_MAX, NA_C = 1000.0, 0.005, 200, 100
IC_MOMBIN_CLAMP = 5          # enum of include/mcs.h, offset from n_grid in the int64 tallies
PROBLEMS = ("protons", "general2", "oblique", "electrons", "nothermal")


def pack(i_grid, i_grid_old, ig3, inj, aux, kind):
    return np.uint64(int(i_grid) | int(i_grid_old) << 8 | int(ig3) << 16 | int(bool(inj)) << 24 | int(aux) << 32 | int(kind) << 40)


@dataclass
class Case:
    """A problem and the species the records belong to."""
    name: str
    prob: object
    i_ion: int
    aa: float
    zz: float
    start: tuple = None      # (T, I) of a fresh context after begin(): set by whoever needs a common starting state

    def begin(self, be):
        sp = self.prob.cfg.species[self.i_ion - 1]
        pmax = mcs.inputs.get_pmax_cutoff(self.prob.Emax_keV, self.prob.Emax_per_aa_keV, self.prob.pmax, sp.aa)
        be.begin_iteration(1)
        be.begin_species(1, self.i_ion, sp.aa, abs(sp.zz), pmax, sp.density, 1.0)


def make_case(name):
    if name == "protons":
        return Case(name, make_problem(64), 1, 1.0, 1.0)
    if name == "nothermal":
        return Case(name, make_problem(64, track_thermal=False), 1, 1.0, 1.0)
    if name == "general2":       # the "general" mix of fuzz_problem with detectors, run as its second species: non-zero per-ion offsets
        kw = dict(species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(4.0, 2.0, 1e6, 0.1)], energy_transfer_frac=0.1,
                  FEB_downstream=(30.0, 0.0), INJFR=[0.7, 1.0], maximum_energy=(0.0, 0.0, 1e3))
        rg0 = make_problem(64, **kw).rg0
        prob = make_problem(64, XSPEC=tuple(x * rg0 for x in (-0.5, 0.05, 2.0)), **kw)
        assert len(prob.x_spec) == 3 and len(prob.tcuts) > 0
        return Case(name, prob, 2, 4.0, 2.0)
    if name == "oblique":
        prob, aa = fuzz_problem("oblique", 64)
        return Case(name, prob, 1, aa, 1.0)
    if name == "electrons":
        prob, aa = fuzz_problem("electrons", 64)
        assert aa < 1
        return Case(name, prob, 1, aa, 1.0)
    raise KeyError(name)


@dataclass
class Records:
    rows: list = field(default_factory=list)
    words: list = field(default_factory=list)
    tags: list = field(default_factory=list)

    def add(self, tag, kind, pb=0.0, p_perp=0.0, ptot=0.0, gam=1.0, phi=0.0, w=1.0, x=0.0, x_old=0.0, i_grid=0, i_grid_old=0, ig3=0, inj=0, aux=0):
        self.rows.append((pb, p_perp, ptot, gam, phi, w, x, x_old))
        self.words.append(pack(i_grid, i_grid_old, ig3, inj, aux, kind))
        self.tags.append(tag)
        return len(self.rows) - 1

    def arrays(self):
        return np.array(self.rows, dtype=np.float64).reshape(-1, 8), np.array(self.words, dtype=np.uint64)

    def __len__(self):
        return len(self.rows)


def describe(row, word, tag=""):
    w = int(word)
    kind = (w >> 40) & 0xff
    names = ("pb_pf", "p_perp", "ptot_pf", "gam_pf", "phi", "weight", "x", "x_old")
    vals = ", ".join(f"{n}={float(v).hex()}" for n, v in zip(names, row))
    return (f"[{tag}] kind {kind} i_grid {w & 0xff} i_grid_old {(w >> 8) & 0xff} ig3 {(w >> 16) & 0xff} inj {(w >> 24) & 1} "
            f"aux {(w >> 32) & 0xff}: {vals}")


# ---- searching the inputs that straddle an edge -----------------------------------------------------------------------------------
def refine(f, a, fa, b, fb, out, tiny=0.0):
    """Every place in [a, b] where f changes between ADJACENT doubles (or doubles no further apart than `tiny`: an angle that changes
    sign need not be followed into the subnormals), by bisection on the doubles: (lo, hi, f(lo), f(hi))."""
    if fa == fb:
        return
    m = a + (b - a) / 2
    if m == a or m == b or b - a <= tiny:
        out.append((a, b, fa, fb))
        return
    fm = f(m)
    refine(f, a, fa, m, fm, out, tiny)
    refine(f, m, fm, b, fb, out, tiny)


def changes(f, grid, tiny=0.0):
    out, prev, fprev = [], None, None
    for t in grid:
        ft = f(t)
        if prev is not None:
            refine(f, prev, fprev, t, ft, out, tiny)
        prev, fprev = t, ft
    return out


def ladder(lo, hi):
    """The doubles either side of a change between lo and hi = nextafter(lo): two on each side, single ulps apart."""
    return [math.nextafter(lo, -math.inf), lo, hi, math.nextafter(hi, math.inf)]


class Probe:
    """The oracle's transform and bin functions on one state at a time (a context of its own: the probes bump its clamp counter)."""

    def __init__(self, case):
        self.case, self.P, self.prob = case, case.prob.params, case.prob
        self.ob = oracle_backend(case.prob)
        case.begin(self.ob)
        self.lib, self.h = self.ob.lib, self.ob.h
        self._o5 = np.zeros(5)
        self._o5p = self._o5.ctypes.data_as(ct.POINTER(ct.c_double))
        self._cs = {}

    def sk(self, z, pb, p_perp, gam, phi):
        pr, o = self.prob, self._o5
        self.lib.orc_transform_p_PS(self.case.aa, pb, p_perp, gam, phi, float(pr.ux[z]), float(pr.uz[z]), float(pr.utot[z]), float(pr.gam_sf[z]),
                                    self.cos_th(z), self.sin_th(z), self._o5p)
        return float(o[0]), float(o[1]), float(o[2]), float(o[3]), float(o[4])      # ptot_sk, px, py, pz, gam_sk

    def cos_th(self, z):
        if z not in self._cs:
            self._cs[z] = (float(self.ob_eval("cos", self.prob.theta[z])), float(self.ob_eval("sin", self.prob.theta[z])))
        return self._cs[z][0]

    def sin_th(self, z):
        self.cos_th(z)
        return self._cs[z][1]

    def ob_eval(self, fn, x):
        a, out = np.array([float(x)]), np.zeros(1)
        dp = ct.POINTER(ct.c_double)
        assert self.lib.orc_eval_fn(mcs.capi.FN[fn], 1, a.ctypes.data_as(dp), a.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
        return out[0]

    def bin_mom(self, p):
        return int(self.lib.orc_bin_momentum(self.h, float(p)))

    def bin_ang(self, px, p):
        return int(self.lib.orc_bin_angle(self.h, float(px), float(p)))


# ---- the record sets --------------------------------------------------------------------------------------------------------------
def zone_classes(P):
    ng = P.n_grid
    return sorted({0, 1, max(P.i_grid_feb - 1, 1), P.i_grid_feb, P.i_grid_feb + 1, P.i_shock, P.i_shock + 1, ng - 1, ng, ng + 1})


def build_records(case):
    """-> (Records, info): every record set of the issue for one problem, in one pool; info holds what the host tests assert on
    (the ladders with the edge each must straddle, the records whose value is known exactly, the branch cases)."""
    P, prob, aa = case.prob.params, case.prob, case.aa
    ng, m, mc = P.n_grid, aa * MP, aa * MP * CC
    pr = Probe(case)
    R = Records()
    info = dict(ladders=[], direct=[], branches={}, sk=[])
    rng = np.random.default_rng(20240607)
    xg = prob.x_grid_cm
    x_far_old, x_far = 5.0 * prob.rg0, 6.0 * prob.rg0           # a downstream-going move beyond every detector and the upstream FEB
    zone_ctr = [0]
    z_up, z_dn = max(P.i_grid_feb + 5, 2), min(P.i_shock + 5, ng)
    n_tc = len(prob.tcuts)

    def variants(tag, z, pb, p_perp, ptot, gam, phi, w):
        """One state through the four users of the shock-frame bins: an injected and a thermal one-zone crossing (each into a zone
        of its own), a downstream and an upstream exit."""
        ids = []
        for inj in (1, 0):
            zone_ctr[0] = zone_ctr[0] % ng + 1
            i = zone_ctr[0]
            ids.append(R.add(tag, KIND_CROSS, pb, p_perp, ptot, gam, phi, w, x_far, x_far_old, i, i - 1, z, inj))
        for reason in (1, 2):
            ids.append(R.add(tag, KIND_FINISH, pb, p_perp, ptot, gam, phi, w, ig3=z, aux=reason))
        return ids

    # -- momentum edges, controlled directly: the time cut, and the plasma-frame spectrum at a detector crossing
    bpd, nm = P.psd_bins_per_dec_mom, P.num_psd_mom_bins
    vals = []
    for k in range(0, nm + 2):
        e = P.psd_mom_min * 10.0 ** (k / bpd)
        vals += [(k, v) for v in (math.nextafter(math.nextafter(e, 0), 0), math.nextafter(e, 0), e, math.nextafter(e, math.inf),
                                  math.nextafter(math.nextafter(e, math.inf), math.inf))]
    vals += [(-1, P.psd_mom_min * 0.5), (-1, P.psd_mom_min * 1e-3), (-1, math.nextafter(P.psd_mom_min, 0)),
             (nm + 5, P.psd_mom_min * 10.0 ** ((nm + 5) / bpd)), (nm + 40, P.psd_mom_min * 10.0 ** ((nm + 40) / bpd))]
    q_span = math.log10(P.psd_mom_min * 10.0 ** (nm / bpd) / (mc * 10.0 ** 0.5)) - 0.3       # up to just below the clamp
    for j, (k, v) in enumerate(vals):
        w = 0.5 + (j % 7) / 8.0
        if n_tc:
            info["direct"].append((R.add(f"tcut edge {k}", KIND_TCUT, ptot=v, w=w, aux=1 + j % n_tc), v, "spectra_coupled"))
        if len(prob.x_spec):
            d = j % len(prob.x_spec)
            xs = float(prob.x_spec[d])
            # x == x_spec exactly counts as crossed going downstream; x_old == x_spec exactly counts for neither direction
            # (the plasma-frame bin is that of ptot_pf itself; pb, p_perp and gam_pf only place the shock-frame deposit, spread over the bins)
            q = mc * 10.0 ** (0.5 + q_span * j / len(vals))
            info["direct"].append((R.add(f"detector {d} edge {k}", KIND_CROSS, 0.3 * q, 0.9 * q, v, math.hypot(q / mc, 1), 0.7, w,
                                         xs, math.nextafter(xs, -math.inf), z_dn, z_dn, z_dn, 1), v, "spectra_pf"))
    if len(prob.x_spec):
        xs = float(prob.x_spec[0])
        v = 10.0 * mc
        info["branches"]["x_old == x_spec: no deposit"] = [
            R.add("x_old == x_spec upstream-going", KIND_CROSS, -0.3 * v, 0.9 * v, v, math.hypot(v / mc, 1), 0.7, 1.0, math.nextafter(xs, -math.inf), xs, z_dn, z_dn, z_dn, 0),
            R.add("x_old == x_spec downstream-going", KIND_CROSS, 0.3 * v, 0.9 * v, v, math.hypot(v / mc, 1), 0.7, 1.0, math.nextafter(xs, math.inf), xs, z_dn, z_dn, z_dn, 0)]
        info["branches"]["x == x_spec upstream-going: deposit"] = [
            R.add("x == x_spec upstream-going", KIND_CROSS, -0.3 * v, 0.9 * v, v, math.hypot(v / mc, 1), 0.7, 1.0, xs, math.nextafter(xs, math.inf), z_dn, z_dn, z_dn, 0)]

    # -- the angle, through transform_p_PS: the state's direction swept round the x-z plane (phi_p = 0 or pi, so p_y ~ 0): every edge of
    # bin_angle is crossed twice; the first crossing of each is kept
    p_a = 1.0e3 * mc
    g_a = math.hypot(p_a / mc, 1)

    def st_angle(al):
        return p_a * math.cos(al), p_a * abs(math.sin(al)), g_a, (-math.pi / 2 if math.sin(al) >= 0 else math.pi / 2)

    def f_angle(al):
        pb, pp, g, ph = st_angle(al)
        s = pr.sk(z_up, pb, pp, g, ph)
        return pr.bin_ang(s[1], s[0])

    def tighten(lo, hi, blo):
        """Adjacent doubles of the direction still leave p_cos several ulps apart.  From the state at `lo` to the one at `hi` first
        p_perp changes, then pb: the bin changes on one of the two legs, and a bisection on the doubles of THAT input finds two
        states one ulp of one input apart with different bins -- as near the edge as an input can be put.  -> the ladder: those two
        and their neighbours on either side, single ulps of that input apart."""
        (pb0, pp0, g, ph0), (pb1, pp1, _, ph1) = st_angle(lo), st_angle(hi)
        if ph0 != ph1:
            return [st_angle(al) for al in ladder(lo, hi)]
        f2 = lambda pb, pp: pr.bin_ang(*pr.sk(z_up, pb, pp, g, ph0)[1::-1])
        if f2(pb0, pp1) != blo:
            leg, a, b = (lambda v: (pb0, v)), pp0, pp1
        else:
            leg, a, b = (lambda v: (v, pp1)), pb0, pb1
        out = []
        refine(lambda v: f2(*leg(v)), a, f2(*leg(a)), b, f2(*leg(b)), out)
        v0, v1 = out[0][0], out[0][1]
        away0, away1 = (-math.inf, math.inf) if v1 > v0 else (math.inf, -math.inf)
        return [leg(v) + (g, ph0) for v in (math.nextafter(v0, away0), v0, v1, math.nextafter(v1, away1))]

    grid = [float(t) for t in np.linspace(-math.pi, math.pi, 4001)]
    # (the directions along +-x, where p_z changes sign, are grid points: the log-theta bins next to them are narrower than the grid)
    for lo, hi, _, _ in changes(lambda al: int(pr.sk(z_up, *st_angle(al))[3] > 0), grid[::100], 1e-25):
        grid += [lo, hi]
    seen = set()
    for lo, hi, blo, bhi in changes(f_angle, sorted(grid), 1e-25):
        key = (min(blo, bhi), max(blo, bhi))
        if key in seen:
            continue
        seen.add(key)
        ids = []
        for pb, pp, g, ph in tighten(lo, hi, blo):
            ids += variants(f"angle edge {key}", z_up, pb, pp, p_a, g, ph, 1.0 + 0.25 * (len(ids) % 3))
        info["ladders"].append(("angle", key, ids))

    # -- the shock-frame momentum: p_x and p_z cancelled (the plasma-frame momentum in the x-z plane is -gam m u_x along x), p_y = t swept
    # over the whole range, so that p_tot_sk = t up to a rounding residue far below psd_mom_min
    g_m = 1.0
    gmu = g_m * m * float(prob.ux[z_dn])
    q_m = gmu * pr.sin_th(z_dn)

    def st_mom(t):
        return -gmu * pr.cos_th(z_dn), math.hypot(q_m, t), g_m, math.atan2(t, q_m) - math.pi / 2

    def f_mom(t):
        pb, pp, g, ph = st_mom(t)
        return pr.bin_mom(pr.sk(z_dn, pb, pp, g, ph)[0])

    tgrid = [P.psd_mom_min * 10.0 ** (k / (2.0 * bpd)) for k in range(-6, 2 * (nm + 6))]
    seen = set()
    for lo, hi, blo, bhi in changes(f_mom, tgrid):
        key = (min(blo, bhi), max(blo, bhi))
        if key in seen:
            continue
        seen.add(key)
        ids = []
        for t in ladder(lo, hi):
            pb, pp, g, ph = st_mom(t)
            ids += variants(f"momentum edge {key}", z_dn, pb, pp, t, g, ph, 1.0 + 0.25 * (len(ids) % 3))
        info["ladders"].append(("momentum", key, ids))
    # beyond the last bin: the clamp and its counter
    for t in (P.psd_mom_min * 10.0 ** ((nm + 3) / bpd), P.psd_mom_min * 10.0 ** ((nm + 30) / bpd)):
        pb, pp, g, ph = st_mom(t)
        info["branches"].setdefault("momentum clamp", []).extend(variants("momentum clamp", z_dn, pb, pp, t, g, ph, 1.0))

    # -- branch edges
    def f_spike(al):
        pb, pp, g, ph = st_angle(al)
        s = pr.sk(z_up, pb, pp, g, ph)
        return int(s[0] > abs(s[1] * SPIKE_AWAY))

    ids = []
    a0 = changes(lambda al: int(pr.sk(z_up, *st_angle(al))[1] > 0), [float(t) for t in np.linspace(0.0, math.pi, 41)])[0][0]      # p_x changes sign
    for lo, hi, blo, bhi in changes(f_spike, [a0 - 0.1, a0, a0 + 0.1]):
        for al in ladder(lo, hi):
            pb, pp, g, ph = st_angle(al)
            ids += variants("spike-away switch", z_up, pb, pp, p_a, g, ph, 1.0)
    info["branches"]["spike"] = ids

    def f_rel(t):
        pb, pp, g, ph = st_mom(t)
        gs = pr.sk(z_dn, pb, pp, g, ph)[4]
        return int((gs - 1) > E_REL_PT) + int((gs - 1) >= E_REL_PT)

    ids = []
    for lo, hi, blo, bhi in changes(f_rel, [0.01 * mc, 1.0 * mc]):
        for t in ladder(lo, hi):
            pb, pp, g, ph = st_mom(t)
            ids += variants("E_rel_pt switch", z_dn, pb, pp, t, g, ph, 1.0)
    info["branches"]["e_rel"] = ids
    # p_tot_sk == 0 (nothing moves in the shock frame: gam_pf = 0 is no physical state, and a legal input)
    info["branches"]["ptot_sk == 0"] = variants("ptot_sk == 0", z_up, 0.0, 0.0, 1.0 * mc, 0.0, 0.0, 1.0)
    # p_cos = +1 and -1 exactly, and with them the edge of the plasma-frame clamp (p_y = p_z = 0: pt_Xf == |px_Xf|): parallel field only
    if float(prob.theta[z_up]) == 0.0:
        info["branches"]["p_cos == +-1"] = (variants("p_cos == +1", z_up, -p_a, 0.0, p_a, g_a, 0.3, 1.0) +
                                           variants("p_cos == -1", z_up, p_a, 0.0, p_a, g_a, 0.3, 1.0))

    # -- crossings: both directions, 1, 2 and many zones, the ends of the grid, the upstream FEB zone and the FEB itself
    feb = P.i_grid_feb
    pairs = [(k, k + 1) for k in (1, feb, P.i_shock, ng - 1)] + [(k, k + 2) for k in (0, feb - 1, P.i_shock - 1, ng - 2)] + \
            [(3, 60), (0, 3), (ng - 3, ng), (0, ng), (feb - 2, feb + 3)]
    pairs += [(b, a) for a, b in pairs]
    ids = []
    for n_, (i_old, i_new) in enumerate(pairs):
        for inj in (1, 0):
            down = i_new > i_old
            v = mc * 10.0 ** rng.uniform(-2.0, 3.0)
            mu = rng.uniform(0.05, 0.95) * (1 if down else -1)
            x_old, x = 0.5 * (float(xg[i_old]) + float(xg[i_old + 1])), 0.5 * (float(xg[i_new]) + float(xg[i_new + 1]))
            assert (x > x_old) == down
            ids.append(R.add(f"crossing {i_old}->{i_new}", KIND_CROSS, mu * v, math.sqrt(1 - mu * mu) * v, v, math.hypot(v / mc, 1),
                             rng.uniform(0, 2 * math.pi), rng.uniform(0.5, 1.5), x, x_old, i_new, i_old, i_new, inj))
    info["branches"]["crossings"] = ids
    ids = []
    for x_old, x in ((P.feb_upstream, math.nextafter(P.feb_upstream, -math.inf)), (P.feb_upstream * 0.5, P.feb_upstream * 2.0),
                     (math.nextafter(P.feb_upstream, -math.inf), P.feb_upstream * 2.0), (P.feb_upstream, P.feb_upstream * 0.5)):
        for inj in (1, 0):
            v = 50.0 * mc
            ids.append(R.add(f"upstream FEB x_old={x_old:.17g} x={x:.17g}", KIND_CROSS, -0.8 * v, 0.6 * v, v, math.hypot(v / mc, 1), 1.1, 0.75,
                             x, x_old, feb - 1, feb + 1, feb + 1, inj))
    info["branches"]["feb"] = ids

    # -- finished particles: every reason in every zone class
    ids = []
    for z in zone_classes(P):
        for reason in (1, 2, 3, 4):
            v = mc * 10.0 ** rng.uniform(-2.0, 3.0)
            mu = rng.uniform(-0.95, 0.95)
            ids.append(R.add(f"finish reason {reason} zone {z}", KIND_FINISH, mu * v, math.sqrt(1 - mu * mu) * v, v, math.hypot(v / mc, 1),
                             rng.uniform(0, 2 * math.pi), rng.uniform(0.5, 1.5), ig3=z, aux=reason))
    info["branches"]["finish"] = ids
    pr.ob.destroy()
    return R, info


# ---- launches ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Launch:
    name: str
    rec: np.ndarray          # [n_pass][n_thread][8]
    word: np.ndarray         # [n_pass][n_thread]
    ids: np.ndarray          # [n_pass][n_thread]: index into the pool's records (-1 idle), for messages
    exempt: bool = False     # a crafted stack shape: same-bin deposits on purpose
    log: tuple = None        # (record index IN THE LAUNCH, buffer, offset, value) from the oracle


def layout(name, rows, words, ids, n_thread, exempt=False):
    n = len(words)
    n_pass = max((n + n_thread - 1) // n_thread, 1)
    rec = np.zeros((n_pass * n_thread, 8))
    word = np.zeros(n_pass * n_thread, dtype=np.uint64)
    idx = np.full(n_pass * n_thread, -1, dtype=np.int64)
    rec[:n], word[:n], idx[:n] = rows, words, ids
    return Launch(name, rec.reshape(n_pass, n_thread, 8), word.reshape(n_pass, n_thread), idx.reshape(n_pass, n_thread), exempt)


def hist_ranges(L):
    return [(L.offsets[n], L.offsets[n] + int(np.prod(L.shapes[n]))) for n in HIST]


def is_hist(L, off):
    off = np.asarray(off)
    m = np.zeros(off.shape, dtype=bool)
    for lo, hi in hist_ranges(L):
        m |= (off >= lo) & (off < hi)
    return m


def split(case, R, ob, n_thread=448, max_launches=24):
    """The pool dealt into launches in which no histogram cell receives two deposits (first fit on the oracle's log of the whole pool)."""
    rows, words = R.arrays()
    L = ob.layout
    case.begin(ob)
    lr, lb, lo, lv = ob.eval_tally(rows, words)
    hist = (lb == 0) & is_hist(L, lo)
    cells = [[] for _ in range(len(R))]
    for r, o in zip(lr[hist], lo[hist]):
        cells[r].append(int(o))
    used, members = [], []
    for r in range(len(R)):
        cs = set(cells[r])
        for k in range(len(used)):
            if not (cs & used[k]):
                break
        else:
            used.append(set()); members.append([])
            k = len(used) - 1
        used[k] |= cs
        members[k].append(r)
    assert len(members) <= max_launches, f"{case.name}: the pool needs {len(members)} launches"
    return [layout(f"pool {k}", rows[mm], words[mm], np.array(mm), n_thread) for k, mm in enumerate(members)]


def stack_shapes(case):
    """Launches crafted for the record stack: sizes round 64 and 256, one-bin batches with and without an odd lane, crossings mixed in,
    equal bins of reasons 1 and 2, a partial last batch, two pushes per lane before a drain, ragged idle lanes."""
    P, prob, aa = case.prob.params, case.prob, case.aa
    mc = aa * MP * CC
    ng = P.n_grid
    z = min(P.i_shock + 3, ng)
    rng = np.random.default_rng(77)
    x_old, x = 5.0 * prob.rg0, 6.0 * prob.rg0

    def fin(v, mu, reason, w, zone=z):
        return ((mu * v, math.sqrt(1 - mu * mu) * v, v, math.hypot(v / mc, 1), 0.4, w, 0.0, 0.0), pack(0, 0, zone, 0, reason, KIND_FINISH))

    def cross(v, mu, i, inj, w):
        return ((mu * v, math.sqrt(1 - mu * mu) * v, v, math.hypot(v / mc, 1), 0.4, w, x, x_old), pack(i, i - 1, z, inj, 0, KIND_CROSS))

    idle = ((0.0,) * 8, pack(0, 0, 0, 0, 0, KIND_IDLE))
    out = []

    def emit(name, items, n_thread, exempt=True):
        rows = np.array([it[0] for it in items]).reshape(-1, 8)
        words = np.array([it[1] for it in items], dtype=np.uint64)
        out.append(layout(name, rows, words, np.arange(len(items)), n_thread, exempt))

    # sizes: distinct random finished particles and crossings, one pass and three
    for n in (1, 63, 64, 65, 255, 257, 3001):
        items = []
        for j in range(n):
            v, mu = mc * 10.0 ** rng.uniform(-1, 5), rng.uniform(-0.9, 0.9)
            items.append(cross(v, abs(mu), 1 + j % ng, j % 2, 1.0 + j % 5) if j % 5 else fin(v, mu, 1 + (j // 5) % 2, 1.0 + j % 5))
        emit(f"n={n} one pass", items, n, exempt=False)
        if n >= 63:
            emit(f"n={n} three passes", items, (n + 2) // 3, exempt=False)
    same = lambda j, reason=1: fin(20.0 * mc, 0.5, reason, 1.0 + 0.125 * (j % 9))
    other = lambda reason=1: fin(3.0e2 * mc, -0.5, reason, 1.5)
    emit("64 in one bin", [same(j) for j in range(64)], 64)
    for odd in (0, 31, 63):
        emit(f"63 in one bin, lane {odd} in another", [other() if j == odd else same(j) for j in range(64)], 64)
        emit(f"63 in one bin, lane {odd} in another, crossings mixed in",
             [other() if j == odd else (cross(7.0 * mc, 0.3, 1 + j, 1, 1.0) if j % 4 == 1 else same(j)) for j in range(64)], 64)
    emit("reasons 1 and 2 with equal bins", [same(j, 1 + j % 2) for j in range(64)], 64)
    emit("a partial last batch: 64 + 23 in one bin", [same(j) for j in range(87)], 64)
    emit("two pushes per lane before a drain", [same(j) for j in range(40)] + [idle] * 24 + [same(j) for j in range(64)] + [same(j, 2) for j in range(64)], 64)
    ragged = []
    for j in range(4 * 300):
        v, mu = mc * 10.0 ** rng.uniform(-1, 5), rng.uniform(0.1, 0.9)
        ragged.append(idle if (j * 7 + j // 300) % 5 >= 3 else (same(j) if j % 4 == 0 else cross(v, mu, 1 + j % ng, j % 2, 1.0)))
    emit("ragged idle lanes, 300 threads x 4 passes", ragged, 300)
    return out


def attach_logs(case, launches, ob, f32=False):
    """The oracle's log of every launch (record indices within the launch)."""
    case.begin(ob)
    for la in launches:
        la.log = ob.eval_tally(la.rec, la.word, f32_units=f32)
    return launches


# ---- the expected buffers ---------------------------------------------------------------------------------------------------------
def expected(L, T0, I0, log):
    """-> (offs, serial, k, K, S, ioffs, iexp): for the fp64 cells the log names, the reference on top of T0 (one term: fl(T0 + term), which
    is the serial sum; more: the correctly rounded exact sum), the number of terms, of non-zero summands, and the sum of magnitudes; for
    the int64 cells, the exact result."""
    lr, lb, lo, lv = log
    f = lb == 0
    offs, inv = np.unique(lo[f], return_inverse=True)
    vals = lv[f]
    serial = T0[offs].copy()
    np.add.at(serial, inv, vals)                    # unbuffered: the adds of a cell happen in log order
    k = np.bincount(inv, minlength=len(offs))
    # a cell with several summands: their EXACT sum, correctly rounded (math.fsum).  The bound above is a theorem about a floating-point
    # sum against the exact one; against another floating-point sum (the serial one, which errs by as much) only twice the bound holds.
    multi = np.flatnonzero(k > 1)
    if len(multi):
        order = np.argsort(inv, kind="stable")
        start = np.searchsorted(inv[order], np.arange(len(offs) + 1))
        for c in multi:
            serial[c] = math.fsum([float(T0[offs[c]])] + vals[order[start[c]:start[c + 1]]].tolist())
    S = np.abs(T0[offs])
    np.add.at(S, inv, np.abs(vals))
    K = np.bincount(inv, weights=(vals != 0).astype(np.float64), minlength=len(offs)) + (T0[offs] != 0)
    ioffs, iinv = np.unique(lo[~f], return_inverse=True)
    iexp = I0[ioffs].copy()
    np.add.at(iexp, iinv, lv[~f].astype(np.int64))
    return offs, serial, k, K, S, ioffs, iexp


def bound(K, S):
    Km = np.maximum(K - 1, 0)
    with np.errstate(invalid="ignore"):          # (a cell that holds inf has no bound: it is compared bit for bit)
        return Km * U * S / (1 - Km * U)


def feeders(launch, off, buf=0, limit=6):
    lr, lb, lo, lv = launch.log
    sel = np.flatnonzero((lb == buf) & (lo == off))
    rec, word = launch.rec.reshape(-1, 8), launch.word.reshape(-1)
    lines = [f"    record {int(lr[i])} (pass {int(lr[i]) // launch.word.shape[1]}, thread {int(lr[i]) % launch.word.shape[1]}) "
             f"term {float(lv[i]).hex()} {describe(rec[lr[i]], word[lr[i]])}" for i in sel[:limit]]
    if len(sel) > limit:
        lines.append(f"    ... and {len(sel) - limit} more records")
    return "\n".join(lines)


def cell_name(L, off):
    for name, o in L.offsets.items():
        n = int(np.prod(L.shapes[name]))
        if o <= off < o + n:
            return f"{name}{list(int(v) for v in np.unravel_index(off - o, L.shapes[name]))}"
    return f"T[{off}]"


def check_launch(L, launch, T0, I0, T1, I1, what):
    """The per-cell rule over the whole of T and I.  -> (bit-exact histogram deposits, histogram deposits in the bound class)."""
    offs, serial, k, K, S, ioffs, iexp = expected(L, T0, I0, launch.log)
    changed = np.flatnonzero(T1.view(np.uint64) != T0.view(np.uint64))
    stray = np.setdiff1d(changed, offs)
    if len(stray):
        # a deposit in a cell of nobody's: name the records whose own cell did not change, the likely senders
        lost = [int(o) for o, kk, s_ in zip(offs, k, S) if kk >= 1 and s_ > abs(T0[o]) and T1[o:o + 1].view(np.uint64)[0] == T0[o:o + 1].view(np.uint64)[0]]
        senders = "".join(f"\n  {cell_name(L, o)} did not change; fed by\n{feeders(launch, o, limit=2)}" for o in lost[:3])
        raise AssertionError(f"{what}: {len(stray)} cells changed that no record feeds, first {cell_name(L, int(stray[0]))}: "
                             f"{float(T0[stray[0]]).hex()} -> {float(T1[stray[0]]).hex()}; {len(lost)} fed cells did not change{senders}")
    dev = T1[offs]
    exact = k <= 1
    bad = np.flatnonzero(exact & (dev.view(np.uint64) != serial.view(np.uint64)))
    fin = np.isfinite(serial)
    b = bound(K, S)
    with np.errstate(invalid="ignore"):
        over = ~exact & np.where(fin, ~(np.abs(dev - serial) <= b), dev.view(np.uint64) != serial.view(np.uint64))
    bad = np.concatenate([bad, np.flatnonzero(over)])
    if len(bad):
        i = int(bad[0])
        o = int(offs[i])
        raise AssertionError(f"{what}: {len(bad)} cells off, first {cell_name(L, o)} (T[{o}]): device {float(dev[i]).hex()} reference "
                             f"{float(serial[i]).hex()} before {float(T0[o]).hex()}, {int(k[i])} terms, bound "
                             f"{'bit-exact' if exact[i] else float(b[i]).hex()}; fed by\n{feeders(launch, o)}")
    ichanged = np.flatnonzero(I1 != I0)
    istray = np.setdiff1d(ichanged, ioffs)
    assert len(istray) == 0, f"{what}: int64 tally {int(istray[0])} changed ({int(I0[istray[0]])} -> {int(I1[istray[0]])}) and no record feeds it"
    ibad = np.flatnonzero(I1[ioffs] != iexp)
    if len(ibad):
        o = int(ioffs[ibad[0]])
        raise AssertionError(f"{what}: int64 tally {o}: device {int(I1[o])} reference {int(iexp[ibad[0]])}; fed by\n{feeders(launch, o, buf=1)}")
    h = is_hist(L, offs)
    return int(k[h & exact].sum()), int(k[h & ~exact].sum())


def to_f32_units(case, launch):
    """A launch of form 2: the same records with every value rounded to a float in the fp32 kernels' units (momenta in m_p c, lengths in
    rg0 = gam0 beta0 m_p c^2 / (e B[0])), idle slots untouched.  The reference sees (double) f * unit."""
    P = case.prob.params
    L0 = P.gam0 * P.beta0 * MP * CC * CC / (QCGS * float(case.prob.btot[0]))
    P0 = MP * CC
    rec = launch.rec.copy()
    rec[..., 0:3] /= P0
    rec[..., 6:8] /= L0
    rec = rec.astype(np.float32)
    # a move keeps its direction, and a value that overflows or vanishes in fp32 is pulled inside
    fmax = np.finfo(np.float32).max
    rec = np.clip(rec, -fmax, fmax)
    same = (rec[..., 6] == rec[..., 7]) & (launch.rec[..., 6] != launch.rec[..., 7])
    up = launch.rec[..., 6] > launch.rec[..., 7]
    rec[..., 6] = np.where(same, np.nextafter(rec[..., 7], np.where(up, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)), rec[..., 6])
    return Launch(launch.name + " (fp32 units)", rec.astype(np.float64), launch.word.copy(), launch.ids, True)
