"""The shock-profile update (include/mcs.h, mcs_profile_update) restated in plain Python floats from the header's text -- powers are
products, every operation one IEEE rounding, division by zero and the root of a negative number as IEEE gives them -- and the crafted
inputs of tests/test_profile_update_host.py and tests/test_gpu_profile_update.py.  Nothing here imports the package's consumers or
iter_finalize arithmetic or shares code with csrc/mcs_consumers.hip; iter_finalize.upstream_fluxes only supplies two INPUT numbers.

  scalars   px_esc = sc[2] / F_px; en_esc = sc[3] / F_en; gamma_down = 1 + sc[0] / sc[1]; q by q_esc_calcs; q_avg = (((h0 + h1) + h2) + q) / k
  per zone  pxx = rint(flux 1e13) / 1e13; G = 1 + (P_par + P_perp) / e (1e-99 where e == 1e-99); Xi = G / (G - 1); p_px; p_loc; two roots
  ordered   last-ten sum / 10; smooth_profile!; rescale; pin (x >= 0 -> u2); relativistic: smooth then rescale, classical: the reverse
  per zone  ux_pred = (1 - SMMOE) ux_px + SMMOE ux_en; the arctangent section; ux_next = (v + w u) / (1 + w); shift = (ux_pred - u) / u0"""
import copy
import math

import numpy as np

from conftest import mcs, make_problem

C = mcs.constants.C
MP = mcs.constants.MP
KB = mcs.constants.KB
NAN, INF = float("nan"), float("inf")
ROWS = ("flux_px", "flux_en", "gamma_ad", "p_flux", "p_used", "ux_px", "ux_en", "ux_pred", "ux_next", "shift")
SCALARS = ("gamma_down", "px_esc_up", "en_esc_up", "q_px", "q_en", "q_px_avg", "q_en_avg", "shift_rms")
NEWTON_MAX = 10_000


def div(a, b):
    """a / b as IEEE 754 gives it (Python raises on a zero divisor)."""
    if b == 0:
        if a != a or a == 0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def sqrt(a):
    if a != a or a < 0:
        return NAN
    return math.sqrt(a)


def rint13(x):
    y = x * 1.0e13
    if y != y or y in (INF, -INF):
        return div(y, 1.0e13)
    r = float(round(y)) if abs(y) < 2.0 ** 52 else y       # Python's round(float) rounds half to even, as rint does
    if r == 0:
        r = math.copysign(0.0, y)
    return r / 1.0e13


def q_esc(G, c):
    """-> (q_px, q_en): q_esc_calcs's two returns in the order the reference binds them."""
    if c["r_comp"] == c["r_RH"]:
        return 0.0, 0.0
    u0, b0, g0, u2, b2, g2, rho0, P0 = c["u0"], c["beta0"], c["gam0"], c["u2"], c["beta2"], c["gam2"], c["rho0"], c["P0"]
    Gf = div(G, G - 1.0)
    rho2 = div((rho0 * g0) * b0, g2 * b2)
    if b0 >= 0.02:
        q_fac = C * sqrt(div(1.0 + b0, 2.0))
        e = rho0 * (C * C) + 2.5 * P0
        Fp = ((g0 * g0) * (b0 * b0)) * e + P0
        Fe = ((g0 * g0) * u0) * e
        aux = (g2 * g2) * (q_fac * (b2 * b2) - u2)
        P2 = div((q_fac * Fp - Fe) - (aux * rho2) * (C * C), q_fac + Gf * aux)
        t = g2 * b2
        Qp = (Fp - (t * t) * (rho2 * (C * C) + Gf * P2)) - P2
        Qe = Qp * q_fac
        return div(Qe, Fe - ((g0 * u0) * rho0) * (C * C)), div(Qp, Fp)
    Fp = rho0 * (u0 * u0) + P0
    Fe = div(rho0 * ((u0 * u0) * u0), 2.0) + (2.5 * P0) * u0
    P2 = Fp - rho2 * (u2 * u2)
    Qe = (Fe - div((rho0 * u0) * (u2 * u2), 2.0)) - (P2 * u2) * Gf
    return div(Qe, Fe), 0.0


def newton(f_df, x):
    """-> (x, steps, ran_out)"""
    for k in range(NEWTON_MAX):
        f, df = f_df(x)
        dx = div(f, df)
        x = x - dx
        if abs(dx) <= 1.0e-14 * abs(x):
            return x, k + 1, False
    return x, NEWTON_MAX, True


def smooth(a):
    n = len(a)
    for i in range(n - 1, 0, -1):
        if a[i - 1] < a[i]:
            a[i - 1] = a[i]
    d = list(a)
    d[1] = ((2.0 * a[0] + a[1]) + a[2]) / 4.0
    for i in range(2, n - 2):
        d[i] = ((a[i - 1] + a[i]) + a[i + 1]) / 3.0
    d[n - 2] = ((a[n - 3] + a[n - 2]) + 2.0 * a[n - 1]) / 4.0
    for i in range(1, n - 1):
        a[i] = d[i]


def rescale(a, avg, u0, u2, x_cm):
    s = div(u0 - u2, a[0] - avg)
    for j in range(len(a)):
        v = s * (a[j] - avg) + u2
        a[j] = u2 if x_cm[j + 1] >= 0.0 else v


class Reference:
    def __init__(self, rows, scalars, diag):
        self.rows = np.array(rows, dtype=np.float64)
        self.scalars = np.array(scalars, dtype=np.float64)
        self.diag = np.array(diag, dtype=np.int64)

    def words(self):
        return np.concatenate([self.rows.ravel(), self.scalars])

    def row(self, name):
        return self.rows[ROWS.index(name)]


def restate(c) -> Reference:
    """c: a case dict (make_cases)."""
    n, i_shock = c["n_grid"], c["i_shock"]
    u0, b0, g0, u2 = c["u0"], c["beta0"], c["gam0"], c["u2"]
    F_px, F_en, n0 = c["F_px_upstream"], c["F_energy_upstream"], c["n0_aa"]
    rel = b0 >= 0.02
    sc = [float(v) for v in c["scalars"]]
    px_esc, en_esc = div(sc[2], F_px), div(sc[3], F_en)
    G_down = 1.0 + div(sc[0], sc[1])
    q_px, q_en = q_esc(G_down, c)
    hp, he = list(c["hist_q_px"]) + [q_px], list(c["hist_q_en"]) + [q_en]
    s_px, s_en = hp[0], he[0]
    for k in range(1, len(hp)):
        s_px = s_px + hp[k]; s_en = s_en + he[k]
    q_px_avg, q_en_avg = s_px / float(len(hp)), s_en / float(len(hp))
    pxx = [rint13(float(v)) for v in c["pxx_flux"]]
    en = [rint13(float(v)) for v in c["energy_flux"]]
    Qpx = q_px_avg * pxx[0] if rel else 0.0
    Qen = q_en_avg * en[0]
    wp, mo, w = c["SMPFP"], c["SMMOE"], c["w"]
    rows = {k: [0.0] * n for k in ROWS}
    a_px, a_en = [0.0] * n, [0.0] * n
    steps_max, n_out = 0, 0
    for j in range(n):
        Ptot = float(c["P_par"][j]) + float(c["P_perp"][j])
        ed = float(c["e_dens"][j])
        G = 1.0 + div(Ptot, ed)
        if ed == 1.0e-99:
            G = 1.0e-99
        Xi = div(G, G - 1.0)
        u, g = float(c["ux"][j + 1]), float(c["gam_sf"][j + 1])
        b = u / C
        pxx_EM, en_EM = float(c["pxx_EM"][j]), float(c["en_EM"][j])
        if rel:
            gb = g * b
            gb2 = gb * gb
            dens = div(g0 * b0, g * b) * n0
            p_px = div(pxx[j] - ((gb2 * dens) * MP) * (C * C), 1.0 + gb2 * Xi)
            p_loc = (1.0 - wp) * p_px + wp * Ptot
            y = div(((F_px - Qpx) - pxx_EM) - p_loc, ((g0 * b0) * n0) * (MP * (C * C) + div(p_loc * Xi, dens)))
            a_px[j] = div(y, sqrt(1.0 + y * y)) * C
            K = div((F_en - Qen) - en_EM, C * ((dens * MP) * (C * C) + Xi * p_loc))
            z = (-1.0 + sqrt(1.0 + (4.0 * K) * K)) / 2.0
            y = math.copysign(sqrt(z), K)
            a_en[j] = div(y, sqrt(1.0 + y * y)) * C
        else:
            rm = n0 * MP
            bb = b * b
            p_px = div(pxx[j] - ((rm * u0) * u) * (1.0 + bb), 1.0 + bb * Xi)
            p_loc = (1.0 - wp) * p_px + wp * Ptot
            A = (F_px - Qpx) - pxx_EM
            B = (F_en - Qen) - en_EM

            def f_px(x):
                xx = x * x
                return ((A - ((rm * u0) * (x * C)) * (1.0 + xx)) - (1.0 + xx * Xi) * p_loc,
                        -(((rm * u0) * C) * (1.0 + (3.0 * x) * x) + ((2.0 * x) * Xi) * p_loc))

            def f_en(x):
                t = x / C
                t2 = t * t
                return ((B - ((((0.5 * rm) * u0) * x) * x) * (1.0 + 1.25 * t2)) - ((Xi * p_loc) * x) * (1.0 + t2),
                        -(((rm * u0) * x) * (1.0 + 2.5 * t2) + (Xi * p_loc) * (1.0 + 3.0 * t2)))
            x, k1, o1 = newton(f_px, (u0 / C) * 1.0e-4)
            a_px[j] = x * C
            a_en[j], k2, o2 = newton(f_en, u0 * 1.0e-4)
            steps_max = max(steps_max, k1, k2)
            n_out += 1 if (o1 or o2) else 0
        rows["flux_px"][j] = div(pxx[j], F_px)
        rows["flux_en"][j] = div(en[j], F_en)
        rows["gamma_ad"][j] = G
        rows["p_flux"][j] = p_px
        rows["p_used"][j] = p_loc
    x_cm = [float(v) for v in c["x_grid_cm"]]
    for a in (a_px, a_en):
        avg = 0.0
        for j in range(max(0, n - 10), n):
            avg = avg + a[j]
        avg = avg / 10.0
        if rel:
            smooth(a); rescale(a, avg, u0, u2, x_cm)
        else:
            rescale(a, avg, u0, u2, x_cm); smooth(a)
    pred = [(1.0 - mo) * a_px[j] + mo * a_en[j] for j in range(n)]
    v = list(pred)
    it = c["i_trans"]
    if it > 0:
        last = pred[n - 1]
        s = div(-(pred[it - 1] - last), float(c["atan_x"][it - 1]))
        for j in range(it - 1, i_shock):
            v[j] = (-float(c["atan_x"][j])) * s + last
    S = 0.0
    for j in range(n):
        u = float(c["ux"][j + 1])
        rows["ux_px"][j], rows["ux_en"][j], rows["ux_pred"][j] = a_px[j], a_en[j], pred[j]
        rows["ux_next"][j] = div(v[j] + w * u, 1.0 + w)
        sh = div(pred[j] - u, u0)
        rows["shift"][j] = sh
        S = S + sh * sh
    px_esc = 1.0e-99 if 1.0e-99 > px_esc else px_esc
    en_esc = 1.0e-99 if 1.0e-99 > en_esc else en_esc
    scal = [G_down, px_esc, en_esc, q_px, q_en, q_px_avg, q_en_avg, sqrt(S / float(n))]
    allw = [x for k in ROWS for x in rows[k]] + scal
    bad = sum(1 for x in allw if x != x or x in (INF, -INF))
    return Reference([rows[k] for k in ROWS], scal, [bad, n_out, steps_max])


# ---- the crafted inputs ----------------------------------------------------------------------------------------------------------
def classical_problem(N=64):
    """A problem whose shock speed is 1500 km/s with r = 4, put into the params by hand as tests/test_iter_finalize.py does
    (build_problem cannot make one): to be done BEFORE a backend is created from it."""
    return to_classical(make_problem(N))


def to_classical(prob):
    P = prob.params
    u0 = 1.5e8
    P.u0, P.beta0, P.gam0 = u0, u0 / C, 1 / math.sqrt(1 - (u0 / C) ** 2)
    P.u2 = u0 / 4; prob.beta2 = P.u2 / C; prob.gam2 = 1 / math.sqrt(1 - prob.beta2 ** 2)
    up = prob.x_grid_cm < 0
    prob.ux = np.where(up, u0, P.u2); prob.utot = prob.ux.copy()
    prob.gam_sf = 1 / np.sqrt(1 - (prob.ux / C) ** 2)
    return prob


def base_case(prob):
    """A mildly modified flow on prob's grid: every field of a case."""
    P, cfg = prob.params, prob.cfg
    n = P.n_grid
    F_px, _, F_en = mcs.iter_finalize.upstream_fluxes(prob)
    n0 = np.array([s.density for s in cfg.species]); T0 = np.array([s.temperature for s in cfg.species])
    m = np.array([s.mass for s in cfg.species])
    x = np.asarray(prob.x_grid_rg, dtype=np.float64)[1:n + 1]
    ramp = np.exp(-np.abs(np.clip(x, -1e6, 1e6)) / 30.0)
    ux = np.asarray(prob.ux, dtype=np.float64)
    rel = P.beta0 >= 0.02
    if rel:
        pxx = F_px * (1 - 0.03 * ramp)
        en = F_en * (1 - 0.02 * ramp)
    else:
        pxx = MP * P.u0 * ux[1:n + 1] * (1 + 0.2 * ramp)
        en = 0.5 * MP * P.u0 ** 3 * np.ones(n)
    Pp = 0.004 * F_px * (0.2 + ramp)
    return dict(n_grid=int(n), i_shock=int(P.i_shock), u0=float(P.u0), beta0=float(P.beta0), gam0=float(P.gam0),
                F_px_upstream=float(F_px), F_energy_upstream=float(F_en), P0=float(np.dot(n0, T0)) * KB, rho0=float(np.dot(n0, m)),
                n0_aa=float(sum(s.density * s.aa for s in cfg.species)), r_comp=float(prob.r_comp), r_RH=float(prob.r_comp) * 1.03,
                u2=float(P.u2), beta2=float(prob.beta2), gam2=float(prob.gam2), SMMOE=0.4, SMPFP=0.3, w=1.0, i_trans=0,
                hist_q_px=(), hist_q_en=(), pxx_EM=1.0e-3 * F_px * (1 + ramp), en_EM=2.0e-3 * F_en * (1 + 0.5 * ramp), atan_x=np.arctan(x),
                ux=ux.copy(), gam_sf=np.asarray(prob.gam_sf, dtype=np.float64).copy(), x_grid_cm=np.asarray(prob.x_grid_cm, dtype=np.float64).copy(),
                pxx_flux=pxx, energy_flux=en, scalars=np.array([1.0, 2.5, 0.01 * F_px, 0.02 * F_en]),
                P_par=Pp, P_perp=0.8 * Pp, e_dens=3.1 * 1.8 * Pp)


def make_cases(prob):
    """[(name, case)] for prob's branch (relativistic for a built problem, classical for classical_problem())."""
    b = base_case(prob)
    n, F_px, F_en, i_shock = b["n_grid"], b["F_px_upstream"], b["F_energy_upstream"], b["i_shock"]
    rel = b["beta0"] >= 0.02
    tag = "rel" if rel else "cls"
    out = []

    def case(name, **kw):
        c = copy.deepcopy(b)
        for k, v in kw.items():
            if callable(v):
                v(c[k])
            else:
                c[k] = v
        out.append((f"{tag}_{name}", c))
        return c

    def fill(v):
        return lambda a: a.__setitem__(slice(None), v)

    def ties(a):       # fluxes at (k +- 1/2) 1e-13 (rint's ties to even), negative, 0 and 1e-99
        a[3], a[4], a[5], a[6], a[7], a[8], a[9] = 2.5e-13, 3.5e-13, -2.5e-13, 0.0, 1.0e-99, -4.5e-13, 0.5e-13
        a[0] = a[0] + 0.5e-13

    def edens(a):
        a[2], a[3] = 1.0e-99, 0.0

    def last_ten(a):   # values whose sum depends on the order
        a[n - 10:] = F_px * np.array([0.9, -0.5, 0.3, 0.99, 1.0e-9, -3.0, 0.7, 0.2, 1.0e-5, 0.05])

    def last_ten_en(a):
        a[n - 10:] = F_en * np.array([0.5, 1.0e-7, -2.0, 0.3, 0.9, 0.1, 1.0e-3, 0.77, -0.4, 0.6])

    def k_sign(a):
        a[5], a[6], a[7] = 2.0 * F_en, F_en, 1.5 * F_en

    case("base")
    case("ties", pxx_flux=ties, energy_flux=ties, SMMOE=0.0, w=0.0, hist_q_px=(0.011,), hist_q_en=(0.02,))
    case("edens", e_dens=edens, SMPFP=0.0, SMMOE=1.0, i_trans=2, w=10.35)
    case("equal_neighbours", pxx_flux=fill(b["pxx_flux"][0]), P_par=fill(b["P_par"][0]), P_perp=fill(b["P_perp"][0]),
         e_dens=fill(b["e_dens"][0]), pxx_EM=fill(b["pxx_EM"][0]), hist_q_px=(0.01, 0.012), hist_q_en=(0.02, 0.021))
    case("increasing", pxx_EM=fill(F_px * np.linspace(0.6, 0.05, n)), en_EM=fill(F_en * np.linspace(0.7, 0.1, n)), i_trans=i_shock)
    case("monotone", pxx_EM=fill(F_px * np.linspace(0.05, 0.6, n)), en_EM=fill(F_en * np.linspace(0.1, 0.7, n)), SMPFP=1.0,
         hist_q_px=(0.01, 0.012, -0.003), hist_q_en=(0.02, 0.021, 0.0))
    case("last_ten", pxx_EM=last_ten, en_EM=last_ten_en)
    if rel:
        # every zone the same root 0: arr[0] == avg, a division by zero in the rescale.  (Relativistic only: the classical iteration
        # towards a root 0 never meets |dx| <= tol |x| and every zone would run its 10000 steps.)
        case("first_equals_avg", r_RH=b["r_comp"], SMPFP=1.0, SMMOE=0.0, P_par=fill(0.0), P_perp=fill(0.0), pxx_EM=fill(F_px), e_dens=fill(1.0))
    # K < 0 and K == 0 in the energy equation (no escape, so that Qen is 0 and F_en - en_EM can vanish exactly)
    case("K_sign", r_RH=b["r_comp"], en_EM=k_sign, SMMOE=1.0)
    if not rel:
        # one zone whose momentum iteration never converges (a NaN never passes the test): 10000 plain steps
        case("newton_runs_out", pxx_EM=lambda a: a.__setitem__(7, NAN), i_trans=2, w=10.35, hist_q_px=(0.3, 0.2, 0.1), hist_q_en=(0.0, 0.0, 0.0))
    return out


TALLY_PARTS = ("pxx_flux", "energy_flux", "scalars")


def crafted_tallies(layout, c):
    """A tally buffer that holds the case's fluxes and scalars and a NaN in every word the call must not read."""
    f = np.full(layout.total, np.nan)
    for k in TALLY_PARTS:
        layout.view(f, k)[...] = np.asarray(c[k], dtype=np.float64).reshape(layout.view(f, k).shape)
    return f


def same_words(a, b):
    """Bit-equal, a NaN matching any NaN."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def first_difference(a, b, n):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    for k in range(min(a.size, b.size)):
        if not same_words(a[k:k + 1], b[k:k + 1]):
            name = ROWS[k // n] if k < len(ROWS) * n else "scalars"
            return f"word {k} ({name}[{k % n if k < len(ROWS) * n else k - len(ROWS) * n}]): {a[k]!r} != {b[k]!r}"
    return "lengths differ" if a.size != b.size else "none"
