"""Helpers of the cell-by-cell consumer tests (test_consumers_cells.py, test_gpu_consumers_cells.py and the per-cell criteria of
test_consumers.py / test_photon_ic.py): crafted tallies, and restatements of the three tally consumers that share no code with
oracle/mcs_consumers.cpp or csrc/mcs_consumers.hip.

One PSD cell in one frame (get_dNdp_cr: src/particle_counter.jl:29-306): `cell_parts` is written from the reference's text of
transform_psd_corners (src/transformers.jl:634-682), identify_corners (src/identify_corners.jl:30-245), get_transform_dN and
triangular_distribution! (src/transformers.jl:29-312), with the consumer quirks C1-C6 of DESIGN.md section 3b.  It is generic in its
arithmetic: `F64` runs it in Python floats -- IEEE doubles, one rounding per operation, no fma, the library's own log10
(include/mcs_math.h) -- which is the kernel's arithmetic operation by operation; `MP` runs it in mpmath at 60 digits.  `normalise_row` is
the dN -> dN/dp step (:295-304) and the CR normalisation (:733-790, thermal area zero: C4) in the same two arithmetics.

Crafted tallies: `impulse_launches` (one lit cell per zone) and `dense_tallies` (power laws over > 60 decades).  The profile's gam_sf is
edited per launch (`set_gammas`): the consumers take gam_sf and ux as two independent tables.
"""
import ctypes as ct
import math

import numpy as np

from conftest import make_problem, mcs, oracle_backend, orc

C = mcs.constants.C
U = 2.0 ** -53                                  # unit roundoff of fp64

SMALL_BINNING = dict(num_psd_bins_per_decade=(2, 2), psd_linear_cosine_bins=7, psd_log_theta_decs=1)      # nm = 32, nt = 9
# the largest binning mcs_create accepts (nm + 1, nt + 1 <= MCS_PSD_MAX = 200): nm = 199, nt = 199.  13 momentum bins per decade over the
# 15.2 decades up to 7e9 m_p c (the default 1e10 m_p c gives more than 199, 12 per decade 186); 20 angle bins per decade over 4 decades
# and 119 linear cosine bins
LARGE_BINNING = dict(num_psd_bins_per_decade=(13, 20), psd_linear_cosine_bins=119, psd_log_theta_decs=4, maximum_energy=(0.0, 0.0, 7.0e9))

G_EDGE = 1.000001                               # transformers.jl:639: beta = 0 below this
GAMMAS = (1.0, 1.0000005, float(np.nextafter(G_EDGE, 0.0)), G_EDGE, float(np.nextafter(G_EDGE, 2.0)), 1.03142, 1.5, 5.0, 50.0)
T66 = 1.0e-66                                   # the "lit" threshold, spelled <, <= and > in the three consumers
WEIGHTS = (1.0, T66, float(np.nextafter(T66, 0.0)), float(np.nextafter(T66, 1.0)), 1.0e-99, 1.0e60)
FRAMES_2D = ((None, None), (1.0, 0.0), (1.25, 0.6), (50.0, math.sqrt(1 - 1 / 50.0 ** 2)))     # (None, None): the problem's (gam0, beta0)

# Largest |oracle - mpmath| of one impulse cell's normalised dN/dp row, summed over the bins, in units of the cell's weight psd / gamma
# and divided by gamma^2 of the frame, over the whole sweep of test_consumers_cells.py (every cell x 9 gammas x 2 frames for protons,
# x 3 gammas for the Fe-like ion and the electrons; weights 1 and 1e60).  The Lorentz transform of a forward corner cancels,
# p_x - beta E / c ~ p / (2 gamma^2), so the fp64 error of a corner grows with gamma^2: 2.2e-12 of the weight at gamma = 50, 2.1e-14 at
# gamma = 5, both 8.7e-16 gamma^2.  MEASURED: 1.5e-14 (protons, gamma = 1.000001, the last angle row, momentum bin 3, where the
# transformed p_x of the cell passes through zero; Fe-like ion 5.4e-15, electrons 1.2e-15; gcc 13, x86-64).  Asserted with a margin of
# 4 for another libm or compiler.  Below that sit the knife-edge ties of the beta = 0 frames (every transformed corner lies on a bin
# edge and the rounding of log10 decides the side: about 1e-15 of the weight changes bins) and the rounding of the last bin's
# "cell_weight - fractional_area".
IMPULSE_ERR_MEASURED = 1.5e-14
IMPULSE_ERR_BOUND = 4 * IMPULSE_ERR_MEASURED


# ---- arithmetics ---------------------------------------------------------------------------------------------------------------
_dp = ct.POINTER(ct.c_double)
_LIB = None


def det_log10(x):
    """mcsm::log10 (include/mcs_math.h) through the oracle library's function table: what kernel and oracle call log10."""
    global _LIB
    if _LIB is None:
        _LIB = orc.load("det", mcs.capi)
    a = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64).ravel()
    out = np.zeros_like(a)
    assert _LIB.orc_eval_fn(mcs.capi.FN["log10"], len(a), a.ctypes.data_as(_dp), a.ctypes.data_as(_dp), out.ctypes.data_as(_dp)) == 0
    return out.reshape(np.shape(x))


class F64:
    """Python floats: the kernel's own arithmetic."""
    @staticmethod
    def num(x):
        return float(x)

    sqrt = staticmethod(math.sqrt)

    @staticmethod
    def log10(x):
        return float(det_log10([x])[0])


class MP:
    """mpmath at 60 significant digits."""
    def __init__(self, digits=60):
        import mpmath
        self.ctx = mpmath.mp.clone()
        self.ctx.dps = digits

    def num(self, x):
        return self.ctx.mpf(x)

    def sqrt(self, x):
        return self.ctx.sqrt(x)

    def log10(self, x):
        return self.ctx.log10(x)


# ---- one PSD cell in one frame ---------------------------------------------------------------------------------------------------
def corner(A, gam, beta, E0, p_edge, cos_edge):
    """One transformed corner (transformers.jl:662-676) -> (log10 of the momentum, cosine).  The edges come in cgs and as true
    cosines (C1, C2); hypot is spelled sqrt(a*a + b*b) as in the library."""
    c = A.num(C)
    px = p_edge * cos_edge
    pc = p_edge * c
    etot = A.sqrt(pc * pc + E0 * E0)
    pxt = gam * (px - beta * etot / c)
    ptt = A.sqrt(p_edge * p_edge + pxt * pxt - px * px)
    return A.log10(ptt), pxt / ptt


def frame_beta(A, gam):
    """transformers.jl:639, the frame's one "administrative constant": formed in fp64 in either arithmetic and then taken as given.
    1 - 1 / gam^2 cancels: just above gam = 1.000001 the fp64 beta is 5e-11 (relative) off the exact one, and a high-precision beta
    would put 6e-10 of a cell's weight into other bins than the reference's own fp64 statement does (measured) -- the conditioning
    of the formula, not a property of the code under test, whose sqrt the fp64 form checks bit by bit."""
    g = float(gam)
    return A.num(math.sqrt(1 - 1 / (g * g)) if g >= G_EDGE else 0.0)


def identify_corners(pts, cts):
    """identify_corners.jl:30-245 on the four corners (i,j), (i+1,j), (i,j+1), (i+1,j+1) -> (pt_lo_pt, pt_hi_pt, ct_lo_pt, ct_hi_pt),
    or None on one of its error() paths (C6).  findmin / findmax / maxloc / minloc take the first of equal entries (C3)."""
    mask = [True] * 4
    i_lo = min(range(4), key=lambda q: (pts[q], q))
    pt_lo_pt, pt_lo_ct = pts[i_lo], cts[i_lo]
    mask[i_lo] = False
    lo_tied = 1 if sum(1 for q in range(4) if pts[q] == pt_lo_pt) > 1 else 0
    i_hi = min(range(4), key=lambda q: (-pts[q], q))
    pt_hi_pt, pt_hi_ct = pts[i_hi], cts[i_hi]
    mask[i_hi] = False
    hi_tied = 1 if sum(1 for q in range(4) if pts[q] == pt_hi_pt) > 1 else 0
    rest = [q for q in range(4) if mask[q]]
    if not rest:
        return None
    j_hi = min(rest, key=lambda q: (-cts[q], q))
    ct_hi_pt, ct_hi_ct = pts[j_hi], cts[j_hi]
    mask[j_hi] = False
    rest = [q for q in range(4) if mask[q]]
    if not rest:
        return None
    j_lo = min(rest, key=lambda q: (cts[q], q))
    ct_lo_pt, ct_lo_ct = pts[j_lo], cts[j_lo]
    if ct_hi_ct == ct_lo_ct:                                       # :106-123
        if ct_hi_pt > ct_lo_pt:
            pass
        elif ct_hi_pt < ct_lo_pt:
            ct_hi_pt, ct_hi_ct, ct_lo_pt, ct_lo_ct = pts[j_lo], cts[j_lo], pts[j_hi], cts[j_hi]
        else:
            return None
    if lo_tied:                                                    # :131-182
        if pt_lo_pt == ct_lo_pt:
            if pt_lo_ct > ct_lo_ct:
                pt_lo_pt, pt_lo_ct, ct_lo_pt, ct_lo_ct = pts[j_lo], cts[j_lo], pts[i_lo], cts[i_lo]
            elif not pt_lo_ct < ct_lo_ct:
                return None
        elif pt_lo_pt == ct_hi_pt:
            if pt_lo_ct > ct_hi_ct:
                pt_lo_pt, pt_lo_ct, ct_hi_pt, ct_hi_ct = pts[j_hi], cts[j_hi], pts[i_lo], cts[i_lo]
            elif not pt_lo_ct < ct_hi_ct:
                return None
        else:
            return None
    if hi_tied:                                                    # :184-236
        if pt_hi_pt == ct_lo_pt:
            if pt_hi_ct > ct_lo_ct:
                pt_hi_pt, pt_hi_ct, ct_lo_pt, ct_lo_ct = pts[j_lo], cts[j_lo], pts[i_hi], cts[i_hi]
            elif not pt_hi_ct < ct_lo_ct:
                return None
        elif pt_hi_pt == ct_hi_pt:
            if pt_hi_ct > ct_hi_ct:
                pt_hi_pt, pt_hi_ct, ct_hi_pt, ct_hi_ct = pts[j_hi], cts[j_hi], pts[i_hi], cts[i_hi]
            elif not pt_hi_ct < ct_hi_ct:
                return None
        else:
            return None
    return pt_lo_pt, pt_hi_pt, ct_lo_pt, ct_hi_pt


def triangular_parts(A, p_hi, p_lo, ct_lo_pt, ct_hi_pt, w, l_lo, l_hi, lb):
    """triangular_distribution! with i_approx = 2 (transformers.jl:209-312) -> [(bin, part)] in the order it adds them.  Replicated as
    written: ct_height = 2 w / length_tot with length_tot = 1 / (p_hi - p_lo)."""
    out = []
    length_tot = 1 / (p_hi - p_lo)
    ct_height = 2 * w / length_tot
    p_bottom = p_lo
    p_peak = (ct_lo_pt + ct_hi_pt) / 2
    p_denom_lo = 1 / (p_peak - p_lo)
    p_denom_hi = 1 / (p_hi - p_peak)
    done = A.num(0.0)
    for l in range(l_lo, l_hi + 1):
        if l + 1 >= len(lb):                                       # (no bin above the table's last edge)
            break
        if p_hi < lb[l_lo + 1]:
            out.append((l, w))
            break
        top = lb[l + 1]
        if top <= p_peak:
            base = top - p_bottom
            rh = (top - p_lo) * p_denom_lo * ct_height
            lh = A.num(0.0) if p_bottom == p_lo else (p_bottom - p_lo) * p_denom_lo * ct_height
            part = base / 2 * (lh + rh)
            out.append((l, part))
            p_bottom = top
            done = done + part
            continue
        if top < p_hi:
            base = p_hi - top
            lh = base * p_denom_hi * ct_height
            missing = base / 2 * lh
            part = (w - done) - missing
            out.append((l, part))
            p_bottom = top
            done = done + part
            continue
        out.append((l, w - done))
        break
    return out


def cell_parts(A, p_edges, c_edges, psd_value, E0, gam, lb, nm):
    """What get_dNdp_cr does with ONE cell of the PSD in the frame of Lorentz factor `gam`: p_edges = (lower, upper) momentum edge
    [cgs], c_edges = the two cosine edges, psd_value = the cell's content, E0 = rest energy, lb = log10 of all momentum edges (an
    fp64 table in both arithmetics) -> ([(bin, part)], n_corner_errors, n_clamps): the two counts are what the cell adds to diag."""
    if float(psd_value) < T66:                                     # transformers.jl:40
        return [], 0, 0
    g = A.num(gam)
    beta = frame_beta(A, gam)
    w = A.num(psd_value) / g
    e0 = A.num(E0)
    pts, cts = [], []
    for ce in c_edges:                                             # (i,j), (i+1,j), (i,j+1), (i+1,j+1)
        for pe in p_edges:
            lp, ctv = corner(A, g, beta, e0, A.num(pe), A.num(ce))
            pts.append(lp); cts.append(ctv)
    ident = identify_corners(pts, cts)
    if ident is None:
        return [], 1, 0
    return _spread(A, ident, w, lb, nm)


def _spread(A, ident, w, lb, nm):
    p_lo, p_hi, ct_lo_pt, ct_hi_pt = ident
    clamps = 0
    first = next((l for l in range(len(lb)) if lb[l] > p_lo), None)          # findfirst(>(p_cell_lo)) - 1
    l_lo = first - 1 if first is not None else -1
    if l_lo < 0:                                                   # transformers.jl:68-74 (C6: counted, not warned)
        l_lo = nm; clamps += 1
    l_hi = next((l for l in range(l_lo, len(lb)) if lb[l] >= p_hi), None)    # findnext(>=(p_cell_hi), ., l_lo)
    if l_hi is None:                                               # :86-92
        l_hi = nm; clamps += 1
    return triangular_parts(A, p_hi, p_lo, ct_lo_pt, ct_hi_pt, w, l_lo, l_hi, lb), 0, clamps


def corner_tables_f64(gam, E0, pe, ce):
    """All transformed corners of one frame at once, [j][i], in the kernel's arithmetic (numpy: one rounding per operation)."""
    beta = math.sqrt(1 - 1 / (gam * gam)) if gam >= G_EDGE else 0.0
    p = np.asarray(pe)[None, :]; cs = np.asarray(ce)[:, None]
    px = p * cs
    pc = p * C
    etot = np.sqrt(pc * pc + E0 * E0)
    pxt = gam * (px - beta * etot / C)
    ptt = np.sqrt(p * p + pxt * pxt - px * px)
    return det_log10(ptt), pxt / ptt


def zone_parts_f64(psd_zone, gam, E0, pe, ce, lb, nm, nt, tables=None):
    """The fp64 one-cell form over every cell of a zone's slab psd_zone [nt+2][nm+2] -> (parts {bin: [part, ...]} in the reference's
    cell order (j outer, i inner), n_corner_errors, n_clamps).  Same operations as `cell_parts(F64, ...)`, corners from one table."""
    lpt, ctt = tables if tables is not None else corner_tables_f64(gam, E0, pe, ce)
    lpt, ctt = lpt.tolist(), ctt.tolist()
    lbl = [float(v) for v in lb]
    parts, errs, clamps = {}, 0, 0
    js, ks = np.nonzero(psd_zone[:nt + 1, :nm + 1] >= T66)
    for j, i in zip(js.tolist(), ks.tolist()):
        w = float(psd_zone[j, i]) / gam
        pts = [lpt[j][i], lpt[j][i + 1], lpt[j + 1][i], lpt[j + 1][i + 1]]
        cts = [ctt[j][i], ctt[j][i + 1], ctt[j + 1][i], ctt[j + 1][i + 1]]
        ident = identify_corners(pts, cts)
        if ident is None:
            errs += 1
            continue
        pp, _, cl = _spread(F64, ident, w, lbl, nm)
        clamps += cl
        for l, v in pp:
            parts.setdefault(l, []).append(v)
    return parts, errs, clamps


def normalise_row(A, dN, pe, n0, gam0, ux1, gam_z, ux_z, pop_z):
    """dN(p) of one zone and frame, bins 0..nm -> the normalised dN/dp row: particle_counter.jl:295-304, then :733-790 with no thermal
    area (C4).  Unlit bins come back as 1e-99.  Also returns the factor `norm` (0 for a dark zone)."""
    nb = len(dN)
    dp = [A.num(pe[l + 1]) - A.num(pe[l]) for l in range(nb)]
    d = [None if x < T66 else x / dp[l] for l, x in enumerate(dN)]
    area = A.num(0.0)
    for l in range(nb):
        if d[l] is not None and d[l] > 1.0e-99:
            area = area + d[l] * dp[l]
    if area > 0:
        density_pf = A.num(n0) * A.num(gam0) * A.num(ux1) / (A.num(gam_z) * A.num(ux_z))
        area_tot = density_pf / A.num(ux_z) + area
    else:
        area_tot = area
    norm = A.num(pop_z) / area_tot if area_tot > 0 else A.num(0.0)
    return [A.num(1.0e-99) if x is None else (x * norm if x > 1.0e-99 else x) for x in d], norm


def shock_frame_row(psd_zone):
    """particle_counter.jl:81-85: per momentum column, the positive cells added in ascending angle order, all nt+2 rows."""
    acc = np.zeros(psd_zone.shape[1])
    for j in range(psd_zone.shape[0]):
        acc = acc + np.where(psd_zone[j] > 0, psd_zone[j], 0.0)
    return acc


# ---- dense references: every output judged against the sum of its own addends ------------------------------------------------------------
K_BOUND = 2.0         # first-order rounding bounds are doubled: second-order terms and the reference's own final roundings


def dndp_cr_reference(prob, t, f, zones=None):
    """Reference of dndp_cr on dense tallies with a bound PER BIN -> (ref, bound, diag), ref / bound [3][n_grid][nm+2].

    Every part that a cell sends to a bin is computed by the fp64 one-cell form, which the impulse tier shows to equal the oracle's
    (and the device's) part bit for bit.  A bin l of a zone and frame receives n_l parts p_1..p_n; the reference combines them with
    math.fsum (the exactly rounded sum) and keeps A_l = sum |p_i|.  Code under test adds the same parts one by one in some order
    (serial on the host, LDS atomics on the device): |sum - exact| <= (n_l - 1) u A_l to first order, u = 2^-53.  The division by
    dp adds one rounding.  The normalisation multiplies by pop / (density + area), area = sum_j d_j dp_j over the <= nm + 1 lit bins:
    each product rounds once, the serial sum (nm + 1 positive terms) nm times, and the d_j carry their own (n_j - 1) u A_j / dp_j, so
    the area is off by at most (n_z + nm + 2) u kappa area, n_z = max_j n_j, kappa = sum_j A_j / sum_j |fsum_j| (1 without
    cancellation); three more roundings make the factor.  Together, for the normalised output d_l:
        |d_l - ref_l| <= (n_l + n_z + nm + 8) u kappa (A_l / dp_l) norm,
    asserted with the factor K_BOUND.  It scales with the bin's own A_l, never with the largest entry of the array.  Frame 0 (shock
    frame): the parts are the column's positive cells, rows 0..nt+1.  Zones not in `zones` (default: all) come back as NaN bounds."""
    P = prob.params
    L = mcs.capi.Layout(P)
    nm, nt, ng = P.num_psd_mom_bins, P.num_psd_tht_bins, P.n_grid
    NM = nm + 2
    psd = L.view(f, "psd")
    pe, ce, lb = t.mom_edge_cgs, t.cos_edge, t.mom_log_cgs
    dp = np.diff(pe)
    ref = np.zeros((3, ng, NM)); bound = np.full((3, ng, NM), np.nan)
    diag = np.zeros(2, dtype=np.int64)
    tabs = {}
    for z in (range(1, ng + 1) if zones is None else zones):
        slab = psd[z - 1]
        for m in range(3):
            if m == 0:
                parts = {k: [float(v) for v in slab[:, k] if v > 0] for k in range(NM)}
            else:
                gam = float(prob.gam_sf[z]) if m == 1 else float(t.gam0)
                if gam not in tabs:
                    tabs[gam] = corner_tables_f64(gam, t.rest_energy, pe, ce)
                parts, e, c = zone_parts_f64(slab, gam, t.rest_energy, pe, ce, lb, nm, nt, tabs[gam])
                diag += (e, c)
            S = [math.fsum(parts.get(l, ())) for l in range(nm + 1)]
            Aabs = [math.fsum(abs(v) for v in parts.get(l, ())) for l in range(nm + 1)]
            n = [len(parts.get(l, ())) for l in range(nm + 1)]
            row, norm = normalise_row(F64, S, pe, t.n0, t.gam0, prob.ux[1], prob.gam_sf[z], prob.ux[z], t.zone_pop[z - 1])
            ref[m, z - 1, :nm + 1] = row
            ref[m, z - 1, nm + 1] = math.fsum(parts.get(nm + 1, ())) if m == 0 else 0.0
            lit = [l for l in range(nm + 1) if row[l] > 1.0e-99]
            tot = math.fsum(abs(S[l]) for l in lit)
            kappa = math.fsum(Aabs[l] for l in lit) / tot if tot > 0 else 1.0
            n_z = max(n) if n else 0
            for l in range(nm + 1):
                bound[m, z - 1, l] = K_BOUND * (n[l] + n_z + nm + 8) * U * kappa * Aabs[l] / dp[l] * norm if row[l] > 1.0e-99 else 0.0
            nl = len(parts.get(nm + 1, ()))
            bound[m, z - 1, nm + 1] = K_BOUND * nl * U * abs(ref[m, z - 1, nm + 1])
    return ref, bound, diag


def _rebin(P, pt, cs, E0, gam_x, beta_x):
    """Centre-point rebin of the cells (thermo_calcs.jl:187-211, particle_counter.jl:562-596): the bin of the transformed centre through
    get_psd_bin_momentum / get_psd_bin_angle (src/get_psd_bins.jl:16-39, 73-97), with the library's log10."""
    nm, nt = P.num_psd_mom_bins, P.num_psd_tht_bins
    px = pt * cs
    pc = pt * C
    et = np.sqrt(pc * pc + E0 * E0)
    pxX = gam_x * (px - beta_x * et / C)
    ptX = np.sqrt(pt * pt - px * px + pxX * pxX)
    kb = np.where(ptX < P.psd_mom_min, 0, np.trunc(det_log10(ptX / P.psd_mom_min) * P.psd_bins_per_dec_mom).astype(int) + 1)
    kb = np.minimum(kb, nm)
    cc = -pxX / ptX
    th = np.arccos(np.clip(cc, -1, 1))
    jl = np.where(th < P.psd_tht_min, 0, np.trunc(det_log10(np.maximum(th, 1e-300) / P.psd_tht_min) * P.psd_bins_per_dec_tht).astype(int) + 1)
    jb = np.minimum(np.where(cc < P.psd_cos_fine, nt - np.trunc((cc + 1) / P.psd_dcos).astype(int), jl), nt)
    return jb, kb


def _group(idx_j, idx_k, vals):
    out = {}
    for j, k, v in zip(idx_j.tolist(), idx_k.tolist(), vals.tolist()):
        out.setdefault((j, k), []).append(v)
    return out


def dndp_2d_reference(prob, t, f, i64, gam_x, beta_x):
    """Reference of dndp_2d (get_dNdp_2D, particle_counter.jl:343-627) with a bound PER OUTPUT CELL -> (ref, bound) [n_grid][nt+2][nm+2].

    All addends are positive.  A slab cell is (1e-99 [+ therm_sf] [+ psd]) / dp: three roundings.  The density is the sum of the N lit
    cells in some order, |error| <= (N + 2) u dens; norm = pop / (dens [+ n0]) two more.  An addend of an output cell is
    ((sf norm) dp_k) / dp_kX: three more roundings, so each addend is within (N + 10) u of itself, and the n_c addends of the cell
    (onto the 1e-99 it starts from) are added in some order: n_c u A_c.  Together |out - ref| <= (n_c + N + 10) u A_c, asserted with
    the factor K_BOUND; A_c = the sum of the cell's own addends."""
    P = prob.params
    L = mcs.capi.Layout(P)
    nm, nt, ng = P.num_psd_mom_bins, P.num_psd_tht_bins, P.n_grid
    psd, ths = L.view(f, "psd"), L.view(f, "therm_sf")
    dp = np.diff(t.mom_edge_cgs)
    K, J = np.meshgrid(np.arange(nm + 1), np.arange(nt + 1))
    jb, kb = _rebin(P, t.pt_center[K], t.cos_center[J], t.rest_energy, gam_x, beta_x)
    ref = np.full((ng, nt + 2, nm + 2), 1.0e-99); bound = np.zeros((ng, nt + 2, nm + 2))
    for z in range(1, ng + 1):
        nc = int(i64[z - 1])
        sf = np.full((nt + 2, nm + 2), 1.0e-99)
        if nc != 0 and t.therm_from_hist:
            sf = sf + ths[z - 1]
        w = np.zeros_like(sf); w[:nt + 1, :nm + 1] = psd[z - 1][:nt + 1, :nm + 1]
        sf = np.where(w > T66, sf + w, sf)
        sf[:, :nm + 1] = np.where(sf[:, :nm + 1] > T66, sf[:, :nm + 1] / dp[None, :], sf[:, :nm + 1])
        lit = sf > T66
        N = int(lit.sum())
        dens = math.fsum(sf[lit].tolist())
        if nc == 0 and dens > 0:
            dens += t.n0
        norm = t.zone_pop[z - 1] / dens if dens > 0 else 0.0
        v = np.where((sf > 1.0e-99) & (norm > 0), sf * norm, 1.0e-99)[:nt + 1, :nm + 1]
        sel = v > T66
        add = (v * dp[None, :]) / dp[kb]
        for (j, k), vals in _group(jb[sel], kb[sel], add[sel]).items():
            A = math.fsum(vals)
            ref[z - 1, j, k] = 1.0e-99 + A
            bound[z - 1, j, k] = K_BOUND * (len(vals) + N + 10) * U * A
    return ref, bound


def thermo_reference(prob, t, f, i64):
    """Reference of thermo_calcs (thermo_calcs.jl:30-352) with a bound PER ZONE AND OUTPUT -> (ref, bound) [3][n_grid].

    A cell of the plasma-frame array collects n_c positive addends: n_c u.  The normalisation sums the N lit cells, and the
    population sums them again after the multiplication: (2 N + 2 n_z + 6) u on every normalised cell and on pop / zone_pop.  A
    pressure term c pfac cos^2 has eight more roundings and the N terms are summed in some order; the terms are positive.  The cold
    pressure enters as coef p_cold (1 - pop / zone_pop), whose cancellation is covered by counting coef p_cold (1 + pop / zone_pop)
    into A.  |out - ref| <= (3 N + 2 n_z + 16) u A with A = sum of the terms + coef p_cold (1 + pop / zone_pop), asserted with K_BOUND."""
    P = prob.params
    L = mcs.capi.Layout(P)
    nm, nt, ng = P.num_psd_mom_bins, P.num_psd_tht_bins, P.n_grid
    psd, thp = L.view(f, "psd"), L.view(f, "therm_pf")
    E0, mc = t.rest_energy, t.mc
    K, J = np.meshgrid(np.arange(nm + 1), np.arange(nt + 1))
    pt, cs = t.pt_center[K], t.cos_center[J]
    tq = pt / mc
    gtmp = np.sqrt(1 + tq * tq)
    vel = pt * C / (mc * gtmp)
    coef = (1.0 / 3, 2.0 / 3, 1.5)
    ref = np.zeros((3, ng)); bound = np.zeros((3, ng))
    for z in range(1, ng + 1):
        nc = int(i64[z - 1])
        base = np.full((nt + 2, nm + 2), 1.0e-99)
        if t.therm_from_hist:
            base = base + thp[z - 1]
        w = psd[z - 1][:nt + 1, :nm + 1]
        sel = w > T66
        jb, kb = _rebin(P, pt, cs, E0, float(prob.gam_sf[z]), float(prob.ux[z]) / C)
        d2 = base.copy()
        n_z = 0
        for (j, k), vals in _group(jb[sel], kb[sel], w[sel]).items():
            d2[j, k] = math.fsum([base[j, k]] + vals)
            n_z = max(n_z, len(vals))
        lit = d2 > T66
        N = int(lit.sum())
        nf = math.fsum(d2[lit].tolist())
        if nc == 0 and nf > 0:
            nf += t.n0 / prob.ux[z]
        if nf > 0:
            nf = t.zone_pop[z - 1] / nf
        d2 = np.where(lit, d2 * nf, d2)
        pop = math.fsum(d2[d2 > T66].tolist())
        ploc = t.cold_pressure[z - 1]
        share = pop / t.zone_pop[z - 1]
        if d2.max() < T66 and nc == 0:
            ref[:, z - 1] = [cf * ploc for cf in coef]
            bound[:, z - 1] = [K_BOUND * 2 * U * cf * ploc for cf in coef]
            continue
        cold = ploc * (1 - share) if nc == 0 else 0.0
        dens = t.density_loc[z - 1] / t.zone_pop[z - 1]
        c = d2[:nt + 1, :nm + 1]
        c = np.where(c < T66, 0.0, c)
        pfac = 1.0 / 3 * pt * vel * dens
        terms = (c * pfac * (cs * cs), c * pfac * (1 - cs * cs), (gtmp - 1) * E0 * c * dens)
        for q in range(3):
            s = math.fsum(terms[q].ravel().tolist())
            ref[q, z - 1] = coef[q] * cold + s
            A = s + (coef[q] * ploc * (1 + share) if nc == 0 else 0.0)
            bound[q, z - 1] = K_BOUND * (3 * N + 2 * n_z + 16) * U * A
    return ref, bound


def excess(got, ref, bound):
    """Largest |got - ref| / bound over the entries with a positive bound (0 if none), and whether all others are equal to ref."""
    pos = bound > 0
    r = float(np.max(np.abs(got - ref)[pos] / bound[pos])) if pos.any() else 0.0
    return r, bool(np.array_equal(got[~pos], ref[~pos]))


def own_size_excess(got, want, n_adds):
    """For outputs that are sums of positive addends (real tallies: no cancellation): the largest |got - want| / (K_BOUND n_adds u want)
    over the lit entries (> 1e-90) -- each entry is judged against its own value.  n_adds broadcasts against the arrays."""
    lit = want > 1.0e-90
    if not lit.any():
        return 0.0
    b = K_BOUND * np.broadcast_to(n_adds, want.shape)[lit] * U * want[lit]
    return float(np.max(np.abs(got - want)[lit] / b))


def lit_cells_per_zone(L, f, names=("psd",)):
    """Per zone, the number of slab cells above 1e-66 summed over the named histograms: an upper bound of the number of addends of
    any output of that zone."""
    return sum((L.view(f, name) > T66).sum(axis=(1, 2)) for name in names)


# ---- problems and tables -----------------------------------------------------------------------------------------------------------
def small_problem(**kw):
    return make_problem(64, **{**SMALL_BINNING, **kw})


def three_species_problem():
    """protons, an Fe-like ion and electrons on the small binning: the species scalars of tier 2."""
    S = mcs.inputs.Species
    return small_problem(species=[S(1.0, 1.0, 1e6, 1.0), S(56.0, 26.0, 1e6, 1e-4), S(mcs.constants.ME / mcs.constants.MP, -1.0, 1e6, 1.0)])


def set_gammas(prob, gam_zone):
    """gam_sf of zones 1..n_grid replaced (the ghost entries 0 and n_grid+1 copy their neighbours); ux is left alone."""
    g = np.asarray(prob.gam_sf, dtype=np.float64).copy()
    g[1:len(gam_zone) + 1] = gam_zone
    g[0], g[-1] = g[1], g[-2]
    prob.gam_sf = g


def tables(prob0, prob, i_ion, hist=True):
    """consumer_tables of the edited problem; density_loc and cold_pressure, which divide by sqrt(gam_sf^2 - 1), are taken from the
    unedited profile `prob0` so that they stay finite where gam_sf was set to 1."""
    t = mcs.consumers.consumer_tables(prob, i_ion, therm_from_hist=hist)
    t0 = mcs.consumers.consumer_tables(prob0, i_ion, therm_from_hist=hist)
    t.density_loc, t.cold_pressure = t0.density_loc, t0.cold_pressure
    assert np.all(np.isfinite(t.density_loc)) and np.all(np.isfinite(t.cold_pressure)) and np.all(np.isfinite(t.zone_pop))
    return t


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- crafted tallies -----------------------------------------------------------------------------------------------------------------
class Launch:
    """One set of tallies with the profile that goes with it."""
    def __init__(self, f, i, gam_zone, cells, frame):
        self.f, self.i, self.gam_zone, self.cells, self.frame = f, i, gam_zone, cells, frame      # cells: {zone: (j, k, value)}


def impulse_launches(prob, n_cell_classes=None):
    """The impulse sweep: every cell (j, k) of the (nt+2) x (nm+2) slab meets every gamma of GAMMAS, one lit psd cell per zone.
    Pairs (cell, gamma) are dealt to the lit zones in order, so a launch mixes all gammas over its zones and the assignment moves on
    from launch to launch.  Weights cycle through WEIGHTS with cell + gamma index; at gamma = 1 every sixth cell holds 1e-66 exactly.
    Every ninth zone has a dark psd: in turn it is empty with no crossings (cold-pressure branch), or holds one lit cell of therm_pf
    and therm_sf with crossings, or the same with none.  Lit zones alternate num_crossings = 0 / 3.  The frame of dndp_2d cycles
    through FRAMES_2D.  n_cell_classes: deal only every cell's first so many gammas, rotated by the cell index (a shorter sweep)."""
    P = prob.params
    L = mcs.capi.Layout(P)
    nm, nt, ng = P.num_psd_mom_bins, P.num_psd_tht_bins, P.n_grid
    NM, NT = nm + 2, nt + 2
    ncls = len(GAMMAS) if n_cell_classes is None else n_cell_classes
    pairs = [(c, (c + s) % len(GAMMAS)) for c in range(NM * NT) for s in range(ncls)]
    lit_zones = [z for z in range(1, ng + 1) if z % 9]
    out = []
    for r in range(0, len(pairs), len(lit_zones)):
        n = len(out)
        f = np.zeros(L.total); i = np.zeros(L.n_i64, dtype=np.int64)
        psd, tsf, tpf = L.view(f, "psd"), L.view(f, "therm_sf"), L.view(f, "therm_pf")
        gam_zone = np.array([GAMMAS[(z + n) % len(GAMMAS)] for z in range(1, ng + 1)])
        cells = {}
        for z, (c, g) in zip(lit_zones, pairs[r:r + len(lit_zones)]):
            j, k = divmod(c, NM)
            v = WEIGHTS[(c + g) % len(WEIGHTS)]
            psd[z - 1, j, k] = v
            gam_zone[z - 1] = GAMMAS[g]
            cells[z] = (j, k, v)
            i[z - 1] = 0 if z % 2 else 3
        for z in range(9, ng + 1, 9):
            d = z // 9 + n
            if d % 3 == 0:
                continue
            j, k = divmod((7 * d + 3 * n) % (NM * NT), NM)
            tpf[z - 1, j, k] = WEIGHTS[d % len(WEIGHTS)]
            tsf[z - 1, (j + 1) % NT, (k + 5) % NM] = WEIGHTS[(d + 1) % len(WEIGHTS)]
            i[z - 1] = 7 if d % 3 == 1 else 0
        out.append(Launch(f, i, gam_zone, cells, FRAMES_2D[n % len(FRAMES_2D)]))
    return out


def dense_gammas(ng):
    return np.array([GAMMAS[(3 * z) % len(GAMMAS)] for z in range(1, ng + 1)])


def dense_tallies(prob, seed=5, lit_zones=None, decades=80.0, fill=1.0):
    """Dense tallies: per lit zone a power law in momentum over `decades` decades (slope and sign of the slope change from zone to
    zone) times a random angular pattern, a tenth of the cells 0 and a tenth 1e-99 (and of the rest all but the share `fill` 0 as well),
    rows nt+1 and column nm+1 filled too; therm_sf / therm_pf get a narrower random pattern; every fifth zone stays dark; num_crossings cycles 0, 0, 4.  gam_sf: `dense_gammas`."""
    P = prob.params
    L = mcs.capi.Layout(P)
    nm, nt, ng = P.num_psd_mom_bins, P.num_psd_tht_bins, P.n_grid
    NM, NT = nm + 2, nt + 2
    rng = np.random.default_rng(seed)
    f = np.zeros(L.total); i = np.zeros(L.n_i64, dtype=np.int64)
    psd, tsf, tpf = L.view(f, "psd"), L.view(f, "therm_sf"), L.view(f, "therm_pf")
    zones = [z for z in range(1, ng + 1) if z % 5] if lit_zones is None else list(lit_zones)
    for z in zones:
        slope = decades / NM * rng.uniform(0.8, 1.0)               # falling with momentum in odd zones, rising in even ones
        k = np.arange(NM)
        law = 10.0 ** (10.0 - slope * (k if z % 2 else NM - 1 - k))          # 1e10 down to 1e-70: the last bins fall below 1e-66
        cellsv = law[None, :] * 10.0 ** rng.uniform(-2, 2, (NT, NM))
        u = rng.random((NT, NM))
        cellsv[u < 0.1] = 0.0
        cellsv[(u >= 0.1) & (u < 0.2)] = 1.0e-99
        cellsv[u > 0.2 + 0.8 * fill] = 0.0
        psd[z - 1] = cellsv
        th = 10.0 ** rng.uniform(-30, -10, (NT, NM)) * (rng.random((NT, NM)) < 0.3)
        tpf[z - 1] = th
        tsf[z - 1] = th[::-1, ::-1] * 3.0
        i[z - 1] = (0, 0, 4)[z % 3]
    return f, i


# ---- the impulse sweep through the oracle -----------------------------------------------------------------------------------------------
class Sweep:
    """The impulse sweep of one species through the oracle: per launch the tables and every output."""
    def __init__(self, prob0, i_ion, n_cell_classes=None):
        self.prob0, self.i_ion = prob0, i_ion
        self.prob = prob = mcs.inputs.build_problem(prob0.cfg)
        self.launches = impulse_launches(prob, n_cell_classes)
        be = oracle_backend(prob)
        P = prob.params
        self.runs = []
        for la in self.launches:
            set_gammas(prob, la.gam_zone)
            gsf = prob.gam_sf.copy()
            T = (la.f, la.i)
            t1, t0 = tables(prob0, prob, i_ion, True), tables(prob0, prob, i_ion, False)
            gx, bx = la.frame if la.frame[0] else (P.gam0, P.beta0)
            dndp, diag = be.dndp_cr(t1, tallies=T)
            self.runs.append(dict(la=la, gsf=gsf, t=(t0, t1), dndp=dndp, diag=diag, frame=(gx, bx),
                                  thermo=[np.array(be.thermo_calcs(t, tallies=T)) for t in (t0, t1)],
                                  d2=[be.dndp_2d(t, gx, bx, tallies=T).copy() for t in (t0, t1)]))
        be.destroy()


def impulse_sweeps(only=None):
    """protons: every cell x every gamma; the Fe-like ion and the electrons: every cell x three gammas, rotating with the cell."""
    make = {"protons": lambda: Sweep(small_problem(), 1), "iron": lambda: Sweep(three_species_problem(), 2, 3),
            "electrons": lambda: Sweep(three_species_problem(), 3, 3)}
    return {name: mk() for name, mk in make.items() if only in (None, name)}
