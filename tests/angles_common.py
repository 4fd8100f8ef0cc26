"""Helpers of the pitch-angle-distribution tests (test_angle_dist_host.py, test_gpu_angle_dist.py, test_gpu_ens_angles.py): crafted
tallies and a restatement of mcs_angle_dist (include/mcs.h) in plain Python floats that shares no code with csrc/mcs_consumers.hip.

The image of a cell in a moving frame is written from the statements of consumers_common._rebin (the centre-point rebin of
thermo_calcs.jl:187-211 / particle_counter.jl:562-596 through get_psd_bin_momentum / get_psd_bin_angle), with the library's own log10
and acos taken through the oracle library's function table, as consumers_common.det_log10 does.  numpy's elementwise operations
round once each and form no fma: the kernel's arithmetic, operation by operation.  The adds then go in the order the header fixes:

  weight    v = 0.0; [v = v + therm_sf[z][j][k] if therm_from_hist and num_crossings[z] != 0]; [v = v + psd[z][j][k] if psd > 1e-66]
  lit       v > 1e-66
  A[jX]     the weights of the lit cells whose image lies in row jX and in the window, added to 0.0, j ascending, k ascending
  number    ((0.0 + A[0]) + A[1]) + ... + A[nt]
  dist[j]   (A[j] / number) / (cos_edge[j+1] - cos_edge[j]) where A[j] > 0, else 1e-99; dist[nt+1] = 1e-99
  <mu>      s1 / number, s1 the serial sum of t_j = A[j] * cos_center[j];  <mu^2> = s2 / number, s2 that of t_j * cos_center[j]
            both NaN where number == 0
"""
import ctypes as ct
import math

import numpy as np

import consumers_common as cc
from conftest import mcs, orc

C = cc.C
U = cc.U
T66 = cc.T66
FLOOR = 1.0e-99
MAX_WINDOWS = 8

_dp = ct.POINTER(ct.c_double)
_LIB = None


def lib_fn(name, x):
    """A one-argument function of include/mcs_math.h through the oracle library's function table, elementwise."""
    global _LIB
    if _LIB is None:
        _LIB = orc.load("det", mcs.capi)
    a = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64).ravel()
    out = np.zeros_like(a)
    assert _LIB.orc_eval_fn(mcs.capi.FN[name], len(a), a.ctypes.data_as(_dp), a.ctypes.data_as(_dp), out.ctypes.data_as(_dp)) == 0
    return out.reshape(np.shape(x))


def image(P, t, gam, log10=None, acos=None):
    """(jX, kX) [nt+1][nm+1]: the bins of the transformed centre of every cell (j, k) in the frame of Lorentz factor `gam`, beta by
    consumers_common.frame_beta.  log10 / acos: the library's by default."""
    log10 = log10 or (lambda a: lib_fn("log10", a))
    acos = acos or (lambda a: lib_fn("acos", a))
    nm, nt = P.num_psd_mom_bins, P.num_psd_tht_bins
    gam = float(gam)
    beta = float(cc.frame_beta(cc.F64, gam))
    E0 = float(t.rest_energy)
    K, J = np.meshgrid(np.arange(nm + 1), np.arange(nt + 1))
    pt = np.asarray(t.pt_center, dtype=np.float64)[K]
    cs = np.asarray(t.cos_center, dtype=np.float64)[J]
    px = pt * cs
    pc = pt * C
    et = np.sqrt(pc * pc + E0 * E0)
    pxX = gam * (px - beta * et / C)
    ptX = np.sqrt(pt * pt - px * px + pxX * pxX)
    # get_psd_bin_momentum
    below = ptX < P.psd_mom_min
    kb = np.where(below, 0, np.trunc(log10(np.where(below, P.psd_mom_min, ptX) / P.psd_mom_min) * P.psd_bins_per_dec_mom).astype(int) + 1)
    kb = np.minimum(kb, nm)
    # get_psd_bin_angle
    c = -pxX / ptX
    th = acos(c)
    small = th < P.psd_tht_min
    jl = np.where(small, 0, np.trunc(log10(np.where(small, P.psd_tht_min, th) / P.psd_tht_min) * P.psd_bins_per_dec_tht).astype(int) + 1)
    jb = np.where(c < P.psd_cos_fine, nt - np.trunc((c + 1) / P.psd_dcos).astype(int), jl)
    jb = np.where(ptX == 0.0, 0, np.minimum(jb, nt))
    return jb, kb


_IMAGES = {}


def image_of(P, t, gam):
    key = (P.num_psd_mom_bins, P.num_psd_tht_bins, float(gam), float(t.rest_energy), np.asarray(t.pt_center).tobytes(), np.asarray(t.cos_center).tobytes())
    if key not in _IMAGES:
        if len(_IMAGES) > 64:
            _IMAGES.clear()
        _IMAGES[key] = image(P, t, gam)
    return _IMAGES[key]


def weights(psd_z, ths_z, ncross, hist, nm, nt):
    """The weight of every cell j <= nt, k <= nm of one zone, [nt+1][nm+1], in the header's order of operations."""
    v = np.zeros((nt + 1, nm + 1))
    if hist and int(ncross) != 0:
        v = v + ths_z[:nt + 1, :nm + 1]
    w = psd_z[:nt + 1, :nm + 1]
    with np.errstate(invalid="ignore"):
        v = np.where(w > T66, v + w, v)
    return v


def row_sums(v, jb, kb, windows, nt):
    """A [n_win][nt+1] as Python floats: the lit cells in cell order, each added to the accumulator of its image's row for every
    window that holds its image's momentum bin.  Also the number of lit cells."""
    A = [[0.0] * (nt + 1) for _ in windows]
    with np.errstate(invalid="ignore"):
        js, ks = np.nonzero(v > T66)                                   # (row-major: j ascending, within a row k ascending)
    for val, jx, kx in zip(v[js, ks].tolist(), jb[js, ks].tolist(), kb[js, ks].tolist()):
        for m, (lo, hi) in enumerate(windows):
            if lo <= kx < hi:
                A[m][jx] = A[m][jx] + val
    return A, len(js)


def finish(A_m, cos_edge, cos_center, nt):
    """One row: (dist [nt+2], number, <mu>, <mu^2>) from its A [nt+1]."""
    number = 0.0
    s1 = 0.0
    s2 = 0.0
    for j in range(nt + 1):
        tj = A_m[j] * cos_center[j]
        number = number + A_m[j]
        s1 = s1 + tj
        s2 = s2 + tj * cos_center[j]
    dist = [FLOOR] * (nt + 2)
    for j in range(nt + 1):
        if A_m[j] > 0:
            dist[j] = (A_m[j] / number) / (cos_edge[j + 1] - cos_edge[j])
    if number == 0.0:
        return dist, number, math.nan, math.nan
    return dist, number, s1 / number, s2 / number


class Reference:
    """mcs_angle_dist restated: dist [3][ng][n_win][nt+2], number [3][ng][n_win], moments [3][ng][n_win][2], A [3][ng][n_win][nt+1]
    (the row sums before the division) and lit [ng], the lit cells of every zone."""

    def __init__(self, dist, number, moments, A, lit):
        self.dist, self.number, self.moments, self.A, self.lit = dist, number, moments, A, lit

    @property
    def mean_mu(self):
        return np.ascontiguousarray(self.moments[..., 0])

    @property
    def mean_mu2(self):
        return np.ascontiguousarray(self.moments[..., 1])


def reference(prob, t, f, i64, windows, images=None):
    """prob: gam_sf is read (zone z, 1-based: prob.gam_sf[z]); t: the consumer tables (pt_center, cos_center, cos_edge, rest_energy,
    gam0, therm_from_hist); (f, i64): the tallies; windows ((l_lo, l_hi), ...).  images: {gam: (jb, kb)} to use instead of `image_of`."""
    P = prob.params
    L = mcs.capi.Layout(P)
    nm, nt, ng = P.num_psd_mom_bins, P.num_psd_tht_bins, P.n_grid
    psd, ths = L.view(f, "psd"), L.view(f, "therm_sf")
    nw = len(windows)
    ce = [float(x) for x in t.cos_edge]
    cc_ = [float(x) for x in t.cos_center]
    dist = np.full((3, ng, nw, nt + 2), FLOOR); number = np.zeros((3, ng, nw)); moments = np.full((3, ng, nw, 2), np.nan)
    A_all = np.zeros((3, ng, nw, nt + 1)); lit = np.zeros(ng, dtype=np.int64)
    J0, K0 = np.meshgrid(np.arange(nt + 1), np.arange(nm + 1), indexing="ij")
    for z in range(ng):
        v = weights(psd[z], ths[z], i64[z], t.therm_from_hist, nm, nt)
        with np.errstate(invalid="ignore"):
            if not np.any(v > T66):
                continue
        for fr in range(3):
            if fr == 0:
                jb, kb = J0, K0
            else:
                gam = float(prob.gam_sf[z + 1]) if fr == 1 else float(t.gam0)
                jb, kb = images[gam] if images is not None else image_of(P, t, gam)
            A, lit[z] = row_sums(v, jb, kb, windows, nt)
            for m in range(nw):
                d, n, m1, m2 = finish(A[m], ce, cc_, nt)
                dist[fr, z, m] = d; number[fr, z, m] = n; moments[fr, z, m] = (m1, m2); A_all[fr, z, m] = A[m]
    return Reference(dist, number, moments, A_all, lit)


def same_words(a, b):
    """Bit-equal, where a NaN equals a NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def assert_equal_to_reference(got, ref, what=""):
    """got: (dist, number, moments) of HipBackend.angle_dist, or an AngleDistributions."""
    if not isinstance(got, tuple):
        got = (got.dist, got.number, np.stack([got.mean_mu, got.mean_mu2], axis=-1))
    dist, number, moments = got
    assert same_words(number, ref.number), f"{what}: number differs in {(number != ref.number).sum()} words"
    assert not np.isnan(dist).any() and same_words(dist, ref.dist), f"{what}: dist differs in {(dist != ref.dist).sum()} words"
    assert same_words(moments, ref.moments), f"{what}: moments differ"


# ---- crafted tallies -------------------------------------------------------------------------------------------------------------
def impulse_launches(prob):
    """The impulse sweep: every cell (j, k) of the (nt+2) x (nm+2) slab once, one lit psd cell per zone, so a launch covers n_grid
    cells.  The cells are dealt momentum column by momentum column: a launch lights a band of columns, its images stay within a few
    bins of the band (the small binning has two bins per decade, gamma = 50 moves a momentum by two decades), and a momentum bin
    that nothing of the launch reaches exists.  The zone's gamma walks cc.GAMMAS with cell + launch index, the weight cc.WEIGHTS with cell + gamma index, the ISM
    frame's gamma cc.GAMMAS with the launch.  -> [(f, i64, gam_zone [ng], gam0, cells {zone (0-based): (j, k, value)})]"""
    P = prob.params
    L = mcs.capi.Layout(P)
    nm, nt, ng = P.num_psd_mom_bins, P.num_psd_tht_bins, P.n_grid
    NM, NT = nm + 2, nt + 2
    G, W = cc.GAMMAS, cc.WEIGHTS
    out = []
    for n, c0 in enumerate(range(0, NM * NT, ng)):
        f = np.zeros(L.total); i = np.zeros(L.n_i64, dtype=np.int64)
        psd = L.view(f, "psd")
        gam_zone = np.ones(ng)
        cells = {}
        for z, c in enumerate(range(c0, min(c0 + ng, NM * NT))):
            k, j = divmod(c, NT)
            g = (c + n) % len(G)
            v = W[(c + g) % len(W)]
            psd[z, j, k] = v
            gam_zone[z] = G[g]
            cells[z] = (j, k, v)
            i[z] = 0 if z % 2 else 3
        out.append((f, i, gam_zone, max(G[(n + 5) % len(G)], 1.0), cells))
    return out


def numpy_form(prob, t, f, i64, windows, fr, z):
    """An independent form of A of one zone and frame: the lit cells grouped by their image with numpy, every group summed exactly
    (math.fsum) -> (A [n_win][nt+1], n_adds [n_win][nt+1]).  It shares `image` and `weights` with the restatement, not the adds."""
    P = prob.params
    L = mcs.capi.Layout(P)
    nm, nt = P.num_psd_mom_bins, P.num_psd_tht_bins
    v = weights(L.view(f, "psd")[z], L.view(f, "therm_sf")[z], i64[z], t.therm_from_hist, nm, nt)
    if fr == 0:
        jb, kb = np.meshgrid(np.arange(nt + 1), np.arange(nm + 1), indexing="ij")
    else:
        gam = float(prob.gam_sf[z + 1]) if fr == 1 else float(t.gam0)
        jb, kb = image(P, t, gam)
    lit = v > T66
    A = np.zeros((len(windows), nt + 1)); n_adds = np.zeros((len(windows), nt + 1), dtype=np.int64)
    for m, (lo, hi) in enumerate(windows):
        sel = lit & (kb >= lo) & (kb < hi)
        for j in range(nt + 1):
            vals = v[sel & (jb == j)]
            A[m, j] = math.fsum(vals.tolist())
            n_adds[m, j] = vals.size
    return A, n_adds
