"""Host side of the tally consumers: the part of `ion_finalize`
(src/ion_finalize.jl:26-48) that turns the PSD into spectra and pressures.

The reductions over the 22 MB histograms run on the device (`mcs_dndp_cr`, `mcs_thermo_calcs`
in include/mcs.h); this module only builds the O(bins) / O(n_grid) tables they take and
mirrors the reference's call order.  Consumer quirks C1-C6 are listed in DESIGN.md section 3b.
"""
from __future__ import annotations

import ctypes as ct
import dataclasses
import math

import numpy as np

from . import capi
from .constants import C, KB, MP

PC_CM = 3.0856775814913674e18      # UnitfulAstro.pc in cm


def angle_edges_intended(prob) -> np.ndarray:
    """theta (rad) for the log region then cosines for the linear region, in the order
    `set_psd_angle_bins` builds them before its `sort!` (src/initializers.jl:272-279; quirk C2)."""
    P, cfg = prob.params, prob.cfg
    bpd = P.psd_bins_per_dec_tht
    lin = cfg.psd_linear_cosine_bins
    log_bins = P.num_psd_tht_bins - lin                # entries 1..log_bins hold theta
    b = [1.0e-99] + [P.psd_tht_min * (10.0 ** (1 / bpd)) ** k for k in range(log_bins)]
    b += [P.psd_cos_fine - P.psd_dcos * k for k in range(lin + 1)]
    b = np.asarray(b)
    assert len(b) == P.num_psd_tht_bins + 2, (len(b), P.num_psd_tht_bins)
    return b


def find_shock_index(x_grid: np.ndarray) -> int:
    """src/particle_counter.jl:936-947 (x_grid indexed 0..n_grid+1)."""
    for i in range(len(x_grid) - 1):
        if x_grid[i] == 0 or x_grid[i] * x_grid[i + 1] < 0:
            return i
    return 0


def set_grid_volumes(prob, i_ion: int):
    """`set_grid_volumes!` (src/particle_counter.jl:1466-1524) -> (zone_pop, zone_vol), zones 1..n_grid."""
    P, cfg = prob.params, prob.cfg
    x, ux, gsf = prob.x_grid_cm, prob.ux, prob.gam_sf
    n = P.n_grid
    i_shock = find_shock_index(x)
    dx = np.diff(x)                                  # dx[i] = x[i+1]-x[i], i = 0..n_grid
    sph = jet_sphere_fraction(cfg)
    jet_rad_cm = cfg.jet_shock_radius * PC_CM
    surf = np.zeros(n + 1)
    rad_min = jet_rad_cm - x[i_shock]
    for i in range(i_shock - 1, 0, -1):
        rad_max = rad_min + dx[i] / P.gam0
        surf[i] = math.pi * (rad_max + rad_min) ** 2 * sph
        rad_min = rad_max
    rad_max = jet_rad_cm - x[i_shock]
    for i in range(i_shock, n + 1):
        rad_min = rad_max - dx[i] / P.gam0
        surf[i] = math.pi * (rad_max + rad_min) ** 2 * sph
        rad_max = rad_min
    n0 = cfg.species[i_ion - 1].density
    zone_pop = np.zeros(n)
    zone_vol = np.zeros(n)
    for i in range(1, n + 1):
        dwell = dx[i] / ux[i]
        F_up = P.gam0 * n0 * P.beta0 * C
        zone_pop[i - 1] = F_up * surf[i] * dwell
        density_pf = P.gam0 * ux[1] / (gsf[i] * ux[i])
        zone_vol[i - 1] = zone_pop[i - 1] / density_pf
    return zone_pop, zone_vol


def jet_sphere_fraction(cfg) -> float:
    """`parse_jet_frac` (src/data_input.jl:153-167)."""
    if cfg.JETFR is None:
        return 0.0
    frac, ang = cfg.JETFR
    if 0 < frac <= 1:
        return float(frac)
    if 0 < ang <= 180:
        return (1 - math.cos(math.radians(ang))) / 2
    raise ValueError("JETFR: Unphysical values entered.")


@dataclasses.dataclass
class ConsumerTables:
    mom_log_cgs: np.ndarray
    mom_edge_cgs: np.ndarray
    cos_edge: np.ndarray
    cos_center: np.ndarray
    pt_center: np.ndarray
    zone_pop: np.ndarray
    zone_vol: np.ndarray
    density_loc: np.ndarray
    cold_pressure: np.ndarray
    rest_energy: float
    mc: float
    n0: float
    gam0: float
    therm_from_hist: int = 1

    def as_struct(self) -> capi.McsConsumerIn:
        s = capi.McsConsumerIn()
        for f in ("mom_log_cgs", "mom_edge_cgs", "cos_edge", "cos_center", "pt_center", "zone_pop", "density_loc",
                  "cold_pressure"):
            a = getattr(self, f)
            assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
            setattr(s, f, a.ctypes.data_as(capi.c_double_p))
        s.rest_energy, s.mc, s.n0, s.gam0 = self.rest_energy, self.mc, self.n0, self.gam0
        s.therm_from_hist = int(self.therm_from_hist)
        return s


def consumer_tables(prob, i_ion: int, therm_from_hist: bool = True) -> ConsumerTables:
    """Tables of get_dNdp_cr (src/particle_counter.jl:46-62), transform_psd_corners
    (src/transformers.jl:646-660) and thermo_calcs (src/thermo_calcs.jl:55-80, 246, 258-266)."""
    P, cfg = prob.params, prob.cfg
    sp = cfg.species[i_ion - 1]
    nm, nt = P.num_psd_mom_bins, P.num_psd_tht_bins
    lin = cfg.psd_linear_cosine_bins
    mb = np.asarray(prob.psd_mom_bounds, dtype=np.float64)           # log10(p / m_p c), index 0..nm+1
    mom_edge = np.ascontiguousarray(10.0 ** mb * (MP * C))           # C1: cgs
    mom_log = np.ascontiguousarray(np.log10(mom_edge))
    tb = angle_edges_intended(prob)                                  # C2
    j = np.arange(nt + 2)
    cos_edge = np.ascontiguousarray(np.where(j > nt - lin, -tb, -np.cos(tb)))
    cos_center = np.ascontiguousarray(0.5 * (cos_edge[:-1] + cos_edge[1:]))            # thermo_calcs.jl:57-73
    pt_center = np.ascontiguousarray(10.0 ** (0.5 * (mb[:-1] + mb[1:])) * (MP * C))    # thermo_calcs.jl:75-80
    zone_pop, zone_vol = set_grid_volumes(prob, i_ion)
    x, ux, gsf = prob.x_grid_cm, prob.ux, prob.gam_sf
    n = P.n_grid
    with np.errstate(divide="ignore", invalid="ignore"):
        density_loc = P.gam0 * P.beta0 * sp.density / np.sqrt(gsf[1:n + 1] ** 2 - 1)
    cold_pressure = density_loc ** (5.0 / 3.0) * KB * sp.temperature
    m = sp.aa * MP
    return ConsumerTables(mom_log, mom_edge, cos_edge, cos_center, pt_center,
                          np.ascontiguousarray(zone_pop), np.ascontiguousarray(zone_vol),
                          np.ascontiguousarray(density_loc), np.ascontiguousarray(cold_pressure),
                          m * C * C, m * C, sp.density, P.gam0, int(therm_from_hist))


@dataclasses.dataclass
class IonFinal:
    """What `ion_finalize` returns for the transport consumers (src/ion_finalize.jl:78-82)."""
    dNdp_cr: np.ndarray          # [3][n_grid][nmom+2]: shock, plasma, ISM frame; normalised dN/dp
    zone_pop: np.ndarray
    P_psd_par: np.ndarray
    P_psd_perp: np.ndarray
    energy_density_psd: np.ndarray
    diag: np.ndarray


def ion_finalize(prob, backend, i_ion: int, therm_from_hist: bool = True) -> IonFinal:
    """get_normalized_dNdp (CR part) then thermo_calcs, on the backend's resident tallies."""
    tabs = consumer_tables(prob, i_ion, therm_from_hist)
    dndp, diag = backend.dndp_cr(tabs)
    ppar, pperp, edens = backend.thermo_calcs(tabs)
    return IonFinal(dndp, tabs.zone_pop, ppar, pperp, edens, diag)


@dataclasses.dataclass
class EscapeSpectra:
    """dN/dp of the particles that leave the shock, per door (0: the upstream free-escape boundary and p_max, 1: the downstream end)
    and frame (0: shock, 1: the door's plasma frame, 2: ISM).  Not normalised to a volume: a door has none."""
    dndp: np.ndarray             # [2][3][nmom+2]; entry nmom+1 and every empty bin 1e-99
    number: np.ndarray           # [2][3]: the summed weight of each row, before the division by the bin widths
    diag: np.ndarray             # [2][2]: per door, cells skipped on identify_corners error paths and bin searches that left the table
    gam_pf: np.ndarray           # [2]: the Lorentz factor of each door's plasma frame
    mom_edge_cgs: np.ndarray     # [nmom+2]


def escape_gam_pf(prob) -> np.ndarray:
    """The flow the escaping particles leave behind: at the upstream free-escape boundary and far downstream."""
    P = prob.params
    return np.array([prob.gam_sf[P.i_grid_feb], prob.gam_sf[P.n_grid]], dtype=np.float64)


def escape_spectra(prob, backend, i_ion: int, gam_pf=None) -> EscapeSpectra:
    """The escape slabs of the backend's resident tallies through get_dNdp_cr's rebinning (the reference's print_dNdp_esc,
    src/ion_finalize.jl:65-68, which has no body there)."""
    if not hasattr(backend, "dndp_esc"):
        raise ValueError("escape_spectra: the backend has no dndp_esc (the escape spectra are made on the device, K10; there is no host twin)")
    tabs = consumer_tables(prob, i_ion)
    g = escape_gam_pf(prob) if gam_pf is None else np.ascontiguousarray(gam_pf, dtype=np.float64)
    dndp, number, diag = backend.dndp_esc(tabs, g)
    return EscapeSpectra(dndp, number, diag, g, tabs.mom_edge_cgs)


@dataclasses.dataclass
class AngleDistributions:
    """The pitch-angle distribution of every grid zone over momentum windows (K11, include/mcs.h mcs_angle_dist), per frame (0: shock,
    1: the zone's plasma frame, 2: ISM), zone (0-based) and window.  The windows select momentum bins OF THE TARGET FRAME."""
    dist: np.ndarray             # [3][n_grid][n_win][ntht+2]: (share of the window's weight in the angle bin) / (cos_edge[j+1] - cos_edge[j]); empty: 1e-99
    number: np.ndarray           # [3][n_grid][n_win]: the summed weight of the window
    mean_mu: np.ndarray          # [3][n_grid][n_win]: <mu> over cos_center; NaN where number is 0
    mean_mu2: np.ndarray         # [3][n_grid][n_win]: <mu^2>; NaN where number is 0
    windows: tuple               # ((l_lo, l_hi), ...): momentum bins l_lo <= k < l_hi
    cos_edge: np.ndarray         # [ntht+2]
    cos_center: np.ndarray       # [ntht+1]


def momentum_windows(prob, windows) -> tuple:
    """((l_lo, l_hi), ...) of `angle_distributions` from momenta [(p_lo, p_hi), ...] in cgs: the bins whose centre lies in
    [p_lo, p_hi], by the bin centres of ensemble.slope_window.  An empty window, or more than eight, raises ValueError."""
    from . import ensemble as ens
    x_log = ens.bin_centres_log10(prob)
    windows = list(windows)
    if not 1 <= len(windows) <= ens.ANGLE_MAX_WINDOWS:
        raise ValueError(f"momentum_windows: 1..{ens.ANGLE_MAX_WINDOWS} windows, not {len(windows)}")
    out = []
    for p_lo, p_hi in windows:
        if not 0 < p_lo < p_hi:
            raise ValueError(f"momentum_windows: a window needs momenta 0 < p_lo < p_hi, not {p_lo!r}, {p_hi!r}")
        inside = np.flatnonzero((x_log >= math.log10(p_lo)) & (x_log <= math.log10(p_hi)))
        if inside.size == 0:
            raise ValueError(f"momentum_windows: no momentum bin has its centre in [{p_lo!r}, {p_hi!r}]")
        out.append((int(inside[0]), int(inside[-1]) + 1))
    return tuple(out)


def angle_distributions(prob, backend, i_ion: int, windows, therm_from_hist: bool = True) -> AngleDistributions:
    """The pitch-angle distributions of the backend's resident tallies over the momentum-bin windows ((l_lo, l_hi), ...)
    (`momentum_windows` makes them from cgs momenta)."""
    if not hasattr(backend, "angle_dist"):
        raise ValueError("angle_distributions: the backend has no angle_dist (the distributions are made on the device, K11; there is no host twin)")
    from . import ensemble as ens
    windows = tuple((int(a), int(b)) for a, b in windows)
    lo, hi = ens.check_angle_windows(prob.params.num_psd_mom_bins, [w[0] for w in windows], [w[1] for w in windows])
    tabs = consumer_tables(prob, i_ion, therm_from_hist=therm_from_hist)
    dist, number, moments = backend.angle_dist(tabs, lo, hi)
    return AngleDistributions(dist, number, np.ascontiguousarray(moments[..., 0]), np.ascontiguousarray(moments[..., 1]), windows,
                              np.asarray(tabs.cos_edge), np.asarray(tabs.cos_center))


@dataclasses.dataclass
class TcutSpectra:
    """The spectra of the time cuts of one species in one iteration (K12, include/mcs.h mcs_tcut_spectra): of the weight still
    coupled to the shock at the cut's time, per cut k.  A cut that no particle reached is a DEAD row: spectrum all 1e-99, number 0.0,
    mean_log_p and the quantiles NaN."""
    spectrum: np.ndarray         # [nt][nmom+2]: the growth of spectra_coupled over the species, normalised to its sum; empty: 1e-99
    weight: np.ndarray           # [nt]: weight_coupled as it stands, floored as tcut_print floors it
    number: np.ndarray           # [nt]: the sum the spectrum was normalised with; 0.0 in a dead row
    mean_log_p: np.ndarray       # [nt]: the mean of log10 p (cgs) over the spectrum
    quantile: np.ndarray         # [3][nt]: log10 of the momentum below which the share TCUT_Q[j] of the weight lies
    index: np.ndarray            # [3]: d quantile / d log10 t over the live rows; NaN with fewer than three
    diag: np.ndarray             # [2]: live rows, words with now < base (must be 0)
    tcuts: np.ndarray            # [nt]: the times of the cuts
    mom_log_cgs: np.ndarray      # [nmom+2]: log10 of the momentum bin edges (cgs)

    def words(self) -> np.ndarray:
        """The result as one vector in mcs_tcut_layout, the tcuts sample of the ensemble statistics."""
        return np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in
                               (self.spectrum, self.weight, self.number, self.mean_log_p, self.quantile, self.index)])


TCUT_Q = capi.TCUT_Q


def _tcut_from_words(out, diag, nt, NM, tcuts, mom_log) -> TcutSpectra:
    o = np.asarray(out, dtype=np.float64)
    a = nt * NM
    return TcutSpectra(o[:a].reshape(nt, NM).copy(), o[a:a + nt].copy(), o[a + nt:a + 2 * nt].copy(), o[a + 2 * nt:a + 3 * nt].copy(),
                       o[a + 3 * nt:a + 6 * nt].reshape(3, nt).copy(), o[a + 6 * nt:a + 6 * nt + 3].copy(), np.asarray(diag, dtype=np.int64),
                       np.array(tcuts, dtype=np.float64), np.array(mom_log, dtype=np.float64))


def _growth_rows_host(now, base, e, nm: int):
    """The row rules that K12 and K14 share (include/mcs.h, mcs_tcut_spectra: GROWTH AND NUMBER, LIVE AND DEAD ROWS, the spectrum's
    normalisation and floor, MEAN, QUANTILES) for rows side by side: now, base [rows][nm+1], e [nm+2] ->
    (g, n_neg, num, live, spectrum [rows][nm+2], mean [rows], quant [3][rows]).  To be called under np.errstate(all="ignore")."""
    nt, NM = now.shape[0], nm + 2
    g = now - base
    n_neg = int(np.count_nonzero(now < base))
    num = np.zeros(nt)
    for l in range(nm + 1):
        num = num + g[:, l]
    live = num > 1.0e-99
    spectrum = np.full((nt, NM), 1.0e-99)
    s = g / np.where(live, num, 1.0)[:, None]
    spectrum[:, :nm + 1] = np.where(live[:, None], np.where(s < 1.0e-60, 1.0e-99, s), 1.0e-99)
    c = 0.5 * (e[:-1] + e[1:])
    sm = np.zeros(nt)
    for l in range(nm + 1):
        sm = sm + g[:, l] * c[l]
    mean = np.where(live, sm / num, np.nan)
    quant = np.full((3, nt), np.nan)
    for j, q in enumerate(TCUT_Q):
        T = q * num
        C = np.zeros(nt)
        found = np.zeros(nt, dtype=bool)
        last = np.full(nt, -1)
        val = np.full(nt, np.nan)
        for l in range(nm + 1):
            gl = g[:, l]
            Cn = C + gl
            lit = (gl > 0) & ~found
            hit = lit & (Cn >= T)
            f = (T - C) / np.where(hit, gl, 1.0)
            val = np.where(hit, e[l] + f * (e[l + 1] - e[l]), val)
            found = found | hit
            last = np.where(lit & ~hit, l, last)
            C = Cn
        short = ~found & (last >= 0)
        lz = np.where(short, last, 0)
        val = np.where(short, e[lz] + 1.0 * (e[lz + 1] - e[lz]), val)
        quant[j] = np.where(live, val, np.nan)
    return g, n_neg, num, live, spectrum, mean, quant


def tcut_spectra_host(now, base, weight, mom_log, tcuts, nmom: int, log10) -> TcutSpectra:
    """The rules of mcs_tcut_spectra (include/mcs.h) in numpy, the cuts side by side and the bins of a row one after the other, so
    that every sum is the serial one.  now, base: [>= nt][>= nmom+1] rows of spectra_coupled of the species and what they held at
    its start; weight: [>= nt] of weight_coupled; log10: the deterministic one (ensemble._det_log10)."""
    from . import ensemble as ens
    tcuts = np.asarray(tcuts, dtype=np.float64)
    nt, nm, NM = len(tcuts), int(nmom), int(nmom) + 2
    e = np.asarray(mom_log, dtype=np.float64)[:NM]
    now = np.asarray(now, dtype=np.float64)[:nt, :nm + 1]
    base = np.asarray(base, dtype=np.float64)[:nt, :nm + 1]
    with np.errstate(all="ignore"):
        g, n_neg, num, live, spectrum, mean, quant = _growth_rows_host(now, base, e, nm)
        w = np.asarray(weight, dtype=np.float64)[:nt]
        weight_out = np.where(w < 1.0e-60, 1.0e-99, w)
        x = log10(np.ascontiguousarray(tcuts))
        index = ens.slopes_xy(x, quant, np.broadcast_to(live, quant.shape))
    number = np.where(live, num, 0.0)
    return TcutSpectra(spectrum, weight_out, number, mean, quant, index, np.array([int(live.sum()), n_neg], dtype=np.int64),
                       tcuts.copy(), e.copy())


def tcut_spectra(prob, backend, i_ion: int, base=None) -> TcutSpectra:
    """The time-cut spectra of species i_ion from the backend's resident weight_coupled and spectra_coupled: on a HIP backend the
    device call (K12; the base is the one its begin_species took), on a backend without it the numpy statement of the same rules on
    the tallies read back and on `base`, the species' [100][201] block of spectra_coupled as it stood at the species' start."""
    P = prob.params
    if not P.do_tcuts or len(prob.tcuts) < 1:
        raise ValueError("tcut_spectra: the problem tracks no time cuts")
    tabs = consumer_tables(prob, i_ion)
    nt, NM = len(prob.tcuts), P.num_psd_mom_bins + 2
    if hasattr(backend, "tcut_spectra"):
        out, diag = backend.tcut_spectra(tabs)
        return _tcut_from_words(out, diag, nt, NM, prob.tcuts, tabs.mom_log_cgs)
    if base is None:
        raise ValueError("tcut_spectra: a backend without tcut_spectra needs the base, spectra_coupled of the species as it stood at its start")
    from . import ensemble as ens
    L = backend.layout
    f, _ = backend.read_tallies()
    return tcut_spectra_host(L.view(f, "spectra_coupled")[i_ion - 1], base, L.view(f, "weight_coupled")[i_ion - 1], tabs.mom_log_cgs,
                             prob.tcuts, P.num_psd_mom_bins, ens._det_log10(backend))


# ---- K14: the spectra at the detectors (include/mcs.h, mcs_detector_spectra) ------------------------------------------------------
@dataclasses.dataclass
class DetectorSpectra:
    """The spectra that the XSPEC detectors saw of one species in one iteration (K14, include/mcs.h mcs_detector_spectra), per frame
    f (0: shock frame, spectra_sf; 1: plasma frame, spectra_pf) and detector d.  A detector that no particle crossed is a DEAD row:
    spectrum and dndp all 1e-99, number 0.0, mean_log_p, the quantiles and slope NaN."""
    spectrum: np.ndarray         # [2][nd][nmom+2]: the growth of the detector's row over the species, normalised to its sum; empty: 1e-99
    dndp: np.ndarray             # [2][nd][nmom+2]: the growth per unit momentum (cgs); empty: 1e-99
    number: np.ndarray           # [2][nd]: the sum the spectrum was normalised with; 0.0 in a dead row
    mean_log_p: np.ndarray       # [2][nd]: the mean of log10 p (cgs) over the spectrum
    quantile: np.ndarray         # [3][2][nd]: log10 of the momentum below which the share TCUT_Q[j] of the weight lies
    slope: np.ndarray            # [2][nd]: d log10 dndp / d log10 p over the window; NaN with fewer than three lit bins
    gradient: np.ndarray         # [nmom+2]: d log10 g / d (x / x_unit) over the upstream detectors, shock frame; ln 10 times it is u0 / D(p)
    diag: np.ndarray             # [3]: live rows, words with now < base (must be 0), finite gradient words
    x_spec: np.ndarray           # [nd]: the detectors' positions (cm)
    window: tuple                # (l_lo, l_hi) of the slope
    x_unit: float                # what the gradient's x was divided by (rg0)
    mom_log_cgs: np.ndarray      # [nmom+2]: log10 of the momentum bin edges (cgs)

    def words(self) -> np.ndarray:
        """The result as one vector in mcs_detector_layout, the detectors sample of the ensemble statistics."""
        return np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in
                               (self.spectrum, self.dndp, self.number, self.mean_log_p, self.quantile, self.slope, self.gradient)])

    def settings(self) -> tuple:
        """What an ensemble keeps of its first detectors sample: nd, the window, the bits of x_unit and of x_spec."""
        return (len(self.x_spec), int(self.window[0]), int(self.window[1]), np.float64(self.x_unit).tobytes(),
                np.ascontiguousarray(self.x_spec, dtype=np.float64).tobytes())


def _detector_from_words(out, diag, nd, NM, x_spec, window, x_unit, mom_log) -> DetectorSpectra:
    o = np.asarray(out, dtype=np.float64)
    r, a = 2 * nd, 2 * nd * NM
    return DetectorSpectra(o[:a].reshape(2, nd, NM).copy(), o[a:2 * a].reshape(2, nd, NM).copy(), o[2 * a:2 * a + r].reshape(2, nd).copy(),
                           o[2 * a + r:2 * a + 2 * r].reshape(2, nd).copy(), o[2 * a + 2 * r:2 * a + 5 * r].reshape(3, 2, nd).copy(),
                           o[2 * a + 5 * r:2 * a + 6 * r].reshape(2, nd).copy(), o[2 * a + 6 * r:2 * a + 6 * r + NM].copy(),
                           np.asarray(diag, dtype=np.int64), np.array(x_spec, dtype=np.float64), (int(window[0]), int(window[1])), float(x_unit),
                           np.array(mom_log, dtype=np.float64))


def check_detector_window(nmom: int, window) -> tuple:
    """(l_lo, l_hi) of a slope window over the bins 0..nmom; None: all bins.  ValueError for what mcs_detector_spectra refuses."""
    l_lo, l_hi = (0, int(nmom) + 1) if window is None else (int(window[0]), int(window[1]))
    if l_lo < 0 or l_hi > nmom + 1 or l_hi - l_lo < 3:
        raise ValueError(f"detector_spectra: window [{l_lo}, {l_hi}) needs 0 <= l_lo, l_hi <= {nmom + 1} and at least three bins")
    return l_lo, l_hi


def detector_spectra_host(now, base, mom_log, mom_edge, x_spec, nmom: int, window, x_unit: float, log10) -> DetectorSpectra:
    """The rules of mcs_detector_spectra (include/mcs.h) in numpy, the rows side by side and the bins of a row one after the other,
    so that every sum is the serial one.  now, base: [2][>= nd][>= nmom+1], the rows of spectra_sf and spectra_pf and what they held
    at the species' start; log10: the deterministic one (ensemble._det_log10)."""
    from . import ensemble as ens
    x_spec = np.array(x_spec, dtype=np.float64)
    nd, nm, NM = len(x_spec), int(nmom), int(nmom) + 2
    if nd < 1:
        raise ValueError("detector_spectra: no detector is set")
    l_lo, l_hi = check_detector_window(nm, window)
    if not (np.isfinite(x_unit) and x_unit > 0):
        raise ValueError("detector_spectra: x_unit must be finite and positive")
    e = np.asarray(mom_log, dtype=np.float64)[:NM]
    E = np.asarray(mom_edge, dtype=np.float64)[:NM]
    if not np.all(E[1:] > E[:-1]):
        raise ValueError("detector_spectra: mom_edge_cgs is not strictly ascending")
    now = np.asarray(now, dtype=np.float64)[:, :nd, :nm + 1].reshape(2 * nd, nm + 1)
    base = np.asarray(base, dtype=np.float64)[:, :nd, :nm + 1].reshape(2 * nd, nm + 1)
    with np.errstate(all="ignore"):
        g, n_neg, num, live, spectrum, mean, quant = _growth_rows_host(now, base, e, nm)
        dE = E[1:] - E[:-1]
        dndp = np.full((2 * nd, NM), 1.0e-99)
        lit = live[:, None] & (g != 0.0)
        dndp[:, :nm + 1] = np.where(lit, g / dE[None, :], 1.0e-99)
        valid = g > 0
        y = np.zeros_like(g)
        y[valid] = log10(np.ascontiguousarray(dndp[:, :nm + 1][valid]))
        xc = 0.5 * (e[:-1] + e[1:])
        slope = ens.slopes_xy(xc[l_lo:l_hi], y[:, l_lo:l_hi], valid[:, l_lo:l_hi])
        slope = np.where(live, slope, np.nan)
        # the gradient: per momentum bin a slope over the detectors, shock frame
        g0 = g[:nd].T                                           # [nm+1][nd]
        vg = (g0 > 0) & (x_spec < 0.0)[None, :]
        yg = np.zeros_like(g0)
        yg[vg] = log10(np.ascontiguousarray(g0[vg]))
        gradient = np.full(NM, np.nan)
        gradient[:nm + 1] = ens.slopes_xy(x_spec / x_unit, yg, vg)
    number = np.where(live, num, 0.0)
    diag = np.array([int(live.sum()), n_neg, int(np.isfinite(gradient).sum())], dtype=np.int64)
    return DetectorSpectra(spectrum.reshape(2, nd, NM), dndp.reshape(2, nd, NM), number.reshape(2, nd), mean.reshape(2, nd),
                           quant.reshape(3, 2, nd), slope.reshape(2, nd), gradient, diag, x_spec, (l_lo, l_hi), float(x_unit), e.copy())


def detector_base(backend, nd: int) -> np.ndarray:
    """Rows 0..nd-1 of spectra_sf and spectra_pf as the backend holds them now, [2][nd][201]: the base that a backend without the
    device call needs of the species' start."""
    L = backend.layout
    f, _ = backend.read_tallies()
    return np.stack([L.view(f, "spectra_sf")[:nd], L.view(f, "spectra_pf")[:nd]]).copy()


def detector_spectra(prob, backend, i_ion: int, window=None, base=None) -> DetectorSpectra:
    """The detector spectra of species i_ion from the backend's resident spectra_sf and spectra_pf: on a HIP backend the device call
    (K14; the base is the one its begin_species took), on a backend without it the numpy statement of the same rules on the tallies
    read back and on `base` (detector_base at the species' start).  window: (l_lo, l_hi) of the slope, None: all bins.  The gradient's
    x is in units of rg0."""
    P = prob.params
    nd = len(prob.x_spec)
    if nd < 1:
        raise ValueError("detector_spectra: the problem has no detector (XSPEC)")
    tabs = consumer_tables(prob, i_ion)
    nm, NM = P.num_psd_mom_bins, P.num_psd_mom_bins + 2
    l_lo, l_hi = check_detector_window(nm, window)
    x_unit = float(prob.rg0)
    if hasattr(backend, "detector_spectra"):
        out, diag = backend.detector_spectra(tabs, l_lo, l_hi, x_unit)
        return _detector_from_words(out, diag, nd, NM, prob.x_spec, (l_lo, l_hi), x_unit, tabs.mom_log_cgs)
    if base is None:
        raise ValueError("detector_spectra: a backend without detector_spectra needs the base, detector_base at the species' start")
    from . import ensemble as ens
    return detector_spectra_host(detector_base(backend, nd), base, tabs.mom_log_cgs, tabs.mom_edge_cgs, prob.x_spec, nm, (l_lo, l_hi), x_unit,
                                 ens._det_log10(backend))


# ---- K13: the shock-profile update (include/mcs.h, mcs_profile_update) ----------------------------------------------------------
PROFILE_ROWS = ("flux_px", "flux_en", "gamma_ad", "p_flux", "p_used", "ux_px", "ux_en", "ux_pred", "ux_next", "shift")
PROFILE_SCALARS = ("gamma_down", "px_esc_up", "en_esc_up", "q_px", "q_en", "q_px_avg", "q_en_avg", "shift_rms")
PROFILE_SETTINGS = ("F_px_upstream", "F_energy_upstream", "P0", "rho0", "n0_aa", "r_comp", "r_RH", "u2", "beta2", "gam2", "SMMOE",
                    "SMPFP", "w", "i_trans")
PROFILE_MAX_HIST = 3
PROFILE_NEWTON_TOL = 1.0e-14
PROFILE_NEWTON_MAX = 10_000
BETA_REL_FL = 0.02          # src/parameters.jl:30 (iter_finalize.BETA_REL_FL)


@dataclasses.dataclass
class ProfileIn:
    """`mcs_profile_in`: what the host hands to the profile update; nothing in it depends on the iteration's tallies.  The first
    fourteen fields (PROFILE_SETTINGS) are the settings an ensemble keeps of its first profile sample."""
    F_px_upstream: float
    F_energy_upstream: float
    P0: float                    # kB sum(n0 T0): the species sum of q_esc_calcs
    rho0: float                  # sum(n0 m)
    n0_aa: float                 # sum(n0 aa)
    r_comp: float
    r_RH: float
    u2: float
    beta2: float
    gam2: float
    SMMOE: float
    SMPFP: float
    w: float                     # the old-profile weight AFTER the increase_old_profile_weighting rule
    i_trans: int                 # first zone of the artificial arctangent section (Julia zone number); 0: none
    hist_q_px: tuple = ()        # the q of up to three earlier iterations, oldest first
    hist_q_en: tuple = ()
    pxx_EM: np.ndarray = None    # [n_grid]: the electromagnetic momentum flux of the current profile and field
    en_EM: np.ndarray = None     # [n_grid]
    atan_x: np.ndarray = None    # [n_grid]: atan(x_grid_rg) of zones 1..n_grid

    def settings(self) -> np.ndarray:
        return np.array([float(getattr(self, k)) for k in PROFILE_SETTINGS], dtype=np.float64)

    def as_struct(self) -> "capi.McsProfileIn":
        self._keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (self.pxx_EM, self.en_EM, self.atan_x)]
        s = capi.McsProfileIn()
        for k in PROFILE_SETTINGS[:-1]:
            setattr(s, k, float(getattr(self, k)))
        s.i_trans = int(self.i_trans)
        s.n_hist = len(self.hist_q_px)
        for k in range(min(len(self.hist_q_px), PROFILE_MAX_HIST)):
            s.hist_q_px[k] = float(self.hist_q_px[k]); s.hist_q_en[k] = float(self.hist_q_en[k])
        dp = ct.POINTER(ct.c_double)
        s.pxx_EM, s.en_EM, s.atan_x = (a.ctypes.data_as(dp) for a in self._keep)
        return s


@dataclasses.dataclass
class ProfileUpdate:
    """The profile that smooth_grid_par WOULD write from one iteration's fluxes and pressures (K13, include/mcs.h
    mcs_profile_update), with the intermediate rows.  Rows are zones 1..n_grid."""
    rows: np.ndarray             # [10][n_grid], PROFILE_ROWS
    scalars: np.ndarray          # [8], PROFILE_SCALARS
    diag: np.ndarray             # [3]: non-finite output words, zones whose Newton ran out of steps, the largest Newton step count
    settings: np.ndarray         # ProfileIn.settings() of the call

    def __getattr__(self, name):
        if name in PROFILE_ROWS:
            return self.rows[PROFILE_ROWS.index(name)]
        if name in PROFILE_SCALARS:
            return float(self.scalars[PROFILE_SCALARS.index(name)])
        raise AttributeError(name)

    def words(self) -> np.ndarray:
        """The result as one vector in mcs_profile_layout, the profile sample of the ensemble statistics."""
        return np.concatenate([np.asarray(self.rows, dtype=np.float64).ravel(), np.asarray(self.scalars, dtype=np.float64)])


def _profile_from_words(out, diag, n, settings) -> ProfileUpdate:
    o = np.asarray(out, dtype=np.float64)
    return ProfileUpdate(o[:10 * n].reshape(10, n).copy(), o[10 * n:10 * n + 8].copy(), np.asarray(diag, dtype=np.int64).copy(),
                         np.asarray(settings, dtype=np.float64))


def _profile_smooth(y):
    """`smooth_profile!` on a numpy row: the descending `<` pass, then the 1-2-1 / three-point filter."""
    n = len(y)
    for i in range(n - 1, 0, -1):
        if y[i - 1] < y[i]:
            y[i - 1] = y[i]
    d = y.copy()
    d[1] = (2 * y[0] + y[1] + y[2]) / 4
    for i in range(2, n - 2):
        d[i] = (y[i - 1] + y[i] + y[i + 1]) / 3
    d[n - 2] = (y[n - 3] + y[n - 2] + 2 * y[n - 1]) / 4
    y[1:n - 1] = d[1:n - 1]


def _profile_newton(f_df, x0):
    x, steps = np.float64(x0), 0
    for _ in range(PROFILE_NEWTON_MAX):
        f, df = f_df(x)
        dx = f / df
        x = x - dx
        steps += 1
        if abs(dx) <= PROFILE_NEWTON_TOL * abs(x):
            return x, steps, False
    return x, steps, True


def profile_update_host(pin: ProfileIn, params, ux_tab, gam_sf_tab, x_grid_cm, pxx_flux, energy_flux, scalars, P_par, P_perp,
                        e_dens) -> ProfileUpdate:
    """The rules of mcs_profile_update (include/mcs.h) in numpy: the elementwise lines side by side over the zones, the ordered
    ones zone after zone; powers are products.  params: u0, beta0, gam0, n_grid, i_shock; the three tables have n_grid + 2 entries,
    the tallies and pressures n_grid."""
    f8 = np.float64
    n, i_shock = int(params.n_grid), int(params.i_shock)
    if n < 3:
        raise ValueError("profile_update: a profile has at least three zones")
    if not 0 <= int(pin.i_trans) <= i_shock:
        raise ValueError(f"profile_update: i_trans {pin.i_trans} outside 0..i_shock ({i_shock})")
    if len(pin.hist_q_px) > PROFILE_MAX_HIST or len(pin.hist_q_px) != len(pin.hist_q_en):
        raise ValueError(f"profile_update: at most {PROFILE_MAX_HIST} earlier (q_px, q_en) pairs")
    u0, b0, g0 = f8(params.u0), f8(params.beta0), f8(params.gam0)
    c, mp = f8(C), f8(MP)
    F_px, F_en, P0, rho0, n0 = f8(pin.F_px_upstream), f8(pin.F_energy_upstream), f8(pin.P0), f8(pin.rho0), f8(pin.n0_aa)
    u2, b2, g2 = f8(pin.u2), f8(pin.beta2), f8(pin.gam2)
    rel = bool(b0 >= BETA_REL_FL)
    arr = lambda a: np.array(a, dtype=np.float64)[:n].copy()
    sc = np.asarray(scalars, dtype=np.float64)
    ux, g = np.asarray(ux_tab, dtype=np.float64)[1:n + 1], np.asarray(gam_sf_tab, dtype=np.float64)[1:n + 1]
    down = np.asarray(x_grid_cm, dtype=np.float64)[1:n + 1] >= 0
    Ppar, Pperp, ed = arr(P_par), arr(P_perp), arr(e_dens)
    pxx_EM, en_EM, atan_x = arr(pin.pxx_EM), arr(pin.en_EM), arr(pin.atan_x)
    with np.errstate(all="ignore"):
        px_esc, en_esc = sc[2] / F_px, sc[3] / F_en
        gam_down = 1 + sc[0] / sc[1]
        # q_esc_calcs
        if f8(pin.r_comp) == f8(pin.r_RH):
            q_px, q_en = f8(0.0), f8(0.0)
        else:
            Gf = gam_down / (gam_down - 1)
            rho2 = ((rho0 * g0) * b0) / (g2 * b2)
            if rel:
                q_fac = c * np.sqrt((1 + b0) / 2)
                e = rho0 * (c * c) + 2.5 * P0
                Fp = ((g0 * g0) * (b0 * b0)) * e + P0
                Fe = ((g0 * g0) * u0) * e
                aux = (g2 * g2) * (q_fac * (b2 * b2) - u2)
                P2 = ((q_fac * Fp - Fe) - (aux * rho2) * (c * c)) / (q_fac + Gf * aux)
                t = g2 * b2
                Q_px = (Fp - (t * t) * (rho2 * (c * c) + Gf * P2)) - P2
                Q_en = Q_px * q_fac
                q_px, q_en = Q_en / (Fe - ((g0 * u0) * rho0) * (c * c)), Q_px / Fp
            else:
                Fp = rho0 * (u0 * u0) + P0
                Fe = (rho0 * ((u0 * u0) * u0)) / 2 + (2.5 * P0) * u0
                P2 = Fp - rho2 * (u2 * u2)
                Q_en = (Fe - ((rho0 * u0) * (u2 * u2)) / 2) - (P2 * u2) * Gf
                q_px, q_en = Q_en / Fe, f8(0.0)
        k = len(pin.hist_q_px) + 1
        s_px, s_en = None, None
        for a, b in list(zip(pin.hist_q_px, pin.hist_q_en)) + [(q_px, q_en)]:
            s_px = f8(a) if s_px is None else s_px + f8(a)
            s_en = f8(b) if s_en is None else s_en + f8(b)
        q_px_avg, q_en_avg = s_px / k, s_en / k
        pxx = np.rint(arr(pxx_flux) * 1.0e13) / 1.0e13
        en = np.rint(arr(energy_flux) * 1.0e13) / 1.0e13
        G = 1 + (Ppar + Pperp) / ed
        G[ed == 1.0e-99] = 1.0e-99
        Xi = G / (G - 1)
        Ptot = Ppar + Pperp
        wp = f8(pin.SMPFP)
        Qpx = q_px_avg * pxx[0] if rel else f8(0.0)
        Qen = q_en_avg * en[0]
        bux = ux / c
        steps_max, n_out = 0, 0
        if rel:
            gb = g * bux
            gb2 = gb * gb
            dens = ((g0 * b0) / (g * bux)) * n0
            p_px = (pxx - ((gb2 * dens) * mp) * (c * c)) / (1 + gb2 * Xi)
            p_loc = (1 - wp) * p_px + wp * Ptot
            gbn = (((F_px - Qpx) - pxx_EM) - p_loc) / (((g0 * b0) * n0) * (mp * (c * c) + (p_loc * Xi) / dens))
            ux_px = (gbn / np.sqrt(1 + gbn * gbn)) * c
            K = ((F_en - Qen) - en_EM) / (c * ((dens * mp) * (c * c) + Xi * p_loc))
            y = (-1 + np.sqrt(1 + (4 * K) * K)) / 2
            gbn = np.copysign(np.sqrt(y), K)
            ux_en = (gbn / np.sqrt(1 + gbn * gbn)) * c
        else:
            rm = n0 * mp
            b2x = bux * bux
            p_px = (pxx - ((rm * u0) * ux) * (1 + b2x)) / (1 + b2x * Xi)
            p_loc = (1 - wp) * p_px + wp * Ptot
            ux_px, ux_en = np.zeros(n), np.zeros(n)
            for j in range(n):
                X, pl = Xi[j], p_loc[j]
                A = (F_px - Qpx) - pxx_EM[j]
                B = (F_en - Qen) - en_EM[j]

                def f_px(b):
                    return ((A - ((rm * u0) * (b * c)) * (1 + b * b)) - (1 + (b * b) * X) * pl,
                            -(((rm * u0) * c) * (1 + (3 * b) * b) + ((2 * b) * X) * pl))

                def f_en(u):
                    t = u / c
                    t2 = t * t
                    return ((B - ((((0.5 * rm) * u0) * u) * u) * (1 + 1.25 * t2)) - ((X * pl) * u) * (1 + t2),
                            -(((rm * u0) * u) * (1 + 2.5 * t2) + (X * pl) * (1 + 3 * t2)))
                x, s1, o1 = _profile_newton(f_px, (u0 / c) * 1.0e-4)
                ux_px[j] = x * c
                ux_en[j], s2, o2 = _profile_newton(f_en, u0 * 1.0e-4)
                steps_max = max(steps_max, s1, s2)
                n_out += int(o1 or o2)
        avg_px, avg_en = f8(0.0), f8(0.0)
        for j in range(max(0, n - 10), n):
            avg_px = avg_px + ux_px[j]; avg_en = avg_en + ux_en[j]
        avg_px, avg_en = avg_px / 10, avg_en / 10
        if rel:
            _profile_smooth(ux_px); _profile_smooth(ux_en)
        for a, avg in ((ux_px, avg_px), (ux_en, avg_en)):
            s = (u0 - u2) / (a[0] - avg)
            a[:] = s * (a - avg) + u2
            a[down] = u2
        if not rel:
            _profile_smooth(ux_px); _profile_smooth(ux_en)
        mo = f8(pin.SMMOE)
        ux_pred = (1 - mo) * ux_px + mo * ux_en
        ux_new = ux_pred.copy()
        it = int(pin.i_trans)
        if it > 0:
            last = ux_pred[n - 1]
            s = -(ux_pred[it - 1] - last) / atan_x[it - 1]
            ux_new[it - 1:i_shock] = (-atan_x[it - 1:i_shock]) * s + last
        w = f8(pin.w)
        ux_next = (ux_new + w * ux) / (1 + w)
        shift = (ux_pred - ux) / u0
        s = f8(0.0)
        for j in range(n):
            s = s + shift[j] * shift[j]
        rms = np.sqrt(s / n)
        px_esc = f8(1.0e-99) if 1.0e-99 > px_esc else px_esc
        en_esc = f8(1.0e-99) if 1.0e-99 > en_esc else en_esc
    rows = np.stack([pxx / F_px, en / F_en, G, p_px, p_loc, ux_px, ux_en, ux_pred, ux_next, shift])
    svec = np.array([gam_down, px_esc, en_esc, q_px, q_en, q_px_avg, q_en_avg, rms], dtype=np.float64)
    bad = int(np.count_nonzero(~np.isfinite(rows))) + int(np.count_nonzero(~np.isfinite(svec)))
    return ProfileUpdate(rows, svec, np.array([bad, n_out, steps_max], dtype=np.int64), pin.settings())


def profile_in(prob, it_state, sm, i_iter: int, history=None) -> ProfileIn:
    """The `mcs_profile_in` of iteration i_iter from the quantities iter_finalize uses: the upstream fluxes of `it_state`, the
    species sums, the weight after the increase_old_profile_weighting rule, the start of the artificial section, the
    electromagnetic fluxes of the current profile.  history: [(q_px, q_en)] of earlier iterations, oldest first (the last three
    count); None: none, the samples of a fixed profile stay independent."""
    P, cfg = prob.params, prob.cfg
    n = P.n_grid
    n0 = np.array([s.density for s in cfg.species]); T0 = np.array([s.temperature for s in cfg.species])
    m = np.array([s.mass for s in cfg.species])
    w = sm.old_profile_weight
    if sm.increase_old_profile_weighting and i_iter != 1:
        w = max(10.0, w * (1.15 if i_iter < 6 else 1.5))
    xs = sm.artificial_smoothing_start_rg
    i_trans = 0
    if xs < 0:
        i_trans = int(np.argmax(prob.x_grid_rg > xs)) - 1
        if not 1 <= i_trans <= P.i_shock:
            raise ValueError(f"profile_update: the artificial section would start at zone {i_trans}, outside 1..i_shock")
    ux = np.asarray(prob.ux, dtype=np.float64)[1:n + 1]; g = np.asarray(prob.gam_sf, dtype=np.float64)[1:n + 1]
    B = np.asarray(prob.btot, dtype=np.float64)[1:n + 1]; th = np.asarray(prob.theta, dtype=np.float64)[1:n + 1]
    bux = ux / C
    gb, g2_ = g * bux, g * g
    Bx, Bz = B * np.cos(th), B * np.sin(th)
    pxx_EM = gb ** 2 / (8 * math.pi) * B ** 2 + g2_ / (8 * math.pi) * (Bz ** 2 - Bx ** 2)
    en_EM = g2_ / (4 * math.pi) * bux * Bz ** 2
    hist = list(history or [])[-PROFILE_MAX_HIST:]
    return ProfileIn(it_state.F_px_upstream, it_state.F_energy_upstream, float(np.dot(n0, T0)) * KB, float(np.dot(n0, m)),
                     float(sum(s.density * s.aa for s in cfg.species)), prob.r_comp, it_state.r_RH, P.u2, prob.beta2, prob.gam2,
                     sm.SMMOE, sm.SMPFP, w, i_trans, tuple(h[0] for h in hist), tuple(h[1] for h in hist), pxx_EM, en_EM,
                     np.arctan(np.asarray(prob.x_grid_rg, dtype=np.float64)[1:n + 1]))


def profile_update(prob, backend, it_state, sm, i_iter: int, history=None, pressures=None) -> ProfileUpdate:
    """The profile update of iteration i_iter from the backend's resident fluxes and running scalars and the pressures of the last
    ion_finalize: on a HIP backend the device call (K13; the pressures are those mcs_thermo_calcs left on the device, or
    `pressures` = (P_par, P_perp, energy_density) in their place), on a backend without it the numpy statement of the same rules
    on the tallies read back, with `pressures` or, without them, those of a thermo_calcs of the last species.  Nothing of `prob`,
    `it_state` or the tallies is changed."""
    pin = profile_in(prob, it_state, sm, i_iter, history)
    n = prob.params.n_grid
    if hasattr(backend, "profile_update"):
        out, diag = backend.profile_update(pin, pressures)
        return _profile_from_words(out, diag, n, pin.settings())
    if pressures is None:
        pressures = backend.thermo_calcs(consumer_tables(prob, len(prob.cfg.species)))
    L = backend.layout
    f, _ = backend.read_tallies()
    return profile_update_host(pin, prob.params, prob.ux, prob.gam_sf, prob.x_grid_cm, L.view(f, "pxx_flux"), L.view(f, "energy_flux"),
                               L.view(f, "scalars"), *pressures)


# ---- photon post-processing -------------------------------------------------------------------------
# photon_calcs.jl:11-19: the common energy grid of the emission spectra
PHOTON_E_MIN_MEV = 1.0e-13
PHOTON_BINS_PER_DEC = 10
PHOTON_SYNCH_E_MAX_MEV = 1.0e5
MEV_ERG = 1.602176634e-6
KPC_CM = 3.0856775814913674e21


@dataclasses.dataclass
class PhotonSynch:
    """What `photon_synch` computes per grid zone (src/photon_synch.jl:28-133) -- it writes it to photon_synch_grid.dat."""
    energy_MeV: np.ndarray         # [n_photon]
    emis_erg_s: np.ndarray         # [n_grid][n_photon]  dP/d(ln E) emitted by the zone
    energy_flux_MeV: np.ndarray    # [n_grid][n_photon]  MeV / (cm^2 s) per d(ln E) at Earth, floor 1e-99
    photon_flux: np.ndarray        # [n_grid][n_photon]  photons / (cm^2 s) per d(ln E) at Earth, floor 1e-99


def photon_synch(prob, backend, ion_fin: IonFinal, i_ion: int, jet_dist_kpc: float = 1.0e6, redshift: float = 0.0) -> PhotonSynch:
    """The synchrotron branch of `photon_calcs` (src/photon_calcs.jl:27-113) for an electron species: per zone, the fold of
    src/synch_emission.jl over the plasma-frame dN/dp (frame 2 of get_dNdp_cr; the thermal part is empty, quirk C4), on the
    device (K5), then photon_synch's conversion to fluxes at Earth (src/photon_synch.jl:74-108) with the luminosity distance
    of photon_calcs.jl:40.  The photon stack is dead code in the reference: followed as
    specification.  Inverse Compton: `photon_ic` below; pion decay (nuclei): `photon_pion`; the sum of the three: `summed_emission`."""
    P = prob.params
    sp = prob.cfg.species[i_ion - 1]
    if sp.aa >= 1:
        raise ValueError("photon_synch: synchrotron emission is computed for the electron species (aa < 1)")
    tabs = consumer_tables(prob, i_ion)
    n_photon = int(math.log10(PHOTON_SYNCH_E_MAX_MEV / PHOTON_E_MIN_MEV) * PHOTON_BINS_PER_DEC)      # photon_calcs.jl:51
    E_erg, emis = backend.photon_synch(ion_fin.dNdp_cr[1], tabs.mom_edge_cgs, tabs.mc, n_photon, PHOTON_E_MIN_MEV, PHOTON_BINS_PER_DEC)
    dist_lum = jet_dist_kpc * (1 + redshift) * KPC_CM
    E_MeV = E_erg / MEV_ERG
    flux_erg = np.maximum(emis / (4 * math.pi * dist_lum ** 2), 1.0e-99)
    eflux_MeV = np.where(flux_erg > 1.0e-99, flux_erg / MEV_ERG, 1.0e-99)
    pflux = np.where(eflux_MeV <= 1.0e-99, 1.0e-99, eflux_MeV / E_MeV[None, :])
    return PhotonSynch(E_MeV, emis, eflux_MeV, pflux)


# ---- inverse Compton (src/photon_calcs.jl:116-138 -> src/inverse_compton.jl) ---------------------------------------------------
PHOTON_IC_E_MIN_MEV = 1.0e-2          # photon_calcs.jl:18
PHOTON_E_MAX_MEV = 1.0e12             # photon_calcs.jl:11
T_CMB0_K = 2.725                      # constants.jl:12
WIEN_B_NU = 5.879e10                  # Hz / K (inverse_compton.jl:167)
H_PLANCK = 6.62607015e-27             # erg s
ME = 9.1093837015e-28                 # g


def photon_field_cmb(redshift: float = 0.0):
    """`photon_field!` (src/inverse_compton.jl:313-383): the CMB at the source's redshift as 60 logarithmic frequency bins between
    nu_peak / 30 and 20 nu_peak -> (photon energy / m_e c^2, photons per cm^3) per bin."""
    T = T_CMB0_K * (1 + redshift)
    nu_peak = WIEN_B_NU * T
    n_nu = 60
    log_nu_min = math.log10(nu_peak / 30)
    dlog = (math.log10(nu_peak * 20) - log_nu_min) / n_nu
    con_f1 = 8 * math.pi * H_PLANCK / C ** 3
    con_f2 = H_PLANCK / (KB * T)
    alpha, dens = np.zeros(n_nu), np.zeros(n_nu)
    for j in range(1, n_nu + 1):
        log_nu1 = log_nu_min + (j - 1) * dlog
        nu1, nu2 = 10.0 ** log_nu1, 10.0 ** (log_nu1 + dlog)
        nu_avg = math.sqrt(nu1 * nu2)
        exp_fac = math.exp(min(con_f2 * nu_avg, 200.0))
        u = (nu2 - nu1) * con_f1 * nu_avg ** 3 / (exp_fac - 1)
        e = H_PLANCK * nu_avg
        alpha[j - 1] = e / (ME * C * C)
        dens[j - 1] = u / e
    return alpha, dens


def ic_cone_last_bin(cos_edge: np.ndarray, jet_sph_frac: float, num_psd_tht_bins: int) -> int:
    """`findfirst(>(2 jet_sph_frac - 1), cos_bounds)` (src/inverse_compton.jl:215): the last angle bin whose electrons can send
    photons to Earth; every bin when nothing exceeds the bound (a full sphere) or the hit lies past the last bin (mcs_ic.h, I2)."""
    hit = np.nonzero(cos_edge > 2 * jet_sph_frac - 1)[0]
    j = int(hit[0]) if len(hit) else num_psd_tht_bins
    return min(j, num_psd_tht_bins)


@dataclasses.dataclass
class PhotonIC:
    """What `photon_IC` computes per grid zone (src/inverse_compton.jl:36-188) -- it writes it to photon_IC_grid.dat."""
    energy_MeV: np.ndarray         # [n_photon]
    emis_erg: np.ndarray           # [n_grid][n_photon]  energy flux per d(ln E) at Earth, erg / (cm^2 s), floor 1e-99
    energy_flux_MeV: np.ndarray    # [n_grid][n_photon]  the same in MeV / (cm^2 s), floor 1e-99
    photon_flux: np.ndarray        # [n_grid][n_photon]  photons / (cm^2 s) per d(ln E), floor 1e-99
    ic_photon_sum: np.ndarray      # [n_grid][n_photon]  1e-99 + emis / E (the array get_summed_emission reads, :100-104)
    d2N_ef: object = None          # [n_grid][ntht+2][nmom+2] get_dNdp_2D's array, if it was downloaded


def photon_ic(prob, backend, i_ion: int, jet_dist_kpc: float = 1.0e6, redshift: float = 0.0, jet_sph_frac=None,
              download_d2n: bool = False, therm_from_hist: bool = True) -> PhotonIC:
    """The inverse-Compton branch of `photon_calcs` (src/photon_calcs.jl:116-138) for the electron species: `get_dNdp_2D`
    (src/particle_counter.jl:343-627 as called at src/ion_finalize.jl:50-59: the electrons' d2N/dp dcos in the ISM frame) and
    `photon_IC` -> `IC_emission_FCJ` on the CMB of `photon_field!` (src/inverse_compton.jl), both on the device (K6) on the
    histograms K1 left there; then photon_IC's conversions (:93-133).  Dead code in the reference, followed as specification
    (include/mcs_ic.h: I1-I3)."""
    P = prob.params
    sp = prob.cfg.species[i_ion - 1]
    if sp.aa >= 1:
        raise ValueError("photon_ic: inverse-Compton emission is computed for the electron species (aa < 1)")
    if jet_sph_frac is None:
        jet_sph_frac = jet_sphere_fraction(prob.cfg)
    if not 0 < jet_sph_frac <= 1:
        raise ValueError("photon_ic: the jet must cover a fraction 0 < f <= 1 of the sphere (JETFR)")
    tabs = consumer_tables(prob, i_ion, therm_from_hist)
    if _takes_download(backend):
        d2n = backend.dndp_2d(tabs, P.gam0, P.beta0, download=download_d2n)
    else:
        d2n = backend.dndp_2d(tabs, P.gam0, P.beta0)
    n_photon = int(math.log10(PHOTON_E_MAX_MEV / PHOTON_IC_E_MIN_MEV) * PHOTON_BINS_PER_DEC)          # photon_calcs.jl:50
    alpha_in, n_in = photon_field_cmb(redshift)
    j_max = ic_cone_last_bin(tabs.cos_edge, jet_sph_frac, P.num_psd_tht_bins)
    dist_lum = jet_dist_kpc * (1 + redshift) * KPC_CM
    beam_area = 4 * math.pi * dist_lum ** 2 * jet_sph_frac
    E_erg, emis = backend.photon_ic(tabs.mom_edge_cgs, tabs.mc, j_max, alpha_in, n_in, n_photon, PHOTON_IC_E_MIN_MEV, PHOTON_BINS_PER_DEC, beam_area)
    E_MeV = E_erg / MEV_ERG
    eflux_MeV = np.where(emis > 1.0e-99, emis / MEV_ERG, 1.0e-99)
    pflux = np.where(eflux_MeV <= 1.0e-99, 1.0e-99, eflux_MeV / E_MeV[None, :])
    ic_sum = 1.0e-99 + np.where(emis > 1.0e-99, emis / E_erg[None, :], 0.0)
    return PhotonIC(E_MeV, emis, eflux_MeV, pflux, ic_sum, d2n)


# ---- pion decay (src/photon_calcs.jl:66-88 -> src/photon_pion_decay.jl -> src/pion_kafexhiu.jl) ------------------------------------
PHOTON_PION_E_MIN_MEV = 1.0           # photon_calcs.jl:15


@dataclasses.dataclass
class PhotonPion:
    """What `photon_pion_decay` computes per grid zone (src/photon_pion_decay.jl:40-183) -- it writes it to photon_pion_decay_grid.dat."""
    energy_MeV: np.ndarray         # [n_photon]
    emis_erg_s: np.ndarray         # [n_grid][n_photon]  dP/d(ln E) emitted by the zone (pion_kafexhiu), floor 1e-99
    energy_flux: np.ndarray        # [n_grid][n_photon]  emis / (4 pi d_lum^2): erg / (cm^2 s) per d(ln E) at Earth, floor 1e-99
    photon_flux: np.ndarray        # [n_grid][n_photon]  energy_flux / E, floor 1e-99
    pion_photon_sum: np.ndarray    # [n_grid][n_photon]  this species' term of the array get_summed_emission reads (:118-125)
    n_pion_specs: int              # nuclei species of the run (:69)
    energy_erg: object = None      # [n_photon]  the energies as the fold returned them (the photon flux is divided by these)


def pion_scaling_factor(cfg, aa: float) -> float:
    """Baring et al. (1999) eq. 26 summed over the target nuclei (src/pion_kafexhiu.jl:60-65)."""
    n1 = cfg.species[0].density
    return float(sum((aa ** 0.375 + sp.aa ** 0.375 - 1) ** 2 * sp.density / n1 for sp in cfg.species if sp.aa >= 1))


def photon_pion(prob, backend, ion_fin: IonFinal, i_ion: int, jet_dist_kpc: float = 1.0e6, redshift: float = 0.0, i_data: int = 1) -> PhotonPion:
    """The pion-decay branch of `photon_calcs` (src/photon_calcs.jl:66-88) for a nucleus species: per zone, the fold of
    src/pion_kafexhiu.jl (Kafexhiu et al. 2014) over the plasma-frame dN/dp (frame 2 of get_dNdp_cr; the thermal histogram is empty,
    quirk C4) against the zone's thermal protons at rest, on the device (K7), then photon_pion_decay's conversion to fluxes at Earth
    (src/photon_pion_decay.jl:112-125).  Dead code in the reference, followed as specification (include/mcs_pion.h: P1-P3)."""
    P, cfg = prob.params, prob.cfg
    sp = cfg.species[i_ion - 1]
    if sp.aa < 1:
        raise ValueError("photon_pion: pion-decay emission is computed for nuclei (aa >= 1)")
    tabs = consumer_tables(prob, i_ion)
    n = P.n_grid
    with np.errstate(divide="ignore", invalid="ignore"):
        target = cfg.species[0].density * (P.gam0 * P.beta0) / np.sqrt(np.asarray(prob.gam_sf)[1:n + 1] ** 2 - 1)      # :62-63
    n_photon = int(math.log10(PHOTON_E_MAX_MEV / PHOTON_PION_E_MIN_MEV) * PHOTON_BINS_PER_DEC)                   # photon_calcs.jl:49
    E_erg, emis = backend.photon_pion(ion_fin.dNdp_cr[1], tabs.mom_edge_cgs, tabs.mc, sp.aa, np.ascontiguousarray(target),
                                      pion_scaling_factor(cfg, sp.aa), n_photon, PHOTON_PION_E_MIN_MEV, PHOTON_BINS_PER_DEC, i_data)
    dist_lum = jet_dist_kpc * (1 + redshift) * KPC_CM
    eflux = emis / (4 * math.pi * dist_lum ** 2)
    lit = eflux >= 1.0e-99
    eflux = np.where(lit, eflux, 1.0e-99)
    psum = np.where(lit, eflux / E_erg[None, :], 0.0)
    pflux = np.where(eflux <= 1.0e-99, 1.0e-99, eflux / E_erg[None, :])
    return PhotonPion(E_erg / MEV_ERG, emis, eflux, pflux, psum, sum(1 for s in cfg.species if s.aa >= 1), E_erg)


# ---- get_summed_emission (src/get_summed_emission.jl:37-413): the arithmetic of it ------------------------------------------------------
# The function is 834 lines of which 700 read the photon_*_grid.dat files back in and write histograms; its calculation is restated here
# on the arrays the three emission routines above return: the plasma-frame spectra (pion decay, synchrotron) are Doppler-shifted into the
# ISM frame, the zones are summed into the photon shells, and the three processes are laid onto one energy grid.  Dead code like the rest
# of the photon stack, followed as specification; where it cannot run as written:
#   S1  `log_energy_MeV_in` is overwritten with the LINEAR energies (:136, :141) and "dlogE" is then taken as the difference of two of them
#       (:150): the logarithmic bin width 1 / bins_per_decade is used, as :258 does;
#   S2  the three factors of the Lorentz factor (:188-198) are applied after the loop over the zones with the LAST zone's value: every zone
#       gets its own;
#   S3  `findnext` returns nothing for a photon shifted beyond the energy grid (:178-179): dropped;
#   S4  `sum_synch_IC_spectra()` is not defined: synchrotron and inverse-Compton bins are ADDED to the total at their offsets, as the pion
#       decay ones are assigned (:277);
#   S6  a shell's sum over its zones adds their 1e-99 floors (:792: log10 then gives -97.5 for a shell of three dark zones): floors are not summed;
#   S5  only the Doppler-shifted spectra are converted from photons per d(log E) to photons per bin (:166-170) while all three are divided by
#       the bin width at the end (:281-312): the inverse-Compton spectrum is converted too.
N_COS_BINS_DOPPLER = 180              # get_summed_emission.jl:117


def photon_shells(prob, num_upstream_shells: int, num_downstream_shells: int):
    """`set_photon_shells` (src/initializers.jl:305-398): shell boundaries between the shock and the free-escape boundaries, equal in
    log10|x / rg0| from 0.1 rg0 outwards; and the grid zone each boundary falls in (src/MonteCarloScattering.jl:392-401).
    -> (x_shell_endpoints_cm [n+1], n_shell_endpoints [n+1], 1-based zone numbers, 0 where no zone holds the boundary)."""
    P, rg0 = prob.params, prob.rg0
    nu, nd = int(num_upstream_shells), int(num_downstream_shells)
    if nu < 1 or nd < 1:
        raise ValueError("photon_shells: at least one shell on either side of the shock")
    ends = np.zeros(nu + nd + 1)
    w = (math.log10(abs(P.feb_upstream / rg0)) + 1) / nu
    for i in range(1, nu + 1):
        start = 0.0 if i == 1 else 10.0 ** (-1 + w * (i - 1))
        n = nu + 1 - i
        ends[n - 1] = -(10.0 ** (-1 + w * i)); ends[n] = -start
    use_prp = not P.feb_downstream > 0
    limit = P.x_grid_stop / rg0 if use_prp else P.feb_downstream / rg0
    w = (math.log10(limit) + 1) / nd
    for i in range(1, nd + 1):
        ends[nu + i - 1] = 0.0 if i == 1 else 10.0 ** (-1 + w * (i - 1))
        ends[nu + i] = 10.0 ** (-1 + w * i)
    ends *= rg0
    x = np.asarray(prob.x_grid_cm)
    zones = np.zeros(nu + nd + 1, dtype=np.int64)
    k = 0
    for i in range(1, P.n_grid + 1):
        if k <= nu + nd and x[i] <= ends[k] and x[i + 1] > ends[k]:
            zones[k] = i
            k += 1
    return ends, zones


def doppler_to_ism(flux, energy_MeV, gam_ef, beta_ef, bins_per_dec=PHOTON_BINS_PER_DEC):
    """get_summed_emission.jl:103-200 for one emission process: photons per d(log10 E) emitted isotropically in the plasma frame of every zone,
    re-binned by the Doppler-shifted energy of the central ray of 180 slices in cos(theta) (boundary 0 points upstream, towards the observer:
    E' = E gamma sqrt((1 - beta c_l)(1 - beta c_l+1))) and multiplied by gamma^3.  flux [n_zone][n] (floor 1e-99) -> photons per BIN [n_zone][n]."""
    flux = np.asarray(flux, dtype=np.float64); E = np.asarray(energy_MeV, dtype=np.float64)
    nz, n = flux.shape
    dlog = 1.0 / bins_per_dec                                                 # S1
    mid = np.empty(n)
    mid[:-1] = np.sqrt(E[:-1] * E[1:]); mid[-1] = mid[-2] * 10.0 ** dlog      # :151-155
    cos_e = np.linspace(-1.0, 1.0, N_COS_BINS_DOPPLER + 1)
    out = np.full((nz, n), 1.0e-99)
    for i in range(nz):
        num = np.where(flux[i] > 1.0e-90, flux[i] * dlog, flux[i]) / N_COS_BINS_DOPPLER        # :166-170, :179
        fac = gam_ef[i] * np.sqrt((1 - beta_ef[i] * cos_e[:-1]) * (1 - beta_ef[i] * cos_e[1:]))     # [l]
        Et = mid[None, :] * fac[:, None]                                                            # [l][j]
        # findnext(>=(E'), E, 2) - 1 with the 1-based E[1..n]: the first index m >= 2 with E[m] >= E' (S3: none -> dropped)
        m = np.searchsorted(E, Et, side="left")                  # 0-based index of the first E >= E'
        m = np.maximum(m, 1)                                     # (the search starts at the second entry)
        ok = (num[None, :] > 1.0e-99) & (m < n)
        np.add.at(out[i], (m - 1)[ok], np.broadcast_to(num[None, :], Et.shape)[ok])
        lit = out[i] > 1.0e-95
        out[i] = np.where(lit, out[i] * gam_ef[i] ** 3, 1.0e-99)                                    # :188-198 (S2)
    return out


@dataclasses.dataclass
class SummedEmission:
    """What `get_summed_emission` writes to photon_*_summed.dat, photon_tot_summed.dat and photon_tot.dat."""
    log_energy_MeV: np.ndarray        # [n_pts]  the common grid: 1e-13 MeV .. 1e12 MeV, 10 per decade
    per_process: dict                 # name -> (log10 E [n], log10 photons / (cm^2 s) per d(log10 E) [n_shell][n], -99 = none)
    per_shell: np.ndarray             # [n_shell][n_pts]  all processes, same units, -99 = none
    total: np.ndarray                 # [n_pts]


def summed_emission(prob, n_shell_endpoints, pion: PhotonPion = None, synch: PhotonSynch = None, ic: PhotonIC = None) -> SummedEmission:
    """The arithmetic of `get_summed_emission` (src/get_summed_emission.jl:37-413) on the per-zone photon fluxes of `photon_pion`,
    `photon_synch` and `photon_ic`: Doppler shift of the plasma-frame spectra, sum over the zones of every photon shell, one energy grid."""
    P = prob.params
    ends = np.asarray(n_shell_endpoints, dtype=np.int64)
    n_shells = len(ends) - 1
    gam_ef, beta_ef = np.asarray(prob.gam_ef)[1:P.n_grid + 1], np.asarray(prob.beta_ef)[1:P.n_grid + 1]
    dlog = 1.0 / PHOTON_BINS_PER_DEC
    n_pts = int((math.log10(PHOTON_E_MAX_MEV) - math.log10(PHOTON_E_MIN_MEV)) * PHOTON_BINS_PER_DEC)
    grid = math.log10(PHOTON_E_MIN_MEV) + dlog * np.arange(n_pts)
    total = np.full((n_shells, n_pts + 1), 1.0e-99)
    per = {}
    for name, ph, e_min, shift in (("pion", pion, PHOTON_PION_E_MIN_MEV, True), ("synch", synch, PHOTON_E_MIN_MEV, True), ("ic", ic, PHOTON_IC_E_MIN_MEV, False)):
        if ph is None:
            continue
        E = np.asarray(ph.energy_MeV)[:-1]                       # "the subroutines don't write out the final value of each spectrum" (:457-466)
        f = np.asarray(ph.photon_flux)[:, :-1]
        if shift:
            nb = doppler_to_ism(f, E, gam_ef, beta_ef)
        else:
            nb = np.where(f > 1.0e-90, f * dlog, f)              # (inverse Compton is computed in the ISM frame: number per bin only)
        sh = np.full((n_shells, len(E)), 1.0e-99)
        for n in range(n_shells):                                # sum_spectral_regions (:788-797)
            lo, hi = int(ends[n]), int(ends[n + 1]) - 1
            if lo >= 1 and hi >= lo:
                sh[n] = np.maximum(np.where(nb[lo - 1:hi] > 1.0e-95, nb[lo - 1:hi], 0.0).sum(axis=0), 1.0e-99)     # (S6)
        start = int(math.log10(e_min / PHOTON_E_MIN_MEV) * PHOTON_BINS_PER_DEC)      # :263-265
        total[:, start + 1:start + 1 + len(E)] += np.where(sh > 1.0e-99, sh, 0.0)    # :277, S4
        per[name] = (np.log10(E), np.where(sh > 1.0e-99, np.log10(np.maximum(sh, 1e-300) / dlog), -99.0))
    tot_sh = total[:, 1:n_pts + 1]                                # (the total's index n_start + j is 1-based)
    tot_all = tot_sh.sum(axis=0)
    back = lambda a: np.where(a > 1.0e-96, np.log10(np.maximum(a, 1e-300) / dlog), -99.0)       # :297-312
    return SummedEmission(grid, per, back(tot_sh), back(tot_all))


def _takes_download(backend) -> bool:
    import inspect
    return "download" in inspect.signature(backend.dndp_2d).parameters


# ---- the observed shell spectra (K9; include/mcs.h "observed shell spectra"): what `summed_emission` computes, per process and as numbers
# (not log10), from the emission a fold returns -- on the device where the backend has `photon_observe`, else by `shell_spectra_host`,
# the numpy statement of the same definition.  Every word of the two is required to have the same bits (tests/test_gpu_photon_observed.py).
PHOTON_PROCESSES = ("synch", "ic", "pion")           # the order of the sections of a photons sample (ensemble.py)


def photon_flux_host(process: str, emis, energy_div, area):
    """Step 1: the photon flux at Earth per d(log E), floor 1e-99, as `photon_synch` (:197-199), `photon_ic` (:281-282) and `photon_pion`
    (:325-329) convert their emission."""
    emis = np.asarray(emis, dtype=np.float64); E = np.asarray(energy_div, dtype=np.float64)
    if process == "synch":
        flux_erg = emis / area
        flux_erg = np.where(flux_erg > 1.0e-99, flux_erg, 1.0e-99)          # (as the definition reads: a NaN becomes the floor)
        eflux = np.where(flux_erg > 1.0e-99, flux_erg / MEV_ERG, 1.0e-99)
    elif process == "ic":
        eflux = np.where(emis > 1.0e-99, emis / MEV_ERG, 1.0e-99)
    elif process == "pion":
        eflux = emis / area
        eflux = np.where(eflux >= 1.0e-99, eflux, 1.0e-99)
    else:
        raise ValueError(f"photon process {process!r}: one of {PHOTON_PROCESSES}")
    return np.where(eflux <= 1.0e-99, 1.0e-99, eflux / E[None, :])


def shell_spectra_host(process: str, emis, energy_div, energy_grid, area, dlog, last_mid_ratio, cos_edge, gam_ef, beta_ef, gam3_ef, shell_ends,
                       flux=None):
    """The definition of mcs_photon_observe in numpy: photons per bin [n_shells + 1][n_photon - 1] of every shell and, last row, of all
    shells, floor 1e-99.  The arguments are those of HipBackend.photon_observe; flux (the [n_grid][n_photon] result of step 1) may be
    given in place of emis.  The Doppler step is `doppler_to_ism` with the caller's tables; np.add.at adds in ascending slice and,
    within a slice, ascending energy -- the order the device gathers in."""
    if process not in PHOTON_PROCESSES:
        raise ValueError(f"photon process {process!r}: one of {PHOTON_PROCESSES}")
    if flux is None:
        flux = photon_flux_host(process, emis, energy_div, area)
    f = np.asarray(flux, dtype=np.float64)[:, :-1]               # the last energy of a spectrum is not written out (:431-432)
    E = np.asarray(energy_grid, dtype=np.float64)[:-1]
    nz, n = f.shape
    ends = np.asarray(shell_ends, dtype=np.int64)
    n_shells = len(ends) - 1
    if process == "ic":
        nb = np.where(f > 1.0e-90, f * dlog, f)                  # S5
    else:
        cos_e = np.asarray(cos_edge, dtype=np.float64)
        n_cos = len(cos_e) - 1
        mid = np.empty(n)
        mid[:-1] = np.sqrt(E[:-1] * E[1:]); mid[-1] = mid[-2] * last_mid_ratio
        nb = np.full((nz, n), 1.0e-99)
        for i in range(nz):
            num = np.where(f[i] > 1.0e-90, f[i] * dlog, f[i]) / n_cos
            fac = gam_ef[i] * np.sqrt((1 - beta_ef[i] * cos_e[:-1]) * (1 - beta_ef[i] * cos_e[1:]))
            Et = mid[None, :] * fac[:, None]
            m = np.maximum(np.searchsorted(E, Et, side="left"), 1)
            ok = (num[None, :] > 1.0e-99) & (m < n)
            np.add.at(nb[i], (m - 1)[ok], np.broadcast_to(num[None, :], Et.shape)[ok])
            nb[i] = np.where(nb[i] > 1.0e-95, nb[i] * gam3_ef[i], 1.0e-99)
    out = np.full((n_shells + 1, n), 1.0e-99)
    allsh = np.zeros(n)
    for s in range(n_shells):
        lo, hi = int(ends[s]), int(ends[s + 1]) - 1
        if lo >= 1 and hi >= lo:
            a = np.where(nb[lo - 1:hi] > 1.0e-95, nb[lo - 1:hi], 0.0).sum(axis=0)      # S6
            out[s] = np.where(a > 1.0e-99, a, 1.0e-99)
        allsh = allsh + np.where(out[s] > 1.0e-99, out[s], 0.0)
    out[n_shells] = np.where(allsh > 1.0e-99, allsh, 1.0e-99)
    return out


@dataclasses.dataclass
class PhotonSetup:
    """What the observed spectra need beyond the run itself: the photon shells (`photon_shells`) and the source's distance."""
    num_upstream_shells: int
    num_downstream_shells: int
    jet_dist_kpc: float = 1.0e6
    redshift: float = 0.0
    jet_sph_frac: object = None

    @property
    def n_shells(self) -> int:
        return int(self.num_upstream_shells) + int(self.num_downstream_shells)


@dataclasses.dataclass
class PhotonLayout:
    """The photons sample of the ensemble statistics (mcs_ens_set_photon_layout): energies per process and their offsets on the common
    grid of `summed_emission` (:442)."""
    n_shells: int
    n: dict            # process -> energy words (n_photon - 1)
    start: dict        # process -> offset on the common grid
    n_pts: int

    def args(self):
        return (self.n_shells, *(int(self.n[p]) for p in PHOTON_PROCESSES), *(int(self.start[p]) for p in PHOTON_PROCESSES), self.n_pts)

    @property
    def rows(self) -> int:
        return self.n_shells + 1

    def offsets(self) -> dict:
        """section -> (first word, row length) of the sample vector: synch, ic, pion, total; `total` the length of the vector."""
        o, out = 0, {}
        for name in PHOTON_PROCESSES + ("total",):
            w = self.n_pts if name == "total" else int(self.n[name])
            out[name] = (o, w)
            o += self.rows * w
        out["_total"] = o
        return out


def photon_e_min(process: str) -> float:
    return {"synch": PHOTON_E_MIN_MEV, "ic": PHOTON_IC_E_MIN_MEV, "pion": PHOTON_PION_E_MIN_MEV}[process]


def photon_n_photon(process: str) -> int:
    e_max = PHOTON_SYNCH_E_MAX_MEV if process == "synch" else PHOTON_E_MAX_MEV
    return int(math.log10(e_max / photon_e_min(process)) * PHOTON_BINS_PER_DEC)      # photon_calcs.jl:49-51


def stock_photon_layout(n_shells: int) -> PhotonLayout:
    """The layout of the stock energy grids: 179 / 139 / 119 words at offsets 0 / 110 / 130 of 250."""
    n = {p: photon_n_photon(p) - 1 for p in PHOTON_PROCESSES}
    start = {p: int(math.log10(photon_e_min(p) / PHOTON_E_MIN_MEV) * PHOTON_BINS_PER_DEC) for p in PHOTON_PROCESSES}
    n_pts = int((math.log10(PHOTON_E_MAX_MEV) - math.log10(PHOTON_E_MIN_MEV)) * PHOTON_BINS_PER_DEC)
    return PhotonLayout(int(n_shells), n, start, n_pts)


def photon_total(per_process: dict, layout: PhotonLayout) -> np.ndarray:
    """The total section of a photons sample, [n_shells + 1][n_pts]: per shell 1e-99 plus the lit words of pion decay, synchrotron and
    inverse Compton, in that order, at their offsets (S4); the last row the serial sum of the shell rows as they stand, floors included
    (`tot_sh.sum(axis=0)` of `summed_emission`)."""
    ns = layout.n_shells
    tot = np.full((ns + 1, layout.n_pts), 1.0e-99)
    for name in ("pion", "synch", "ic"):
        sh = per_process.get(name)
        if sh is None:
            continue
        a = layout.start[name]
        tot[:ns, a:a + sh.shape[1]] += np.where(sh[:ns] > 1.0e-99, sh[:ns], 0.0)
    tot[ns] = tot[:ns].sum(axis=0)
    return tot


@dataclasses.dataclass
class ObservedSpectra:
    """The photon spectra at Earth of one species: photons / (cm^2 s) per BIN, linear, floor 1e-99."""
    processes: tuple               # the processes that were observed, in the order of PHOTON_PROCESSES
    per_process: dict              # name -> [n_shells + 1][n]; the last row is the sum over the shells
    energy_MeV: dict               # name -> [n] the energies of its words
    total: np.ndarray              # [n_shells + 1][n_pts] all processes on the common grid
    log_energy_MeV: np.ndarray     # [n_pts] the common grid
    layout: PhotonLayout
    dlog: float

    def per_dlog(self) -> "ObservedSpectra":
        """The same per d(log10 E)."""
        return dataclasses.replace(self, per_process={k: v / self.dlog for k, v in self.per_process.items()}, total=self.total / self.dlog)

    def sample(self) -> np.ndarray:
        """The sample vector of the ensemble statistics: synch | ic | pion | total, an absent process 1e-99 throughout."""
        parts = []
        for name in PHOTON_PROCESSES:
            a = self.per_process.get(name)
            parts.append((np.full((self.layout.rows, self.layout.n[name]), 1.0e-99) if a is None else a).ravel())
        parts.append(self.total.ravel())
        return np.concatenate(parts)


def observe_tables(prob, setup: PhotonSetup, process: str, energy_MeV) -> dict:
    """The host tables of one mcs_photon_observe call, as keyword arguments of HipBackend.photon_observe / shell_spectra_host."""
    n = prob.params.n_grid
    gam = np.ascontiguousarray(np.asarray(prob.gam_ef, dtype=np.float64)[1:n + 1])
    beta = np.ascontiguousarray(np.asarray(prob.beta_ef, dtype=np.float64)[1:n + 1])
    E_MeV = np.ascontiguousarray(energy_MeV, dtype=np.float64)
    dist_lum = setup.jet_dist_kpc * (1 + setup.redshift) * KPC_CM
    dlog = 1.0 / PHOTON_BINS_PER_DEC
    _, zones = photon_shells(prob, setup.num_upstream_shells, setup.num_downstream_shells)
    return dict(energy_div=E_MeV * MEV_ERG if process == "pion" else E_MeV, energy_grid=E_MeV, area=4 * math.pi * dist_lum ** 2, dlog=dlog,
                last_mid_ratio=10.0 ** dlog, cos_edge=np.linspace(-1.0, 1.0, N_COS_BINS_DOPPLER + 1), gam_ef=gam, beta_ef=beta,
                gam3_ef=gam ** 3, shell_ends=zones)


def observed_spectra(prob, backend, i_ion: int, setup: PhotonSetup, ion_fin: IonFinal) -> ObservedSpectra:
    """The photon spectra at Earth of species i_ion from the tallies on the backend: its folds (electrons: synchrotron, get_dNdp_2D and
    inverse Compton; nuclei: pion decay), then frame, shells and common grid -- on the device where the backend has `photon_observe`
    (K9 reads the emission where the fold left it; the shell spectra come back and also stay there for Ensemble.add_photons), else
    through `shell_spectra_host`.  The folds themselves are the existing calls: they still hand their per-zone emission to the host."""
    sp = prob.cfg.species[i_ion - 1]
    kw = dict(jet_dist_kpc=setup.jet_dist_kpc, redshift=setup.redshift)
    folds = {}
    if sp.aa < 1:
        folds["synch"] = photon_synch(prob, backend, ion_fin, i_ion, **kw)
        folds["ic"] = photon_ic(prob, backend, i_ion, jet_sph_frac=setup.jet_sph_frac, **kw)
    else:
        folds["pion"] = photon_pion(prob, backend, ion_fin, i_ion, **kw)
    on_device = hasattr(backend, "photon_observe")
    per, energy = {}, {}
    for name in PHOTON_PROCESSES:
        if name not in folds:
            continue
        ph = folds[name]
        tabs = observe_tables(prob, setup, name, ph.energy_MeV)
        if name == "pion":       # (photon_pion keeps its energies in MeV; its flux is divided by the erg values the fold returned)
            tabs["energy_div"] = np.ascontiguousarray(ph.energy_erg)
        if on_device:
            per[name] = backend.photon_observe(name, **tabs)
        else:
            emis = ph.emis_erg if name == "ic" else ph.emis_erg_s
            per[name] = shell_spectra_host(name, emis, **tabs)
        energy[name] = np.asarray(ph.energy_MeV)[:-1]
    layout = stock_photon_layout(setup.n_shells)
    dlog = 1.0 / PHOTON_BINS_PER_DEC
    grid = math.log10(PHOTON_E_MIN_MEV) + dlog * np.arange(layout.n_pts)
    return ObservedSpectra(tuple(per), per, energy, photon_total(per, layout), grid, layout, dlog)
