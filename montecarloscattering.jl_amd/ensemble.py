"""Ensemble statistics (K8): per-cell mean and standard error of the tallies over the iterations of a fixed-profile run.

With a fixed shock profile the iterations of a run are independent Monte-Carlo realisations (driver.run_overlapped), yet the
per-species tallies a run hands back are those of the last one.  An ensemble keeps a running mean and a sum of squared
deviations M2 of every word of a SAMPLE vector, per slot (include/mcs.h, "ensemble statistics"):

  slot i_ion - 1   species samples: psd, therm_sf, therm_pf, esc_psd_up, esc_psd_down, pxx_flux, pxz_flux, energy_flux,
                   energy_recv_pool, num_crossings (as doubles), and the six marginals of the three histograms -- "<hist>_mom"
                   [n_grid][nmom+2], summed over the angle index, and "<hist>_tht" [n_grid][ntht+2], summed over the momentum
                   index: the variance of a marginal cannot be had from the per-cell variances
  slot n_species   iteration samples: esc_flux, esc_energy_eff, esc_num_eff, spectra_coupled, spectra_sf, spectra_pf as their
                   growth over the iteration (the transport never resets them), weight_coupled, energy_transfer_pool and scalars
                   as they stand at its end

  update   n += 1; d = x - mean; mean = mean + d / n; M2 = M2 + d * (x - mean)
  merge    n = na + nb; d = mb - ma; mean = ma + d * (nb / n); M2 = (qa + qb) + (d * d) * (na * nb / n)        (Chan)
  stderr   sqrt(M2 / (n (n - 1)))

Running until the error bars are small enough (`Ensemble.summarize`, `Trigger`; driver.run(triggers=...)): a summary reduces a part
of a slot -- or a contiguous slice of its zones -- to a handful of numbers, mcs_ens_summary of include/mcs.h, where the definition is:

  finite word    mean and M2 both finite; n_nonfinite counts the others, which take part in nothing else
  amax           max |mean| over the finite words (0 for an empty range)
  selected word  finite, |mean| > 0 and |mean| >= floor_frac * amax
  per selected word   se = sqrt(M2 / (n (n - 1))), rel = se / |mean|
  max_rel, argmax (the lowest word of the range that attains it; -1: nothing selected), n_over (rel > tol),
  sum_se, sum_abs_mean, sum_rel2 (of rel * rel)

An overlapped run (driver.run_overlapped) keeps one accumulator per context.  `Ensemble.summarize_merged` gives the summary of their
merge without forming it: per word the left fold of the merge above over the accumulators that have samples, in list order, then
the definition above on the merged words with the total count (mcs_ens_summarize_merged of include/mcs.h; on the device each word's
fold is made in registers, no accumulator is changed, no scratch accumulator exists).

Products (include/mcs.h, "products sample"): what a run publishes -- the normalised dN/dp in the three frames, the pressures and the
energy density of ion_finalize, the spectral slope -- is non-linear in the tallies, so its error bars cannot be had from the per-cell
ones; it is sampled once per iteration.  Every species slot s has a companion products slot, `Ensemble.products_slot(s)`, whose two
vectors exist from its first sample on:

  dNdp_sf, dNdp_pf, dNdp_isf                  [n_grid][nmom+2]: frames 0, 1, 2 of ion_finalize's dNdp_cr
  P_psd_par, P_psd_perp, energy_density_psd   [n_grid]
  slope_sf, slope_pf, slope_isf               [n_grid]: the least-squares slope of log10 dN/dp against log10 p (cgs) over the bins
      l_lo <= l < l_hi of the slope window (`set_slope_window`, `slope_window`).  A bin is valid if dN/dp > 1e-99, the consumers'
      floor of an empty bin; with the k valid bins in ascending order, every operation a separate rounding, serial sums:
      xbar = (sum x) / k, ybar = (sum y) / k, Sxx = sum (x - xbar)^2, Sxy = sum (x - xbar)(y - ybar), slope = Sxy / Sxx, where
      y = log10(dN/dp) by the deterministic log10 of include/mcs_math.h.  k < 3 gives NaN: the word stays non-finite, a summary
      counts it in n_nonfinite and a trigger over it is never met -- a slope trigger belongs on zones that the accelerated
      population reaches.  It is the slope of dN/dp, about -2.2 behind a strong shock, not the index of f(p).

Escape (include/mcs.h, "escape sample"): the spectra of the particles that leave the shock, consumers.escape_spectra, sampled once per
species and iteration by driver.run(finalize=True, escape=True, ensemble=...).  Every species slot s has a third companion, the escape
slot `Ensemble.escape_slot(s)`, whose vectors exist from its first sample on.  Its parts have as first axis the row 3 * door + frame
(door 0: upstream, 1: downstream; frame 0: shock, 1: the door's plasma frame, 2: ISM):

  dNdp     [6][nmom+2]: dN/dp of the row
  number   [6]: the row's summed weight
  slope    [6]: the slope of the row over the slope window, by the products sample's rule

zones=Ensemble.escape_row(door, frame) of a `Request` or `Trigger` selects one door and frame, bins= a momentum window of that dNdp
row.  The slope window is shared with the products slots: it is fixed from the first products or escape sample on.

Angles (include/mcs.h, "angles sample"): the pitch-angle distributions of consumers.angle_distributions (K11), sampled once per species
and iteration by driver.run(finalize=True, angles=[(p_lo, p_hi), ...], ensemble=...).  Every species slot s has a fourth companion, the
angles slot `Ensemble.angles_slot(s)`, whose vectors exist from its first sample on.  The ensemble holds the momentum windows of its
angles samples (`set_angle_windows`; consumers.momentum_windows makes them from cgs momenta): they may be set again until the first
angles sample and are fixed from then on; merge, summarize_merged and compare refuse ensembles whose windows differ, and a merge
into an ensemble without windows gives it the source's.  Its parts have as first axis the row (frame * n_grid + zone) * n_win + window
(frame 0: shock, 1: the zone's plasma frame, 2: ISM; zone 0-based):

  dist      [rows][ntht+2]: the normalised distribution over the angle bins, 1e-99 in an empty bin
  number    [rows]: the summed weight of the window
  mean_mu   [rows]: <mu>
  mean_mu2  [rows]: <mu^2>

zones=Ensemble.angles_row(frame, zone, window) of a `Request`, `Trigger`, `CompareRequest` or `Agreement` selects one row, bins= angle
bins of that dist row.  A window that no particle reached has NaN moments in that sample: the word's mean stays non-finite, a summary
counts it in n_nonfinite and a trigger over it is never met -- windows belong on zones and momenta that the population reaches.

Tcuts (include/mcs.h, "tcuts sample"): the time-cut spectra of consumers.tcut_spectra (K12), sampled once per species and iteration by
driver.run(finalize=True, tcuts=True, ensemble=...).  Every species slot s has a fifth companion, the tcuts slot
`Ensemble.tcuts_slot(s)`, whose vectors exist from its first sample on.  The number of time cuts nt is fixed by the ensemble's first
tcuts sample; a later sample, merge, summarize_merged or compare with another nt is refused.  Its parts:

  spectrum    [nt][nmom+2]: the species' growth of spectra_coupled in the iteration, normalised per cut; 1e-99 in an empty bin
  weight      [nt]: weight_coupled, floored as tcut_print floors it
  number      [nt]: the sum a spectrum row was normalised with
  mean_log_p  [nt]: the mean of log10 p over the row
  quantile    [3][nt]: log10 of the momentum below which 50, 90, 99 % of the still-coupled weight lies, "p reached by time t"
  index       [3]: the slope of each quantile against log10 t over the live cuts

zones=Ensemble.tcuts_row(k) of a `Request`, `Trigger` or `CompareRequest` selects cut k of spectrum, weight, number and mean_log_p,
bins= a momentum window of that spectrum row; of quantile, zones=(j, j + 1) selects the quantile and bins=Ensemble.tcuts_row(k) the
cut.  A cut that no particle reached is a dead row: its mean_log_p and quantiles are NaN in that sample, the word's mean stays
non-finite, a summary counts it in n_nonfinite and a trigger over it is never met -- triggers belong on cuts below age_max (the last
cut lies above 10 age_max and is always dead).

Detectors (include/mcs.h, "detectors sample"): the spectra at the XSPEC detectors, consumers.detector_spectra (K14), sampled once per
species and iteration by driver.run(finalize=True, detectors=True, ensemble=...).  Every species slot s has a sixth companion, the
detectors slot `Ensemble.detectors_slot(s)`, whose vectors exist from its first sample on.  The ensemble keeps the settings of its
first detectors sample -- the number of detectors nd, the slope window, the bits of x_unit and of x_spec; a later sample, merge,
summarize_merged or compare with other settings is refused.  Its parts, with the row r = frame * nd + d (frame 0: shock, 1: plasma):

  spectrum    [2 nd][nmom+2]: the species' growth of the detector's row in the iteration, normalised per row; 1e-99 in an empty bin
  dndp        [2 nd][nmom+2]: that growth per unit momentum
  number      [2 nd]: the sum a spectrum row was normalised with
  mean_log_p  [2 nd]: the mean of log10 p over the row
  quantile    [3][2 nd]: log10 of the momentum below which 50, 90, 99 % of the weight lies
  slope       [2 nd]: d log10 dndp / d log10 p over the window
  gradient    [nmom+2]: per momentum bin, d log10 g / d (x / x_unit) over the upstream detectors: ln 10 times it is u0 / D(p)

zones=Ensemble.detectors_row(frame, d) of a `Request`, `Trigger` or `CompareRequest` selects one row of spectrum, dndp, number,
mean_log_p and slope, bins= a momentum window of that spectrum or dndp row; of quantile, zones=(j, j + 1) selects the quantile and
bins=Ensemble.detectors_row(frame, d) the row; of gradient, zones=(l_lo, l_hi) selects momentum bins.  A detector that no particle
crossed is a dead row, and a gradient bin lit in fewer than three upstream detectors is NaN in that sample: the word's mean stays
non-finite, a summary counts it in n_nonfinite and a trigger over it is never met.

Profile (include/mcs.h, "profile sample"): the shock profile that smooth_grid_par WOULD write from an iteration's fluxes and pressures,
consumers.profile_update (K13), sampled once per iteration by driver.run(finalize=True, profile=True, ensemble=...) of a run with a
FIXED profile: the mean and standard error of that prediction say how far the current profile is from self-consistency.  One slot
per ensemble, `Ensemble.profile_slot`, whose vectors exist from its first sample on.  The ensemble keeps the settings of its first
sample's ProfileIn (upstream fluxes, species sums, compression ratios, SMMOE, SMPFP, the old-profile weight, i_trans); a later sample,
merge, summarize_merged or compare whose settings differ in any bit is refused.  Its parts are ten rows [n_grid] -- flux_px, flux_en,
gamma_ad, p_flux, p_used, ux_px, ux_en, ux_pred, ux_next, shift -- of which zones=(a, b) selects zones, and scalars [8] (gamma_down,
px_esc_up, en_esc_up, q_px, q_en, q_px_avg, q_en_avg, shift_rms).  `profile_consistency(ens)` turns mean and M2 of `shift` into
per-zone z-scores and their chi-square over the upstream zones.

Photons (include/mcs.h, "photons sample"): the photon spectra at Earth per photon shell, consumers.observed_spectra.  A shell spectrum is
a sum over zones, slices in cos(theta) and processes, so its variance does not follow from per-cell variances either: every species
slot s has a second companion, `Ensemble.photons_slot(s)`, sampled once per iteration (`add_photons`) and allocated at its first
sample.  `set_photon_layout` (a consumers.PhotonLayout) fixes the vector before that:

  synch, ic, pion   [n_shells + 1][n]: photons per bin of every shell and, last row, of all shells; a process that was not observed
                    enters as 1e-99 throughout
  total             [n_shells + 1][n_pts]: the three on the common energy grid (consumers.photon_total)

zones= of a `Request` or `Trigger` selects shell rows of one of these parts, bins= an energy window of one row.

The source (include/mcs.h, "source sample"): an observer sees one spectrum, summed over species, and the species of an iteration are
correlated, so the sum is sampled itself.  `Ensemble.photons_all_slot`, one per ensemble, has the photons layout and names.  A species'
sample taken with `add_photons(..., deposit=True)` also joins a pending vector -- per word 1e-99, or what earlier deposits left, plus
the word where it is above 1e-99 -- and `add_photons_all` takes that vector as one sample and forgets the deposits
(`pending_photons`, `drop_pending_photons`).  A species slot deposits once between two takes.

A summary range can be restricted in momentum: `Request` / `Trigger(bins=(l_lo, l_hi))` together with a single zone, zones=(z, z+1),
on a part of shape [zone][bins] (the three dNdp_* and the six marginals) is the word range off + z * per + l_lo of l_hi - l_lo
words.  dN/dp spans a dozen decades: without it the floor_frac selection keeps the thermal peak and drops the tail.  Several zones
are several requests (MAX_RANGES in one summary).

Does run B agree with run A within their error bars?  `Ensemble.compare` (`CompareRequest`, `Difference`, `Agreement`,
`check_agreements`) holds a slot of one ensemble against a slot of the same kind of another -- or of the same one: protons against
He -- word by word, mcs_ens_compare of include/mcs.h, where the definition is:

  per word       va = M2_a / (n_a (n_a - 1)), vb likewise; s2 = va + vb; d = mean_a - mean_b; scale = max(|mean_a|, |mean_b|)
  finite word    both means, both M2, d and s2 are finite; n_nonfinite counts the others, which take part in nothing else
  amax           max scale over the finite words; selected word: finite, scale > 0 and scale >= floor_frac * amax
  degenerate     a selected word with s2 == 0 and d != 0 (n_degenerate; it has no z)
  z              0 where s2 == 0 and d == 0, else d / sqrt(s2)
  max_abs_z, argmax, n_over (|z| > zcut), sum_z, sum_abs_z, sum_z2 (the chi-square) over the selected words that have a z;
  sum_abs_diff, sum_scale over all selected words

`Agreement` says what the numbers mean with few samples.

`HipEnsemble` keeps the vectors on the device and updates them with the kernels of csrc/mcs_ensemble.hip: the 22 MB histograms
never cross to the host (it costs device memory: two vectors of the sample length per slot, about twice the tally buffer per
species slot).  `HostEnsemble` does the same arithmetic in numpy, in the same order, on read_tallies() buffers: it lets the driver
path run with the CPU test backends (driver.accumulate_tallies_host is the precedent).  `Ensemble.for_backend` picks one.
"""
from __future__ import annotations

import ctypes as ct
import dataclasses
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import capi
from .hip_backend import HipBackend

HISTOGRAMS = ("psd", "therm_sf", "therm_pf")
SPECIES_TALLIES = ("psd", "therm_sf", "therm_pf", "esc_psd_up", "esc_psd_down", "pxx_flux", "pxz_flux", "energy_flux")
MARGINALS = tuple(f"{h}_{axis}" for h in HISTOGRAMS for axis in ("mom", "tht"))
SPECIES_NAMES = SPECIES_TALLIES + ("energy_recv_pool", "num_crossings") + MARGINALS
# inside [esc_flux, energy_recv_pool) | scalars: what enters as growth since begin_iteration, and what as it stands
ITERATION_INCREMENTS = ("esc_flux", "esc_energy_eff", "esc_num_eff", "spectra_coupled", "spectra_sf", "spectra_pf")
ITERATION_AS_IS = ("weight_coupled", "energy_transfer_pool", "scalars")
# (px_esc_feb and energy_esc_feb are indexed by iteration: they are part of the sample vector, their statistics mean nothing)
ITERATION_NAMES = ITERATION_INCREMENTS + ITERATION_AS_IS
# the parts whose first axis is the zone index: a zone slice of one is a contiguous word range
ZONE_PARTS = HISTOGRAMS + ("pxx_flux", "pxz_flux", "energy_flux", "energy_recv_pool", "num_crossings") + MARGINALS + (
    "spectra_sf", "spectra_pf", "energy_transfer_pool")
STATISTICS = ("max", "rms", "weighted", "fraction_over")
MAX_RANGES = 256          # of one mcs_ens_summarize call
MAX_MERGED = 8            # accumulators of one mcs_ens_summarize_merged call (MCS_ENS_MAX_MERGED)
# what run_overlapped(ensemble=True) adds from the per-iteration ion_finalize of the last species
FINALIZE_NAMES = ("dNdp_cr", "P_psd_par", "P_psd_perp", "energy_density_psd")
# the parts of a products slot, in the order of mcs_ens_products_layout; all have the zone as first axis
PRODUCT_DNDP = ("dNdp_sf", "dNdp_pf", "dNdp_isf")
PRODUCT_SLOPES = ("slope_sf", "slope_pf", "slope_isf")
PRODUCT_NAMES = PRODUCT_DNDP + ("P_psd_par", "P_psd_perp", "energy_density_psd") + PRODUCT_SLOPES
ZONE_PARTS = ZONE_PARTS + PRODUCT_NAMES
# the parts of shape [zone][bins]: a bins=(l_lo, l_hi) window of one zone of them is a contiguous word range
BIN_PARTS = PRODUCT_DNDP + MARGINALS
PRODUCTS_BIT = capi.ENS_PRODUCTS_BIT      # products slot of species slot s: s | PRODUCTS_BIT (MCS_ENS_PRODUCTS)
DNDP_FLOOR = 1.0e-99                      # the consumers' floor: a bin at or below it is empty
# the parts of a photons slot, in the order of mcs_ens_photons_layout: first axis the shell row (zones=), second the energy (bins=)
PHOTON_NAMES = ("synch", "ic", "pion", "total")
ZONE_PARTS = ZONE_PARTS + PHOTON_NAMES
BIN_PARTS = BIN_PARTS + PHOTON_NAMES
PHOTONS_BIT = capi.ENS_PHOTONS_BIT        # photons slot of species slot s: s | PHOTONS_BIT (MCS_ENS_PHOTONS)
PHOTONS_ALL = capi.ENS_PHOTONS_ALL        # the source slot: the photon spectrum summed over species (MCS_ENS_PHOTONS_ALL)
# the parts of an escape slot, in the order of mcs_ens_escape_layout: first axis the row 3 * door + frame (zones=; Ensemble.escape_row),
# dNdp's second the momentum bin (bins=)
ESCAPE_NAMES = ("dNdp", "number", "slope")
ESCAPE_ROWS = 6
ZONE_PARTS = ZONE_PARTS + ESCAPE_NAMES
BIN_PARTS = BIN_PARTS + ("dNdp",)
ESCAPE_BIT = capi.ENS_ESCAPE_BIT          # escape slot of species slot s: s | ESCAPE_BIT (MCS_ENS_ESCAPE)
# the parts of an angles slot, in the order of mcs_ens_angles_layout: first axis the row (frame * n_grid + zone) * n_win + window
# (zones=; Ensemble.angles_row), dist's second the angle bin (bins=)
ANGLES_NAMES = ("dist", "number", "mean_mu", "mean_mu2")
ANGLE_MAX_WINDOWS = 8                     # MCS_ANGLE_MAX_WINDOWS
ZONE_PARTS = ZONE_PARTS + tuple(n for n in ANGLES_NAMES if n not in ZONE_PARTS)
BIN_PARTS = BIN_PARTS + ("dist",)
ANGLES_BIT = capi.ENS_ANGLES_BIT          # angles slot of species slot s: s | ANGLES_BIT (MCS_ENS_ANGLES)
# the parts of a tcuts slot, in the order of mcs_tcut_layout: first axis the cut (zones=; Ensemble.tcuts_row), spectrum's second the
# momentum bin (bins=); quantile is [quantile][cut]
TCUTS_NAMES = ("spectrum", "weight", "number", "mean_log_p", "quantile", "index")
ZONE_PARTS = ZONE_PARTS + tuple(n for n in TCUTS_NAMES if n not in ZONE_PARTS)
BIN_PARTS = BIN_PARTS + ("spectrum", "quantile")
TCUTS_BIT = capi.ENS_TCUTS_BIT            # tcuts slot of species slot s: s | TCUTS_BIT (MCS_ENS_TCUTS)
# the parts of a detectors slot, in the order of mcs_detector_layout: first axis the row frame * nd + d (zones=; Ensemble.detectors_row),
# spectrum's and dndp's second the momentum bin (bins=); quantile is [quantile][row]; gradient's only axis is the momentum bin
DETECTORS_NAMES = ("spectrum", "dndp", "number", "mean_log_p", "quantile", "slope", "gradient")
ZONE_PARTS = ZONE_PARTS + tuple(n for n in DETECTORS_NAMES if n not in ZONE_PARTS)
BIN_PARTS = BIN_PARTS + ("dndp",)
DETECTORS_BIT = capi.ENS_DETECTORS_BIT    # detectors slot of species slot s: s | DETECTORS_BIT (MCS_ENS_DETECTORS)
# the parts of the profile slot, in the order of mcs_profile_layout: ten rows over the zones (zones=), then the scalars
PROFILE_ROW_NAMES = ("flux_px", "flux_en", "gamma_ad", "p_flux", "p_used", "ux_px", "ux_en", "ux_pred", "ux_next", "shift")
PROFILE_SCALAR_NAMES = ("gamma_down", "px_esc_up", "en_esc_up", "q_px", "q_en", "q_px_avg", "q_en_avg", "shift_rms")
PROFILE_NAMES = PROFILE_ROW_NAMES + ("scalars",)
ZONE_PARTS = ZONE_PARTS + tuple(n for n in PROFILE_ROW_NAMES if n not in ZONE_PARTS)
PROFILE_SLOT = capi.ENS_PROFILE           # the profile slot, one per ensemble (MCS_ENS_PROFILE)


class EnsLayout:
    """Python mirror of `mcs_ens_get_layout`: where every named part lies in the two sample vectors."""

    def __init__(self, P: capi.McsParams):
        L = self.tally = capi.Layout(P)
        ng, nm, nt = P.n_grid, P.num_psd_mom_bins + 2, P.num_psd_tht_bins + 2
        o = L.offsets
        self.species: Dict[str, Tuple[int, tuple]] = {}
        for name in SPECIES_TALLIES:
            self.species[name] = (o[name] - o["psd"], L.shapes[name])
        w = o["esc_flux"] - o["psd"]
        self.fields = dict(sp_tallies=0, sp_tallies_n=w, sp_recv_pool=w, sp_recv_pool_n=ng, sp_num_crossings=w + ng, sp_num_crossings_n=ng,
                           sp_marg_mom_n=ng * nm, sp_marg_tht_n=ng * nt)
        self.species["energy_recv_pool"] = (w, (ng,))
        self.species["num_crossings"] = (w + ng, (ng,))
        w += 2 * ng
        for name in MARGINALS:
            shape = (ng, nm) if name.endswith("_mom") else (ng, nt)
            self.species[name] = (w, shape)
            self.fields["sp_" + name] = w
            w += shape[0] * shape[1]
        self.species_total = w
        self.iteration: Dict[str, Tuple[int, tuple]] = {}
        n_sums = o["energy_recv_pool"] - o["esc_flux"]
        for name in capi.RUNNING_F64:
            self.iteration[name] = ((n_sums if name == "scalars" else o[name] - o["esc_flux"]), L.shapes[name])
        self.iteration_total = n_sums + (L.total - o["scalars"])
        self.fields.update(sp_total=w, it_sums=0, it_sums_n=n_sums, it_scalars=n_sums, it_scalars_n=L.total - o["scalars"],
                           it_total=self.iteration_total, tally_sp_first=o["psd"], tally_it_first=o["esc_flux"],
                           tally_recv_pool=o["energy_recv_pool"], tally_scalars=o["scalars"])
        # the products sample: mirror of `mcs_ens_products_get_layout`
        self.products: Dict[str, Tuple[int, tuple]] = {}
        w = 0
        for name in PRODUCT_NAMES:
            shape = (ng, nm) if name in PRODUCT_DNDP else (ng,)
            self.products[name] = (w, shape)
            w += int(np.prod(shape))
        self.products_total = w
        self.products_fields = {name: off for name, (off, _) in self.products.items()}
        self.products_fields.update(dNdp_n=ng * nm, zone_n=ng, total=w)
        # the escape sample: mirror of `mcs_ens_escape_get_layout`
        self.escape: Dict[str, Tuple[int, tuple]] = {"dNdp": (0, (ESCAPE_ROWS, nm)), "number": (ESCAPE_ROWS * nm, (ESCAPE_ROWS,)),
                                                     "slope": (ESCAPE_ROWS * nm + ESCAPE_ROWS, (ESCAPE_ROWS,))}
        self.escape_total = ESCAPE_ROWS * nm + 2 * ESCAPE_ROWS
        self.escape_fields = dict(dNdp=0, number=ESCAPE_ROWS * nm, slope=ESCAPE_ROWS * nm + ESCAPE_ROWS, row_n=nm, total=self.escape_total)

    def angles(self, n_win: int) -> Dict[str, Tuple[int, tuple]]:
        """The angles sample of n_win windows: mirror of `mcs_ens_angles_get_layout` (the one layout that depends on a setting)."""
        nt = self.tally.shapes["psd"][1]
        rows = 3 * self.tally.n_grid * int(n_win)
        return {"dist": (0, (rows, nt)), "number": (rows * nt, (rows,)), "mean_mu": (rows * nt + rows, (rows,)),
                "mean_mu2": (rows * nt + 2 * rows, (rows,))}

    def angles_fields(self, n_win: int) -> Dict[str, int]:
        t = self.angles(n_win)
        rows, nt = t["dist"][1]
        return dict(dist=0, number=t["number"][0], mean_mu=t["mean_mu"][0], mean_mu2=t["mean_mu2"][0], row_n=nt, rows=rows, total=rows * (nt + 3))

    def tcuts(self, n_tcuts: int) -> Dict[str, Tuple[int, tuple]]:
        """The tcuts sample of n_tcuts cuts: mirror of `mcs_ens_tcuts_get_layout`."""
        nm, nt = self.tally.shapes["psd"][2], int(n_tcuts)
        a = nt * nm
        return {"spectrum": (0, (nt, nm)), "weight": (a, (nt,)), "number": (a + nt, (nt,)), "mean_log_p": (a + 2 * nt, (nt,)),
                "quantile": (a + 3 * nt, (3, nt)), "index": (a + 6 * nt, (3,))}

    def tcuts_fields(self, n_tcuts: int) -> Dict[str, int]:
        t = self.tcuts(n_tcuts)
        nt, nm = t["spectrum"][1]
        return dict({name: off for name, (off, _) in t.items()}, row_n=nm, n_tcuts=nt, total=nt * (nm + 6) + 3)

    def detectors(self, n_det: int) -> Dict[str, Tuple[int, tuple]]:
        """The detectors sample of n_det detectors: mirror of `mcs_ens_detectors_get_layout`, the frame and the detector as one row axis."""
        nm, r = self.tally.shapes["psd"][2], 2 * int(n_det)
        a = r * nm
        return {"spectrum": (0, (r, nm)), "dndp": (a, (r, nm)), "number": (2 * a, (r,)), "mean_log_p": (2 * a + r, (r,)),
                "quantile": (2 * a + 2 * r, (3, r)), "slope": (2 * a + 5 * r, (r,)), "gradient": (2 * a + 6 * r, (nm,))}

    def detectors_fields(self, n_det: int) -> Dict[str, int]:
        t = self.detectors(n_det)
        r, nm = t["spectrum"][1]
        return dict({name: off for name, (off, _) in t.items()}, row_n=nm, n_det=r // 2, total=r * (2 * nm + 6) + nm)

    def profile(self) -> Dict[str, Tuple[int, tuple]]:
        """The profile sample: mirror of `mcs_ens_profile_get_layout`."""
        n = self.tally.shapes["pxx_flux"][0]
        t = {name: (k * n, (n,)) for k, name in enumerate(PROFILE_ROW_NAMES)}
        t["scalars"] = (len(PROFILE_ROW_NAMES) * n, (len(PROFILE_SCALAR_NAMES),))
        return t

    def profile_fields(self) -> Dict[str, int]:
        t = self.profile()
        n = t["shift"][1][0]
        return dict({name: off for name, (off, _) in t.items()}, row_n=n, n_scalars=len(PROFILE_SCALAR_NAMES),
                    total=len(PROFILE_ROW_NAMES) * n + len(PROFILE_SCALAR_NAMES))

    def species_sample(self, f: np.ndarray, i: np.ndarray) -> np.ndarray:
        """The species sample of the tally buffers (f, i).  The marginals are serial sums in ascending index order, one index
        slice at a time (np.sum adds pairwise and would round differently)."""
        L, o = self.tally, self.tally.offsets
        x = np.empty(self.species_total)
        n1 = o["esc_flux"] - o["psd"]
        x[:n1] = f[o["psd"]:o["esc_flux"]]
        x[n1:n1 + L.n_grid] = L.view(f, "energy_recv_pool")
        x[n1 + L.n_grid:n1 + 2 * L.n_grid] = i[:L.n_grid].astype(np.float64)
        for h in HISTOGRAMS:
            hist = L.view(f, h)                       # [n_grid][ntht+2][nmom+2]
            mom = hist[:, 0, :].copy()
            for j in range(1, hist.shape[1]):
                mom = mom + hist[:, j, :]
            tht = hist[:, :, 0].copy()
            for k in range(1, hist.shape[2]):
                tht = tht + hist[:, :, k]
            for name, a in ((h + "_mom", mom), (h + "_tht", tht)):
                off = self.species[name][0]
                x[off:off + a.size] = a.ravel()
        return x

    def iteration_sample(self, f: np.ndarray, snapshot: np.ndarray) -> np.ndarray:
        """The iteration sample of the buffer f; snapshot: words [esc_flux, energy_recv_pool) at the begin of the iteration."""
        o = self.tally.offsets
        n_sums = o["energy_recv_pool"] - o["esc_flux"]
        x = np.empty(self.iteration_total)
        x[:n_sums] = f[o["esc_flux"]:o["energy_recv_pool"]]
        for name in ITERATION_INCREMENTS:
            off, shape = self.iteration[name]
            n = int(np.prod(shape))
            x[off:off + n] = x[off:off + n] - snapshot[off:off + n]
        x[n_sums:] = f[o["scalars"]:]
        return x


def welford_update(mean: np.ndarray, m2: np.ndarray, n: int, x: np.ndarray) -> int:
    """One sample more, in place -> the new count."""
    n += 1
    d = x - mean
    mean[...] = mean + d / float(n)
    m2[...] = m2 + d * (x - mean)
    return n


def _chan(m, q, na: int, mb, qb, nb: int):
    """Chan's merge of (mean m, M2 q, na samples) with (mb, qb, nb) -> the merged (mean, M2), new arrays: the one place where the
    formula stands.  A merge that is not finite is counted by a summary, not an error."""
    n = float(na + nb)
    with np.errstate(over="ignore", invalid="ignore"):
        d = mb - m
        return m + d * (float(nb) / n), (q + qb) + (d * d) * (float(na) * float(nb) / n)


class _Slot:
    """The mean, the M2 and the sample count of one slot."""

    def __init__(self, size: int):
        self.mean, self.m2, self.n = np.zeros(size), np.zeros(size), 0

    def copy(self) -> "_Slot":
        c = _Slot(0)
        c.mean, c.m2, c.n = self.mean.copy(), self.m2.copy(), self.n
        return c


def stats_over(samples):
    """(mean, standard error of the mean, count) of a list of equally shaped arrays, by the update above, in list order."""
    mean, m2, n = np.zeros_like(samples[0], dtype=np.float64), np.zeros_like(samples[0], dtype=np.float64), 0
    for x in samples:
        n = welford_update(mean, m2, n, np.asarray(x, dtype=np.float64))
    err = np.sqrt(m2 / (float(n) * float(n - 1))) if n >= 2 else np.full_like(mean, np.nan)
    return mean, err, n


def _check_part(name: str, zones, bins=None):
    """What can be said of a part without an ensemble: the name exists, a zone slice is a pair and the part has a zone axis, a bins
    window is a pair, comes with a single zone and the part has a bins axis."""
    if name not in SPECIES_NAMES + ITERATION_NAMES + PRODUCT_NAMES + PHOTON_NAMES + ESCAPE_NAMES + ANGLES_NAMES + TCUTS_NAMES + PROFILE_NAMES + DETECTORS_NAMES:
        raise ValueError(f"ensemble: no part {name!r}; a species slot has: {', '.join(SPECIES_NAMES)}; the iteration slot: {', '.join(ITERATION_NAMES)}; "
                         f"a products slot: {', '.join(PRODUCT_NAMES)}; a photons slot: {', '.join(PHOTON_NAMES)}; "
                         f"an escape slot: {', '.join(ESCAPE_NAMES)}; an angles slot: {', '.join(ANGLES_NAMES)}; "
                         f"a tcuts slot: {', '.join(TCUTS_NAMES)}; the profile slot: {', '.join(PROFILE_NAMES)}; "
                         f"a detectors slot: {', '.join(DETECTORS_NAMES)}")
    if bins is not None:
        if name not in BIN_PARTS:
            raise ValueError(f"ensemble: {name!r} has no [zone][bins] shape; a bins window fits: {', '.join(BIN_PARTS)}")
        if len(bins) != 2 or int(bins[0]) != bins[0] or int(bins[1]) != bins[1]:
            raise ValueError(f"ensemble: a bins window is a pair (l_lo, l_hi) of integers, not {bins!r}")
        if zones is None or len(zones) != 2 or zones[1] != zones[0] + 1:
            raise ValueError(f"ensemble: a bins window needs a single zone, zones=(z, z + 1), not zones={zones!r}; several zones are several requests")
    if zones is not None:
        if name not in ZONE_PARTS:
            raise ValueError(f"ensemble: {name!r} has no zone axis; a zone slice fits: {', '.join(ZONE_PARTS)}")
        if len(zones) != 2 or int(zones[0]) != zones[0] or int(zones[1]) != zones[1]:
            raise ValueError(f"ensemble: a zone slice is a pair (z_lo, z_hi) of integers, not {zones!r}")


@dataclasses.dataclass(frozen=True)
class Request:
    """One range of a summary: a named part of a slot, or its zones [z_lo, z_hi) where the part's first axis is the zone index, or
    the bins [l_lo, l_hi) of one zone (zones=(z, z + 1)) of a part of shape [zone][bins]."""
    name: str
    zones: Optional[Tuple[int, int]] = None
    floor_frac: float = 1e-3
    tol: float = 0.0
    bins: Optional[Tuple[int, int]] = None

    def __post_init__(self):
        _check_part(self.name, self.zones, self.bins)
        if not 0.0 <= self.floor_frac <= 1.0:
            raise ValueError(f"ensemble: floor_frac {self.floor_frac!r} outside [0, 1]")
        if not self.tol >= 0.0:
            raise ValueError(f"ensemble: tol {self.tol!r} is negative or not a number")


@dataclasses.dataclass(frozen=True)
class Summary:
    """mcs_ens_summary of one range, and the sample count n of its slot."""
    amax: float
    max_rel: float
    sum_se: float
    sum_abs_mean: float
    sum_rel2: float
    n_selected: int
    n_over: int
    n_nonfinite: int
    argmax: int
    n: int


def summary_of(mean: np.ndarray, m2: np.ndarray, n: int, floor_frac: float, tol: float) -> Summary:
    """The definition of the module docstring on the host, for the words of one range; the three sums correctly rounded."""
    mean, m2 = np.asarray(mean, dtype=np.float64).ravel(), np.asarray(m2, dtype=np.float64).ravel()
    finite = np.isfinite(mean) & np.isfinite(m2)
    a = np.abs(mean)
    amax = float(a[finite].max()) if finite.any() else 0.0
    where = np.flatnonzero(finite & (a > 0.0) & (a >= floor_frac * amax))
    n_nonfinite = int(mean.size - np.count_nonzero(finite))
    if where.size == 0:
        return Summary(amax, 0.0, 0.0, 0.0, 0.0, 0, 0, n_nonfinite, -1, int(n))
    se = np.sqrt(m2[where] / (float(n) * float(n - 1)))
    rel = se / a[where]
    k = int(np.argmax(rel))            # (the first of equal maxima)
    return Summary(amax, float(rel[k]), math.fsum(se), math.fsum(a[where]), math.fsum(rel * rel), int(where.size),
                   int(np.count_nonzero(rel > tol)), n_nonfinite, int(where[k]), int(n))


class Trigger:
    """A stop rule on the error bars of one part of a slot (driver.run(triggers=...)): met when its value is <= threshold.
      "max"            max_rel: the largest relative standard error of a selected word
      "rms"            sqrt(sum_rel2 / n_selected)
      "weighted"       sum_se / sum_abs_mean
      "fraction_over"  n_over / n_selected: the share of the selected words whose relative error exceeds tol
    Selected: the words of at least floor_frac times the part's largest |mean| (module docstring).  zones = (z_lo, z_hi): those zones
    of a part whose first axis is the zone index; bins = (l_lo, l_hi): those bins of the single zone zones = (z, z + 1) of a part of
    shape [zone][bins] (the dNdp_* parts of a products slot, the marginals).  Never met while the slot has fewer than two samples, nothing is selected or a
    word of the range is not finite.  predicted_samples: for the three error statistics, the count at which the value would reach the
    threshold if it goes on falling as 1 / sqrt(n): ceil(n (value / threshold)^2); a report, nothing acts on it.
    Refused here: an unknown statistic, threshold <= 0, "fraction_over" without tol, a negative slot, a name no slot has, a zone
    slice on a part without a zone axis, bins without a single zone or on a part without a bins axis.  Whether `slot` is a species slot or the iteration slot only an ensemble knows:
    Ensemble.check_trigger, which driver.run calls before the first iteration, refuses a name the slot does not have."""

    def __init__(self, slot: int, name: str, statistic: str, threshold: float, zones=None, floor_frac: float = 1e-3, tol: Optional[float] = None,
                 bins=None):
        if statistic not in STATISTICS:
            raise ValueError(f"trigger: unknown statistic {statistic!r}; there are: {', '.join(STATISTICS)}")
        if not threshold > 0:
            raise ValueError(f"trigger: threshold {threshold!r} must be positive")
        if statistic == "fraction_over" and tol is None:
            raise ValueError("trigger: 'fraction_over' needs tol, the relative error a word may have")
        if int(slot) != slot or slot < 0:
            raise ValueError(f"trigger: slot {slot!r} is no slot")
        self.request = Request(name, None if zones is None else (int(zones[0]), int(zones[1])), float(floor_frac), 0.0 if tol is None else float(tol),
                               None if bins is None else (int(bins[0]), int(bins[1])))
        self.slot, self.name, self.statistic, self.threshold = int(slot), name, statistic, float(threshold)
        self.zones, self.floor_frac, self.tol, self.bins = self.request.zones, self.request.floor_frac, tol, self.request.bins

    def __repr__(self):
        return (f"Trigger(slot={self.slot}, name={self.name!r}, statistic={self.statistic!r}, threshold={self.threshold!r}, zones={self.zones!r}, "
                f"floor_frac={self.floor_frac!r}, tol={self.tol!r}, bins={self.bins!r})")

    def value(self, s: Summary) -> float:
        """The statistic of a summary; nan where it has none (fewer than two samples, nothing selected)."""
        if s.n < 2 or s.n_selected == 0:
            return float("nan")
        if self.statistic == "max":
            return s.max_rel
        if self.statistic == "rms":
            return math.sqrt(s.sum_rel2 / s.n_selected)
        if self.statistic == "weighted":
            return s.sum_se / s.sum_abs_mean
        return s.n_over / s.n_selected

    def met(self, s: Summary) -> bool:
        return s.n >= 2 and s.n_selected > 0 and s.n_nonfinite == 0 and self.value(s) <= self.threshold

    def predicted_samples(self, s: Summary) -> Optional[int]:
        """None for "fraction_over" (no 1 / sqrt(n) law) and where there is no finite value."""
        v = self.value(s)
        if self.statistic == "fraction_over" or not math.isfinite(v):
            return None
        return int(math.ceil(s.n * (v / self.threshold) ** 2))


AGREEMENT_STATISTICS = ("max_z", "chi2_per_word", "fraction_over", "mean_z", "weighted_diff")


@dataclasses.dataclass(frozen=True)
class CompareRequest:
    """One range of a comparison (`Ensemble.compare`): a named part, a zone slice or a bins window of it as in `Request`, the
    floor of the selection and the |z| above which a word counts in n_over."""
    name: str
    zones: Optional[Tuple[int, int]] = None
    floor_frac: float = 1e-3
    zcut: float = 3.0
    bins: Optional[Tuple[int, int]] = None

    def __post_init__(self):
        _check_part(self.name, self.zones, self.bins)
        if not 0.0 <= self.floor_frac <= 1.0:
            raise ValueError(f"ensemble: floor_frac {self.floor_frac!r} outside [0, 1]")
        if not self.zcut >= 0.0:
            raise ValueError(f"ensemble: zcut {self.zcut!r} is negative or not a number")


@dataclasses.dataclass(frozen=True)
class Difference:
    """mcs_ens_difference of one range, and the sample counts n_a, n_b of the two slots."""
    amax: float
    max_abs_z: float
    sum_z: float
    sum_abs_z: float
    sum_z2: float
    sum_abs_diff: float
    sum_scale: float
    n_selected: int
    n_over: int
    n_nonfinite: int
    n_degenerate: int
    argmax: int
    n_a: int
    n_b: int


def difference_of(ma, qa, n_a: int, mb, qb, n_b: int, floor_frac: float, zcut: float) -> Difference:
    """The definition of mcs_ens_compare (include/mcs.h) on the host, for the words of one range of A (mean ma, M2 qa, n_a samples)
    and B: the per-word quantities elementwise, the five sums correctly rounded."""
    ma, qa, mb, qb = (np.asarray(x, dtype=np.float64).ravel() for x in (ma, qa, mb, qb))
    with np.errstate(all="ignore"):
        s2 = qa / (float(n_a) * float(n_a - 1)) + qb / (float(n_b) * float(n_b - 1))
        d = ma - mb
        scale = np.maximum(np.abs(ma), np.abs(mb))
        finite = np.isfinite(ma) & np.isfinite(qa) & np.isfinite(mb) & np.isfinite(qb) & np.isfinite(d) & np.isfinite(s2)
    n_nonfinite = int(ma.size - np.count_nonzero(finite))
    amax = float(scale[finite].max()) if finite.any() else 0.0
    where = np.flatnonzero(finite & (scale > 0.0) & (scale >= floor_frac * amax))
    if where.size == 0:
        return Difference(amax, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, n_nonfinite, 0, -1, int(n_a), int(n_b))
    d, s2, scale = d[where], s2[where], scale[where]
    keep = ~((s2 == 0.0) & (d != 0.0))                # (the others are degenerate)
    some = s2[keep] != 0.0
    z = np.zeros(int(np.count_nonzero(keep)))         # (s2 == 0 and d == 0: z = 0)
    with np.errstate(all="ignore"):
        z[some] = d[keep][some] / np.sqrt(s2[keep][some])
    az = np.abs(z)
    k = int(np.argmax(az)) if az.size else -1         # (the first of equal maxima)
    return Difference(amax, float(az[k]) if az.size else 0.0, math.fsum(z), math.fsum(az), math.fsum(z * z), math.fsum(np.abs(d)),
                      math.fsum(scale), int(where.size), int(np.count_nonzero(az > zcut)), n_nonfinite,
                      int(where.size - np.count_nonzero(keep)), int(where[keep][k]) if az.size else -1, int(n_a), int(n_b))


class Agreement:
    """A rule on the difference of one part of two slots (`check_agreements`): met when its value is <= threshold.
      "max_z"          max_abs_z: the largest |z| of a selected word
      "chi2_per_word"  sum_z2 / (n_selected - n_degenerate)
      "fraction_over"  n_over / (n_selected - n_degenerate): the share of the words with |z| > zcut
      "mean_z"         sum_z / (n_selected - n_degenerate); met when its absolute value is <= threshold (a bias has a sign)
      "weighted_diff"  sum_abs_diff / sum_scale
    z = (mean_a - mean_b) / sqrt(se_a^2 + se_b^2) per word, over the selected words: those whose larger |mean| is at least floor_frac
    times the part's largest (mcs_ens_compare of include/mcs.h has the definition).  A degenerate word has no z: both error bars are
    zero and the means differ.  Never met with nothing selected, with a word of the range that is not finite, or with a degenerate
    word -- except "weighted_diff", which counts degenerate words like any other.

    What the numbers mean: with few samples z follows Welch's t and not a normal law.  Under the null hypothesis
    E[z^2] = nu / (nu - 2) with nu between min(n_a, n_b) - 1 and n_a + n_b - 2: with three samples a side, chi2_per_word of a
    perfectly good pair lies near 2 and not near 1, and |z| > 3 is nothing rare.  A threshold is therefore best calibrated on a null
    pair: two runs of the same configuration over different iteration numbers (driver.run(first_iter=...))."""

    def __init__(self, slot: int, name: str, statistic: str, threshold: float, zones=None, bins=None, floor_frac: float = 1e-3, zcut: float = 3.0,
                 other_slot: Optional[int] = None):
        if statistic not in AGREEMENT_STATISTICS:
            raise ValueError(f"agreement: unknown statistic {statistic!r}; there are: {', '.join(AGREEMENT_STATISTICS)}")
        if not threshold > 0:
            raise ValueError(f"agreement: threshold {threshold!r} must be positive")
        for s in (slot,) if other_slot is None else (slot, other_slot):
            if int(s) != s or s < 0:
                raise ValueError(f"agreement: slot {s!r} is no slot")
        self.request = CompareRequest(name, None if zones is None else (int(zones[0]), int(zones[1])), float(floor_frac), float(zcut),
                                      None if bins is None else (int(bins[0]), int(bins[1])))
        self.slot, self.other_slot = int(slot), int(slot if other_slot is None else other_slot)
        self.name, self.statistic, self.threshold = name, statistic, float(threshold)
        self.zones, self.bins, self.floor_frac, self.zcut = self.request.zones, self.request.bins, self.request.floor_frac, self.request.zcut

    def __repr__(self):
        return (f"Agreement(slot={self.slot}, name={self.name!r}, statistic={self.statistic!r}, threshold={self.threshold!r}, zones={self.zones!r}, "
                f"bins={self.bins!r}, floor_frac={self.floor_frac!r}, zcut={self.zcut!r}, other_slot={self.other_slot})")

    def value(self, d: Difference) -> float:
        """The statistic of a difference; nan where it has none (no selected word, or none that is not degenerate)."""
        if self.statistic == "weighted_diff":
            return d.sum_abs_diff / d.sum_scale if d.n_selected > 0 else float("nan")
        n = d.n_selected - d.n_degenerate
        if n <= 0:
            return float("nan")
        if self.statistic == "max_z":
            return d.max_abs_z
        if self.statistic == "chi2_per_word":
            return d.sum_z2 / n
        if self.statistic == "fraction_over":
            return d.n_over / n
        return d.sum_z / n

    def met(self, d: Difference) -> bool:
        if d.n_selected == 0 or d.n_nonfinite > 0 or (d.n_degenerate > 0 and self.statistic != "weighted_diff"):
            return False
        return abs(self.value(d)) <= self.threshold


@dataclasses.dataclass
class AgreementCheck:
    """One row of `check_agreements`, the counterpart of driver.TriggerCheck."""
    agreement: Agreement
    difference: Difference
    value: float
    met: bool


def check_agreements(a: "Ensemble", b: "Ensemble", agreements: Sequence[Agreement]) -> List[AgreementCheck]:
    """One `a.compare(b, ...)` per (slot, other_slot) pair that has agreements -> a row per agreement, in their order."""
    agreements = list(agreements)
    rows: List[Optional[AgreementCheck]] = [None] * len(agreements)
    for slot, other_slot in sorted({(t.slot, t.other_slot) for t in agreements}):
        mine = [k for k, t in enumerate(agreements) if (t.slot, t.other_slot) == (slot, other_slot)]
        got = a.compare(b, slot, [agreements[k].request for k in mine], other_slot)
        for k, d in zip(mine, got):
            rows[k] = AgreementCheck(agreements[k], d, agreements[k].value(d), agreements[k].met(d))
    return rows


def bin_centres_log10(prob) -> np.ndarray:
    """x_log [nmom+1] of `Ensemble.set_slope_window`: log10 of every momentum bin's centre in cgs, the centre 0.5 (b[l] + b[l + 1])
    of prob.psd_mom_bounds (log10 of p / m_p c) brought to cgs as consumers.consumer_tables does (pt_center)."""
    from .constants import C, MP
    mb = np.asarray(prob.psd_mom_bounds, dtype=np.float64)
    return np.ascontiguousarray(np.log10(10.0 ** (0.5 * (mb[:-1] + mb[1:])) * (MP * C)))


def slope_window(prob, p_lo: float, p_hi: float):
    """(l_lo, l_hi, x_log), the arguments of `Ensemble.set_slope_window`, from the problem's momentum bins and two momenta in cgs:
    x_log[l] = log10 of the centre of bin l in cgs, the centre 0.5 (b[l] + b[l + 1]) of prob.psd_mom_bounds brought to cgs as
    consumers.consumer_tables does (pt_center), and the window the bins whose centre lies in [p_lo, p_hi]."""
    x_log = bin_centres_log10(prob)
    if not 0 < p_lo < p_hi:
        raise ValueError(f"ensemble: slope window needs momenta 0 < p_lo < p_hi, not {p_lo!r}, {p_hi!r}")
    inside = np.flatnonzero((x_log >= math.log10(p_lo)) & (x_log <= math.log10(p_hi)))
    if inside.size < 3:
        raise ValueError(f"ensemble: fewer than three momentum bins have their centre in [{p_lo!r}, {p_hi!r}]")
    return int(inside[0]), int(inside[-1]) + 1, x_log


def _det_log10(backend):
    """The deterministic log10 of include/mcs_math.h as the backend evaluates it: a -> log10(a), elementwise."""
    if hasattr(backend, "eval_fn"):
        return lambda a: backend.eval_fn("log10", a)
    lib = getattr(backend, "lib", None)
    if lib is not None and hasattr(lib, "orc_eval_fn"):
        def log10(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            out = np.zeros_like(a)
            if lib.orc_eval_fn(capi.FN["log10"], a.size, a.ctypes.data_as(capi.c_double_p), a.ctypes.data_as(capi.c_double_p),
                               out.ctypes.data_as(capi.c_double_p)) != 0:
                raise RuntimeError("ensemble: the backend's log10 failed")
            return out
        return log10
    raise ValueError("ensemble: the backend evaluates no deterministic log10 (eval_fn); a products sample needs it for the slopes")


def slopes_of(dndp: np.ndarray, l_lo: int, l_hi: int, x_log: np.ndarray, log10) -> np.ndarray:
    """The slope definition of the module docstring for every row of dndp [...][nmom+2] -> [...]."""
    d = np.asarray(dndp, dtype=np.float64)
    rows = d.reshape(-1, d.shape[-1])[:, l_lo:l_hi]
    valid = rows > DNDP_FLOOR
    y = np.zeros_like(rows)
    y[valid] = log10(np.ascontiguousarray(rows[valid]))
    return slopes_xy(np.asarray(x_log, dtype=np.float64)[l_lo:l_hi], y, valid).reshape(d.shape[:-1])


def slopes_xy(x: np.ndarray, y: np.ndarray, valid: np.ndarray) -> np.ndarray:
    """The least-squares slope rule of the module docstring for every row of y [rows][n] against x [n] over the entries that
    valid [rows][n] admits -> [rows]: the rows side by side in numpy, the entries of a row one after the other, so that every sum is
    the serial one.  Fewer than three valid entries: NaN."""
    rows = np.asarray(y, dtype=np.float64)
    valid = np.asarray(valid, dtype=bool)
    y = np.where(valid, rows, 0.0)
    x = np.asarray(x, dtype=np.float64)
    k = valid.sum(axis=1).astype(np.float64)
    sx, sy = np.zeros(len(rows)), np.zeros(len(rows))
    for l in range(rows.shape[1]):
        sx = np.where(valid[:, l], sx + x[l], sx)
        sy = np.where(valid[:, l], sy + y[:, l], sy)
    with np.errstate(divide="ignore", invalid="ignore"):
        xbar, ybar = sx / k, sy / k
        sxx, sxy = np.zeros(len(rows)), np.zeros(len(rows))
        for l in range(rows.shape[1]):
            dx = x[l] - xbar
            sxx = np.where(valid[:, l], sxx + dx * dx, sxx)
            sxy = np.where(valid[:, l], sxy + dx * (y[:, l] - ybar), sxy)
        slope = np.where(k >= 3, sxy / sxx, np.nan)
    return slope


def check_angle_windows(nmom: int, l_lo, l_hi) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """The momentum windows of mcs_angle_dist as two tuples of ints, or the ValueError that says which rule they break: 1..8 windows,
    0 <= l_lo < l_hi <= nmom + 1."""
    lo, hi = list(l_lo), list(l_hi)
    if len(lo) != len(hi) or not 1 <= len(lo) <= ANGLE_MAX_WINDOWS:
        raise ValueError(f"ensemble: 1..{ANGLE_MAX_WINDOWS} angle windows, each with its l_lo and l_hi, not {len(lo)} and {len(hi)}")
    for a, b in zip(lo, hi):
        if int(a) != a or int(b) != b or not 0 <= a < b <= nmom + 1:
            raise ValueError(f"ensemble: angle window ({a}, {b}) needs integers 0 <= l_lo < l_hi <= {nmom + 1}")
    return tuple(int(a) for a in lo), tuple(int(b) for b in hi)


class Ensemble:
    """What both kinds have in common: the slots, the named views of a slot's vectors."""

    def __init__(self, P: capi.McsParams, n_species: int):
        self.layout = EnsLayout(P)
        self.n_species = int(n_species)
        self.iteration_slot = self.n_species
        self.i_shock = int(P.i_shock)      # the last upstream zone (profile_consistency)
        # run_overlapped(ensemble=True): mean / standard error / count over the iterations of ion_finalize's FINALIZE_NAMES
        self.finalize_mean: Dict[str, np.ndarray] = {}
        self.finalize_stderr: Dict[str, np.ndarray] = {}
        self.finalize_count = 0
        self.window = None             # (l_lo, l_hi, x_log) of set_slope_window
        self.photon_layout = None      # consumers.PhotonLayout of set_photon_layout
        self.angle_windows = None      # ((l_lo, ...), (l_hi, ...)) of set_angle_windows
        self.tcuts_n = None            # the number of time cuts of the tcuts samples, fixed by the first
        self.profile_settings = None   # ProfileIn.settings() of the first profile sample, fixed by it
        self.detectors_settings = None # DetectorSpectra.settings() of the first detectors sample, fixed by it: (nd, l_lo, l_hi, x_unit, x_spec)
        self._deposited: List[int] = []      # species slots deposited since the last add_photons_all, in deposit order

    @staticmethod
    def for_backend(backend, n_species: int) -> "Ensemble":
        """A device accumulator beside a HIP context, the numpy one for every other backend."""
        if isinstance(backend, HipBackend):
            return HipEnsemble(backend, n_species)
        return HostEnsemble(backend.P, n_species)

    def products_slot(self, s: int) -> int:
        """The slot number of the products of species slot s (MCS_ENS_PRODUCTS)."""
        if not 0 <= s < self.n_species:
            raise ValueError(f"ensemble: slot {s} is no species slot (0..{self.n_species - 1}); only a species slot has a products slot")
        return int(s) | PRODUCTS_BIT

    @staticmethod
    def is_products(slot: int) -> bool:
        return slot >= 0 and bool(slot & PRODUCTS_BIT)

    def photons_slot(self, s: int) -> int:
        """The slot number of the photon spectra of species slot s (MCS_ENS_PHOTONS)."""
        if not 0 <= s < self.n_species:
            raise ValueError(f"ensemble: slot {s} is no species slot (0..{self.n_species - 1}); only a species slot has a photons slot")
        return int(s) | PHOTONS_BIT

    @staticmethod
    def is_photons(slot: int) -> bool:
        return slot >= 0 and not slot & PRODUCTS_BIT and bool(slot & PHOTONS_BIT)

    def escape_slot(self, s: int) -> int:
        """The slot number of the escape spectra of species slot s (MCS_ENS_ESCAPE)."""
        if not 0 <= s < self.n_species:
            raise ValueError(f"ensemble: slot {s} is no species slot (0..{self.n_species - 1}); only a species slot has an escape slot")
        return int(s) | ESCAPE_BIT

    @staticmethod
    def is_escape(slot: int) -> bool:
        return slot >= 0 and slot != PHOTONS_ALL and not slot & (PRODUCTS_BIT | PHOTONS_BIT) and bool(slot & ESCAPE_BIT)

    @staticmethod
    def escape_row(door: int, frame: int) -> Tuple[int, int]:
        """zones= of one door (0: upstream, 1: downstream) and frame (0: shock, 1: the door's plasma frame, 2: ISM) of an escape
        slot's parts: the row 3 * door + frame."""
        if door not in (0, 1) or frame not in (0, 1, 2):
            raise ValueError(f"ensemble: an escape slot has doors 0, 1 and frames 0, 1, 2, not door {door!r}, frame {frame!r}")
        return 3 * door + frame, 3 * door + frame + 1

    def angles_slot(self, s: int) -> int:
        """The slot number of the pitch-angle distributions of species slot s (MCS_ENS_ANGLES)."""
        if not 0 <= s < self.n_species:
            raise ValueError(f"ensemble: slot {s} is no species slot (0..{self.n_species - 1}); only a species slot has an angles slot")
        return int(s) | ANGLES_BIT

    @staticmethod
    def is_angles(slot: int) -> bool:
        return slot >= 0 and slot != PHOTONS_ALL and not slot & (PRODUCTS_BIT | PHOTONS_BIT | ESCAPE_BIT) and bool(slot & ANGLES_BIT)

    def angles_row(self, frame: int, zone: int, window: int) -> Tuple[int, int]:
        """zones= of one frame (0: shock, 1: the zone's plasma frame, 2: ISM), grid zone (0-based) and momentum window of an angles
        slot's parts: the row (frame * n_grid + zone) * n_win + window."""
        if self.angle_windows is None:
            raise ValueError("ensemble: no angle windows (set_angle_windows)")
        ng, n_win = self.layout.tally.n_grid, len(self.angle_windows[0])
        if frame not in (0, 1, 2) or not 0 <= zone < ng or not 0 <= window < n_win or int(zone) != zone or int(window) != window:
            raise ValueError(f"ensemble: an angles slot has frames 0, 1, 2, zones 0..{ng - 1} and windows 0..{n_win - 1}, not frame {frame!r}, "
                             f"zone {zone!r}, window {window!r}")
        r = (int(frame) * ng + int(zone)) * n_win + int(window)
        return r, r + 1

    def set_angle_windows(self, l_lo, l_hi):
        """The momentum windows l_lo[m] <= k < l_hi[m] of the angles samples (consumers.momentum_windows builds them; the rules of
        mcs_angle_dist: 1..8 windows, 0 <= l_lo < l_hi <= nmom + 1, they may overlap).  May be repeated until the first angles sample;
        refused afterwards."""
        lo, hi = check_angle_windows(self.layout.tally.shapes["psd"][2] - 2, l_lo, l_hi)
        self._set_angle_windows(lo, hi)
        self.angle_windows = (lo, hi)

    def has_angle_windows(self) -> bool:
        return self.angle_windows is not None

    @staticmethod
    def _angle_windows_differ(a, b) -> bool:
        return a.angle_windows is not None and b.angle_windows is not None and a.angle_windows != b.angle_windows

    def tcuts_slot(self, s: int) -> int:
        """The slot number of the time-cut spectra of species slot s (MCS_ENS_TCUTS)."""
        if not 0 <= s < self.n_species:
            raise ValueError(f"ensemble: slot {s} is no species slot (0..{self.n_species - 1}); only a species slot has a tcuts slot")
        return int(s) | TCUTS_BIT

    @staticmethod
    def is_tcuts(slot: int) -> bool:
        return (slot >= 0 and slot != PHOTONS_ALL and not slot & (PRODUCTS_BIT | PHOTONS_BIT | ESCAPE_BIT | ANGLES_BIT)
                and bool(slot & TCUTS_BIT))

    @staticmethod
    def tcuts_row(k: int) -> Tuple[int, int]:
        """zones= of time cut k (0-based) of a tcuts slot's spectrum, weight, number and mean_log_p; bins= of cut k of a quantile."""
        if int(k) != k or k < 0:
            raise ValueError(f"ensemble: a time cut is an index 0, 1, ..., not {k!r}")
        return int(k), int(k) + 1

    def expect_tcuts(self, n_tcuts: int):
        """The number of time cuts the tcuts samples will have, so that requests and triggers can name their parts before the first
        sample arrives (which fixes it for good).  Refused where the ensemble's tcuts samples have another."""
        if self.tcuts_n is not None and self.tcuts_n != int(n_tcuts):
            raise ValueError(f"ensemble: {n_tcuts} time cuts, but the ensemble's tcuts samples have {self.tcuts_n}")
        if not 1 <= int(n_tcuts) <= 99:
            raise ValueError(f"ensemble: a tcuts sample has 1..99 time cuts, not {n_tcuts!r}")
        self.tcuts_n = int(n_tcuts)

    @staticmethod
    def _tcuts_differ(a, b) -> bool:
        return a.tcuts_n is not None and b.tcuts_n is not None and a.tcuts_n != b.tcuts_n

    def detectors_slot(self, s: int) -> int:
        """The slot number of the detector spectra of species slot s (MCS_ENS_DETECTORS)."""
        if not 0 <= s < self.n_species:
            raise ValueError(f"ensemble: slot {s} is no species slot (0..{self.n_species - 1}); only a species slot has a detectors slot")
        return int(s) | DETECTORS_BIT

    @staticmethod
    def is_detectors(slot: int) -> bool:
        return (slot >= 0 and slot != PHOTONS_ALL and not slot & (PRODUCTS_BIT | PHOTONS_BIT | ESCAPE_BIT | ANGLES_BIT | TCUTS_BIT | PROFILE_SLOT)
                and bool(slot & DETECTORS_BIT))

    def detectors_row(self, frame: int, d: int) -> Tuple[int, int]:
        """zones= of frame (0: shock, 1: plasma) and detector d (0-based) of a detectors slot's spectrum, dndp, number, mean_log_p and
        slope; bins= of that row of a quantile: the row frame * nd + d."""
        if self.detectors_settings is None:
            raise ValueError("ensemble: the detectors samples have no settings yet (expect_detectors, or the first sample)")
        nd = self.detectors_settings[0]
        if frame not in (0, 1) or int(d) != d or not 0 <= d < nd:
            raise ValueError(f"ensemble: a detectors slot has frames 0, 1 and detectors 0..{nd - 1}, not frame {frame!r}, detector {d!r}")
        r = int(frame) * nd + int(d)
        return r, r + 1

    def expect_detectors(self, settings):
        """The settings the detectors samples will have -- DetectorSpectra.settings(): (nd, l_lo, l_hi, the bits of x_unit, the bits of
        x_spec) -- so that requests and triggers can name their parts before the first sample arrives (which fixes them for good).
        Refused where the ensemble's detectors samples have others."""
        settings = tuple(settings)
        if self.detectors_settings is not None and self.detectors_settings != settings:
            raise ValueError("ensemble: these detector settings (number of detectors, window, x_unit, x_spec) differ from those of the ensemble's "
                             "detectors samples")
        if not 1 <= settings[0] <= self.layout.tally.n_grid:
            raise ValueError(f"ensemble: a detectors sample has 1..{self.layout.tally.n_grid} detectors, not {settings[0]!r}")
        self.detectors_settings = settings

    @staticmethod
    def _detectors_differ(a, b) -> bool:
        return a.detectors_settings is not None and b.detectors_settings is not None and a.detectors_settings != b.detectors_settings

    profile_slot = PROFILE_SLOT        # the profile slot, one per ensemble (MCS_ENS_PROFILE)

    @staticmethod
    def is_profile(slot: int) -> bool:
        return slot == PROFILE_SLOT

    @staticmethod
    def _settings_differ(a, b) -> bool:
        """Two ProfileIn.settings() vectors (or None) that are both there and differ in some bit."""
        return a is not None and b is not None and np.asarray(a, dtype=np.float64).tobytes() != np.asarray(b, dtype=np.float64).tobytes()

    @classmethod
    def _profiles_differ(cls, a, b) -> bool:
        return cls._settings_differ(a.profile_settings, b.profile_settings)

    photons_all_slot = PHOTONS_ALL     # the source slot, one per ensemble (MCS_ENS_PHOTONS_ALL)

    @staticmethod
    def is_photons_all(slot: int) -> bool:
        return slot == PHOTONS_ALL

    @classmethod
    def _has_photon_vector(cls, slot: int) -> bool:
        """A photons slot or the source slot: the sample vector is that of the photon layout."""
        return cls.is_photons(slot) or cls.is_photons_all(slot)

    @property
    def pending_photons(self) -> Tuple[int, ...]:
        """The species slots deposited (add_photons(deposit=True)) since the last add_photons_all, in deposit order."""
        return tuple(self._deposited)

    def set_photon_layout(self, layout):
        """The shells, the energy words of every process and their offsets on the common grid (a consumers.PhotonLayout;
        consumers.stock_photon_layout(n_shells) is that of the stock energy grids).  Before the first photons sample; refused afterwards."""
        from .consumers import PHOTON_PROCESSES
        a = layout.args()
        n_shells, n, start, n_pts = a[0], a[1:4], a[4:7], a[7]
        if not 1 <= n_shells <= 4096 or not 1 <= n_pts <= 65536:
            raise ValueError(f"ensemble: a photon layout needs 1..4096 shells and 1..65536 points on the common grid, not {n_shells} and {n_pts}")
        for p, k, o in zip(PHOTON_PROCESSES, n, start):
            if not (1 <= k <= 255 and 0 <= o and o + k <= n_pts):
                raise ValueError(f"ensemble: {p!r} needs 1..255 energy words inside the common grid, not {k} at {o} of {n_pts}")
        self._set_photon_layout(layout)
        self.photon_layout = layout

    def _decode(self, slot: int) -> Tuple[str, Optional[int]]:
        """(kind, species index) of a slot number -- "species", "iteration", "products", "photons", "source", "escape", "angles", "tcuts", "profile" or "detectors" -- the one place where
        its bits are read; the index is None for the iteration, the source and the profile slot, and not yet checked (`_check_slot`)."""
        if self.is_photons_all(slot):
            return "source", None
        if self.is_profile(slot):
            return "profile", None
        if self.is_products(slot):
            return "products", slot ^ PRODUCTS_BIT
        if self.is_photons(slot):
            return "photons", slot ^ PHOTONS_BIT
        if self.is_escape(slot):
            return "escape", slot ^ ESCAPE_BIT
        if self.is_angles(slot):
            return "angles", slot ^ ANGLES_BIT
        if self.is_tcuts(slot):
            return "tcuts", slot ^ TCUTS_BIT
        if self.is_detectors(slot):
            return "detectors", slot ^ DETECTORS_BIT
        return ("iteration", None) if slot == self.iteration_slot else ("species", slot)

    def _kind(self, slot: int) -> str:
        return self._decode(slot)[0]

    def _describe(self, slot: int) -> str:
        kind, s = self._decode(slot)
        if kind in ("products", "photons", "escape", "angles", "tcuts", "detectors"):
            return f"the {kind} slot of species slot {s}"
        return f"species slot {s}" if kind == "species" else f"the {kind} slot"

    def names(self, slot: int):
        self._check_slot(slot)
        return {"species": SPECIES_NAMES, "iteration": ITERATION_NAMES, "products": PRODUCT_NAMES, "escape": ESCAPE_NAMES,
                "angles": ANGLES_NAMES, "tcuts": TCUTS_NAMES, "profile": PROFILE_NAMES, "detectors": DETECTORS_NAMES}.get(self._kind(slot), PHOTON_NAMES)

    def _check_slot(self, slot: int):
        kind, s = self._decode(slot)
        if kind in ("products", "photons", "escape", "angles", "tcuts", "detectors") and not 0 <= s < self.n_species:
            raise ValueError(f"ensemble: {kind} slot of slot {s}, which is no species slot (0..{self.n_species - 1})")
        if kind == "species" and not 0 <= s < self.n_species:
            raise ValueError(f"ensemble: slot {slot} outside 0..{self.n_species}")

    def _len(self, slot: int) -> int:
        kind = self._kind(slot)
        if kind in ("photons", "source"):
            return 0 if self.photon_layout is None else self.photon_layout.offsets()["_total"]
        if kind == "angles":
            return 0 if self.angle_windows is None else self.layout.angles_fields(len(self.angle_windows[0]))["total"]
        if kind == "tcuts":
            return 0 if self.tcuts_n is None else self.layout.tcuts_fields(self.tcuts_n)["total"]
        if kind == "profile":
            return self.layout.profile_fields()["total"]
        if kind == "detectors":
            return 0 if self.detectors_settings is None else self.layout.detectors_fields(self.detectors_settings[0])["total"]
        return {"species": self.layout.species_total, "iteration": self.layout.iteration_total, "products": self.layout.products_total,
                "escape": self.layout.escape_total}[kind]

    def _where(self, slot: int, name: str):
        self._check_slot(slot)
        kind = self._kind(slot)
        if kind in ("photons", "source"):
            if self.photon_layout is None:
                raise ValueError(f"ensemble: {self._describe(slot)} has no layout yet (set_photon_layout)")
            rows = self.photon_layout.rows
            offs = self.photon_layout.offsets()
            table = {part: (offs[part][0], (rows, offs[part][1])) for part in PHOTON_NAMES}
        elif kind == "angles":
            if self.angle_windows is None:
                raise ValueError(f"ensemble: {self._describe(slot)} has no windows yet (set_angle_windows)")
            table = self.layout.angles(len(self.angle_windows[0]))
        elif kind == "tcuts":
            if self.tcuts_n is None:
                raise ValueError(f"ensemble: {self._describe(slot)} has taken no sample yet (its first fixes the number of time cuts)")
            table = self.layout.tcuts(self.tcuts_n)
        elif kind == "profile":
            table = self.layout.profile()
        elif kind == "detectors":
            if self.detectors_settings is None:
                raise ValueError(f"ensemble: {self._describe(slot)} has taken no sample yet (its first fixes the detectors and the window)")
            table = self.layout.detectors(self.detectors_settings[0])
        else:
            table = {"species": self.layout.species, "iteration": self.layout.iteration, "products": self.layout.products,
                     "escape": self.layout.escape}[kind]
        if name not in self.names(slot):
            raise KeyError(f"ensemble: {self._describe(slot)} has no {name!r}; it has: {', '.join(self.names(slot))}")
        return table[name]

    def _named(self, slot: int, what: int, name: str) -> np.ndarray:
        off, shape = self._where(slot, name)
        return self._read(slot, what, off, int(np.prod(shape))).reshape(shape)

    def mean(self, slot: int, name: str) -> np.ndarray:
        return self._named(slot, 0, name)

    def m2(self, slot: int, name: str) -> np.ndarray:
        """The sum of squared deviations from the mean."""
        return self._named(slot, 1, name)

    def stderr(self, slot: int, name: str) -> np.ndarray:
        """The standard error of the mean, sqrt(M2 / (n (n - 1))); refused below two samples."""
        return self._named(slot, 2, name)

    def word_range(self, slot: int, name: str, zones=None, bins=None) -> Tuple[int, int]:
        """(first, count) of a part of the slot's sample vector, of its zones [z_lo, z_hi), or of the bins [l_lo, l_hi) of its one
        zone zones = (z, z + 1)."""
        off, shape = self._where(slot, name)
        _check_part(name, zones, bins)
        n = int(np.prod(shape))
        if zones is None:
            return off, n
        z_lo, z_hi = int(zones[0]), int(zones[1])
        if not 0 <= z_lo <= z_hi <= shape[0]:
            raise ValueError(f"ensemble: zones ({z_lo}, {z_hi}) outside 0..{shape[0]} of {name!r}")
        per = n // shape[0]
        if bins is None:
            return off + z_lo * per, (z_hi - z_lo) * per
        l_lo, l_hi = int(bins[0]), int(bins[1])
        if not 0 <= l_lo <= l_hi <= per:
            raise ValueError(f"ensemble: bins ({l_lo}, {l_hi}) outside 0..{per} of {name!r}")
        return off + z_lo * per + l_lo, l_hi - l_lo

    def summarize(self, slot: int, requests: Sequence[Request]) -> List[Summary]:
        """One Summary per request (at most MAX_RANGES; they may overlap), in one pass over the slot: on the device one
        mcs_ens_summarize call and one wait.  Refused below two samples."""
        requests = list(requests)
        self._check_slot(slot)
        if len(requests) > MAX_RANGES:
            raise ValueError(f"ensemble: {len(requests)} requests in one summary; at most {MAX_RANGES}")
        ranges = [self.word_range(slot, q.name, q.zones, q.bins) + (float(q.floor_frac), float(q.tol)) for q in requests]
        n = self.count(slot)
        if n < 2:
            raise ValueError(f"ensemble: a summary needs at least two samples; slot {slot} has {n}")
        return self._summarize(slot, n, ranges) if ranges else []

    def summarize_merged(self, others: Sequence["Ensemble"], slot: int, requests: Sequence[Request]) -> List[Summary]:
        """`summarize` of this ensemble merged with `others` in that order (at most MAX_MERGED in all, of this kind, slots and
        layout, each once), none of them changed: Summary.n is the total count, which must be at least two.  On the device one
        mcs_ens_summarize_merged call and one wait; bit for bit what merging them in that order into an empty ensemble and
        summarising it gives.  summarize_merged([], ...) is summarize(...)."""
        others, requests = list(others), list(requests)
        if not others:
            return self.summarize(slot, requests)
        self._check_slot(slot)
        self._check_merged(others)
        if len(requests) > MAX_RANGES:
            raise ValueError(f"ensemble: {len(requests)} requests in one summary; at most {MAX_RANGES}")
        ranges = [self.word_range(slot, q.name, q.zones, q.bins) + (float(q.floor_frac), float(q.tol)) for q in requests]
        n = self.count(slot) + sum(o.count(slot) for o in others)
        if n < 2:
            raise ValueError(f"ensemble: a summary needs at least two samples; slot {slot} has {n} over the {1 + len(others)} ensembles")
        return self._summarize_merged(others, slot, n, ranges) if ranges else []

    def _check_merged(self, others):
        if 1 + len(others) > MAX_MERGED:
            raise ValueError(f"ensemble: a merged summary of {1 + len(others)} ensembles; at most {MAX_MERGED}")
        if len({id(e) for e in [self] + others}) != 1 + len(others):
            raise ValueError("ensemble: a merged summary takes every ensemble once")
        for o in others:
            if type(o) is not type(self) or o.n_species != self.n_species or o.layout.fields != self.layout.fields:
                raise ValueError("ensemble: a merged summary needs ensembles of the same kind, slots and layout")

    def compare(self, other: "Ensemble", slot: int, requests: Sequence[CompareRequest], other_slot: Optional[int] = None) -> List[Difference]:
        """One Difference per request (at most MAX_RANGES; they may overlap): slot `slot` of this ensemble, A, against slot
        `other_slot` (default: the same number) of `other`, B -- two slots of one kind of ensembles of one kind and layout, each with
        at least two samples; `other` may be this ensemble when the slots differ.  Neither is changed.  On the device one
        mcs_ens_compare call and one wait (include/mcs.h has the definition; `Agreement` says what the numbers mean)."""
        requests = list(requests)
        other_slot = slot if other_slot is None else other_slot
        if type(other) is not type(self) or other.layout.fields != self.layout.fields:
            raise ValueError("ensemble: a comparison needs ensembles of the same kind and layout")
        self._check_slot(slot)
        other._check_slot(other_slot)
        if other is self and slot == other_slot:
            raise ValueError(f"ensemble: a comparison of slot {slot} with itself")
        if self._kind(slot) != other._kind(other_slot):
            raise ValueError(f"ensemble: a comparison of a {self._kind(slot)} slot with a {other._kind(other_slot)} slot")
        if len(requests) > MAX_RANGES:
            raise ValueError(f"ensemble: {len(requests)} requests in one comparison; at most {MAX_RANGES}")
        ranges = [self.word_range(slot, q.name, q.zones, q.bins) + (float(q.floor_frac), float(q.zcut)) for q in requests]
        n_a, n_b = self.count(slot), other.count(other_slot)
        if n_a < 2 or n_b < 2:
            raise ValueError(f"ensemble: a comparison needs at least two samples on either side; slot {slot} has {n_a}, the other's slot {other_slot} has {n_b}")
        return self._compare(other, slot, other_slot, n_a, n_b, ranges) if ranges else []

    def check_trigger(self, trigger: Trigger):
        """Refuses a trigger whose slot this ensemble does not have, or whose part (or zone slice, or bins window) that slot does
        not have."""
        self.word_range(trigger.slot, trigger.name, trigger.zones, trigger.bins)

    def set_slope_window(self, l_lo: int, l_hi: int, x_log):
        """The bins l_lo <= l < l_hi over which the slopes of a products sample are fitted, and x_log [nmom+1], the log10 of every
        momentum bin's centre (`slope_window` builds both).  Before the first products sample; refused afterwards."""
        nx = self.layout.tally.shapes["psd"][2] - 1
        x_log = np.ascontiguousarray(x_log, dtype=np.float64)
        if x_log.shape != (nx,):
            raise ValueError(f"ensemble: x_log has shape {x_log.shape}; it holds the {nx} bin centres")
        if int(l_lo) != l_lo or int(l_hi) != l_hi or not (0 <= l_lo and l_hi <= nx and l_hi - l_lo >= 3):
            raise ValueError(f"ensemble: slope window ({l_lo}, {l_hi}) needs 0 <= l_lo, l_hi <= {nx} and at least three bins")
        if not np.all(np.isfinite(x_log)):
            raise ValueError("ensemble: x_log is not finite")
        self._set_slope_window(int(l_lo), int(l_hi), x_log)
        self.window = (int(l_lo), int(l_hi), x_log.copy())

    def has_slope_window(self) -> bool:
        return self.window is not None

    def destroy(self):
        pass


class HostEnsemble(Ensemble):
    """The arithmetic of the device accumulator in numpy, word for word, on read_tallies() buffers."""

    def __init__(self, P: capi.McsParams, n_species: int):
        super().__init__(P, n_species)
        # slot number -> _Slot: the species and the iteration slots from the start; a products, photons or source slot from its first
        # sample or merge on (absent: never sampled)
        self._slots: Dict[int, _Slot] = {s: _Slot(self._len(s)) for s in range(self.n_species + 1)}
        self._snapshot = None          # (backend, words [esc_flux, energy_recv_pool))
        self._pending: Optional[np.ndarray] = None      # the pending vector of the source slot, from the first deposit on

    def _sampled(self, *kinds) -> bool:
        """Some slot of one of these kinds has taken a sample (or a merge)."""
        return any(s.n > 0 and self._kind(k) in kinds for k, s in self._slots.items())

    def _sample(self, slot: int, x: np.ndarray):
        """One sample more of a slot, which is allocated at its first."""
        s = self._slots.get(slot)
        if s is None:
            s = self._slots[slot] = _Slot(x.size)
        s.n = welford_update(s.mean, s.m2, s.n, x)

    def _species_slot(self, slot: int, has: str):
        """The refusal of a slot that is no species slot where only one will do; has: what only a species slot has."""
        self._check_slot(slot)
        if self._kind(slot) != "species":
            raise ValueError(f"ensemble: slot {slot} is no species slot; only a species slot has {has}")

    def _set_photon_layout(self, layout):
        if self._sampled("photons", "source"):
            raise ValueError("ensemble: a photons slot has taken a sample; the photon layout stays as it is")

    def add_photons(self, backend, slot: int, observed=None, deposit: bool = False):
        """One photons sample of species slot `slot` from an `ObservedSpectra` (consumers.observed_spectra on `backend`): the observed
        processes as they are, the others 1e-99, the total rebuilt on this ensemble's layout.  deposit: the sample also joins the pending
        vector of the source slot (include/mcs.h, "source sample"): per word 1e-99 (the first deposit since the last take) or the word
        as it stands (a later one) plus the sample's word where that is above 1e-99.  Refused, with nothing changed, for a species slot
        already deposited since the last take."""
        from .consumers import PHOTON_PROCESSES, photon_total
        self._species_slot(slot, "a photons slot")
        if observed is None:
            raise ValueError("ensemble: the numpy ensemble takes its photons sample from an ObservedSpectra")
        if deposit and slot in self._deposited:
            raise ValueError(f"ensemble: species slot {slot} has been deposited since the last add_photons_all")
        lay = self.photon_layout
        if lay is None:
            raise ValueError("ensemble: no photon layout (set_photon_layout)")
        per = {p: np.asarray(a, dtype=np.float64) for p, a in observed.per_process.items()}
        if not per:
            raise ValueError("ensemble: the ObservedSpectra holds no process")
        for p, a in per.items():
            if a.shape != (lay.rows, lay.n[p]):
                raise ValueError(f"ensemble: {p!r} was observed as {a.shape}; the layout has {(lay.rows, lay.n[p])}")
        parts = [(per[p] if p in per else np.full((lay.rows, lay.n[p]), 1.0e-99)).ravel() for p in PHOTON_PROCESSES]
        x = np.concatenate(parts + [photon_total(per, lay).ravel()])
        self._sample(self.photons_slot(slot), x)
        if deposit:
            lit = np.where(x > 1.0e-99, x, 0.0)
            self._pending = (self._pending if self._deposited else 1.0e-99) + lit
            self._deposited.append(slot)

    def add_photons_all(self):
        """The take: one sample of the source slot, the pending vector as it stands; the deposits are then forgotten.  Refused with
        no deposit pending."""
        if not self._deposited:
            raise ValueError("ensemble: no deposit pending (add_photons(deposit=True))")
        self._sample(PHOTONS_ALL, self._pending)
        self._deposited.clear()

    def drop_pending_photons(self):
        """Forgets the deposits since the last take (the next first deposit starts the pending vector anew)."""
        self._deposited.clear()

    @staticmethod
    def _photon_layouts_differ(a, b) -> bool:
        return a.photon_layout is not None and b.photon_layout is not None and a.photon_layout.args() != b.photon_layout.args()

    def _vectors(self, slot: int):
        """(mean, M2, n) of a slot; (None, None, 0) for a products, photons or source slot that was never sampled."""
        s = self._slots.get(slot)
        return (None, None, 0) if s is None else (s.mean, s.m2, s.n)

    def _set_slope_window(self, l_lo, l_hi, x_log):
        if self._sampled("products", "escape"):
            raise ValueError("ensemble: a products or escape slot has taken a sample; the slope window stays as it is")

    def _set_angle_windows(self, l_lo, l_hi):
        if self._sampled("angles"):
            raise ValueError("ensemble: an angles slot has taken a sample; the angle windows stay as they are")

    def add_angles(self, backend, slot: int, angles):
        """One angles sample of species slot `slot` from an `AngleDistributions` (consumers.angle_distributions) made with this
        ensemble's windows."""
        self._species_slot(slot, "an angles slot")
        if self.angle_windows is None:
            raise ValueError("ensemble: no angle windows (set_angle_windows)")
        if angles is None:
            raise ValueError("ensemble: the numpy ensemble takes its angles sample from an AngleDistributions")
        if tuple(tuple(int(v) for v in w) for w in angles.windows) != tuple(zip(*self.angle_windows)):
            raise ValueError("ensemble: the windows of the AngleDistributions differ from the ensemble's")
        x = np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in (angles.dist, angles.number, angles.mean_mu, angles.mean_mu2)])
        if x.size != self._len(self.angles_slot(slot)):
            raise ValueError(f"ensemble: the AngleDistributions holds {x.size} words; an angles sample has {self._len(self.angles_slot(slot))}")
        with np.errstate(invalid="ignore"):          # (a NaN moment stays NaN)
            self._sample(self.angles_slot(slot), x)

    def add_tcuts(self, backend, slot: int, spectra):
        """One tcuts sample of species slot `slot` from a `TcutSpectra` (consumers.tcut_spectra); the ensemble's first fixes the
        number of time cuts."""
        self._species_slot(slot, "a tcuts slot")
        if spectra is None:
            raise ValueError("ensemble: the numpy ensemble takes its tcuts sample from a TcutSpectra")
        nt = len(spectra.number)
        if self.tcuts_n is not None and nt != self.tcuts_n:
            raise ValueError(f"ensemble: the TcutSpectra has {nt} time cuts, the ensemble's tcuts samples have {self.tcuts_n}")
        x = spectra.words()
        if x.size != self.layout.tcuts_fields(nt)["total"]:
            raise ValueError(f"ensemble: the TcutSpectra holds {x.size} words; a tcuts sample of {nt} cuts has {self.layout.tcuts_fields(nt)['total']}")
        self.tcuts_n = nt
        with np.errstate(invalid="ignore"):          # (a NaN of a dead row stays NaN)
            self._sample(self.tcuts_slot(slot), x)

    def add_detectors(self, backend, slot: int, spectra):
        """One detectors sample of species slot `slot` from a `DetectorSpectra` (consumers.detector_spectra); the ensemble's first
        fixes the settings."""
        self._species_slot(slot, "a detectors slot")
        if spectra is None:
            raise ValueError("ensemble: the numpy ensemble takes its detectors sample from a DetectorSpectra")
        st = spectra.settings()
        if self.detectors_settings is not None and st != self.detectors_settings:
            raise ValueError("ensemble: the settings of the DetectorSpectra (number of detectors, window, x_unit, x_spec) differ from those of "
                             "the ensemble's detectors samples")
        x = spectra.words()
        if x.size != self.layout.detectors_fields(st[0])["total"]:
            raise ValueError(f"ensemble: the DetectorSpectra holds {x.size} words; a detectors sample of {st[0]} detectors has "
                             f"{self.layout.detectors_fields(st[0])['total']}")
        self.detectors_settings = st
        with np.errstate(invalid="ignore"):          # (a NaN of a dead row or gradient bin stays NaN)
            self._sample(self.detectors_slot(slot), x)

    def add_profile(self, backend, update):
        """One profile sample from a `ProfileUpdate` (consumers.profile_update); the ensemble's first fixes the settings."""
        if update is None:
            raise ValueError("ensemble: the numpy ensemble takes its profile sample from a ProfileUpdate")
        if self._settings_differ(self.profile_settings, update.settings):
            raise ValueError("ensemble: the settings of the ProfileUpdate differ from those of the ensemble's profile samples")
        x = update.words()
        if x.size != self.layout.profile_fields()["total"]:
            raise ValueError(f"ensemble: the ProfileUpdate holds {x.size} words; a profile sample has {self.layout.profile_fields()['total']}")
        if self.profile_settings is None:
            self.profile_settings = np.array(update.settings, dtype=np.float64)
        with np.errstate(invalid="ignore"):          # (a non-finite word stays non-finite)
            self._sample(PROFILE_SLOT, x)

    def add_escape(self, backend, slot: int, spectra):
        """One escape sample of species slot `slot` from an `EscapeSpectra` (consumers.escape_spectra on `backend`), the slopes of its
        six rows by the backend's deterministic log10."""
        self._species_slot(slot, "an escape slot")
        if self.window is None:
            raise ValueError("ensemble: no slope window (set_slope_window)")
        if spectra is None:
            raise ValueError("ensemble: the numpy ensemble takes its escape sample from an EscapeSpectra")
        l_lo, l_hi, x_log = self.window
        dndp = np.asarray(spectra.dndp, dtype=np.float64)
        x = np.concatenate([dndp.ravel(), np.asarray(spectra.number, dtype=np.float64).ravel(),
                            slopes_of(dndp, l_lo, l_hi, x_log, _det_log10(backend)).ravel()])
        if x.size != self.layout.escape_total:
            raise ValueError(f"ensemble: the EscapeSpectra holds {x.size} words; an escape sample has {self.layout.escape_total}")
        with np.errstate(invalid="ignore"):          # (a NaN slope stays NaN)
            self._sample(self.escape_slot(slot), x)

    def add_products(self, backend, slot: int, ion_final):
        """One products sample of species slot `slot` from an `IonFinal` (consumers.ion_finalize on `backend`), the slopes by the
        backend's deterministic log10."""
        self._species_slot(slot, "a products slot")
        if self.window is None:
            raise ValueError("ensemble: no slope window (set_slope_window)")
        l_lo, l_hi, x_log = self.window
        dndp = np.asarray(ion_final.dNdp_cr, dtype=np.float64)
        x = np.concatenate([dndp.ravel(), np.asarray(ion_final.P_psd_par, dtype=np.float64), np.asarray(ion_final.P_psd_perp, dtype=np.float64),
                            np.asarray(ion_final.energy_density_psd, dtype=np.float64), slopes_of(dndp, l_lo, l_hi, x_log, _det_log10(backend)).ravel()])
        if x.size != self.layout.products_total:
            raise ValueError(f"ensemble: the IonFinal holds {x.size} words; a products sample has {self.layout.products_total}")
        with np.errstate(invalid="ignore"):          # (a NaN slope stays NaN)
            self._sample(self.products_slot(slot), x)

    @staticmethod
    def _windows_differ(a, b) -> bool:
        if a.window is None or b.window is None:
            return False
        return a.window[:2] != b.window[:2] or not np.array_equal(a.window[2].view(np.uint64), b.window[2].view(np.uint64))

    def begin_iteration(self, backend):
        o = self.layout.tally.offsets
        f, _ = backend.read_tallies()
        self._snapshot = (backend, f[o["esc_flux"]:o["energy_recv_pool"]].copy())

    def add_species(self, backend, slot: int):
        if slot == self.iteration_slot:
            raise ValueError(f"ensemble: slot {slot} is the iteration slot; it takes no species sample")
        self._species_slot(slot, "a species sample")
        f, i = backend.read_tallies()
        self._sample(slot, self.layout.species_sample(f, i))

    def add_iteration(self, backend):
        if self._snapshot is None or self._snapshot[0] is not backend:
            raise ValueError("ensemble: add_iteration without a begin_iteration of this backend since the last iteration sample")
        f, _ = backend.read_tallies()
        self._sample(self.iteration_slot, self.layout.iteration_sample(f, self._snapshot[1]))
        self._snapshot = None

    def merge(self, other: "HostEnsemble"):
        if other is self:
            raise ValueError("ensemble: merge of an ensemble into itself")
        if not isinstance(other, HostEnsemble) or other.n_species != self.n_species or other.layout.fields != self.layout.fields:
            raise ValueError("ensemble: merge needs an ensemble of the same kind, slots and layout")
        if self._windows_differ(self, other):
            raise ValueError("ensemble: merge of ensembles whose slope windows differ")
        if self._photon_layouts_differ(self, other):
            raise ValueError("ensemble: merge of ensembles whose photon layouts differ")
        if self._angle_windows_differ(self, other):
            raise ValueError("ensemble: merge of ensembles whose angle windows differ")
        if self._tcuts_differ(self, other):
            raise ValueError("ensemble: merge of ensembles whose tcuts samples differ in the number of time cuts")
        if self._profiles_differ(self, other):
            raise ValueError("ensemble: merge of ensembles whose profile samples differ in their settings")
        if self._detectors_differ(self, other):
            raise ValueError("ensemble: merge of ensembles whose detectors samples differ in their settings")
        # an ensemble without a photon layout or a slope window takes the one its samples were made with
        if other._sampled("photons", "source") and self.photon_layout is None:
            self.photon_layout = other.photon_layout
        if other._sampled("products", "escape") and self.window is None:
            self.window = other.window
        if other._sampled("angles") and self.angle_windows is None:
            self.angle_windows = other.angle_windows
        if other._sampled("tcuts") and self.tcuts_n is None:
            self.tcuts_n = other.tcuts_n
        if other._sampled("profile") and self.profile_settings is None:
            self.profile_settings = other.profile_settings
        if other._sampled("detectors") and self.detectors_settings is None:
            self.detectors_settings = other.detectors_settings
        for k, b in other._slots.items():      # (what is pending for the source slot on either side stays where it is)
            if b.n == 0:
                continue
            a = self._slots.get(k)
            if a is None or a.n == 0:
                self._slots[k] = b.copy()
            else:
                a.mean, a.m2 = _chan(a.mean, a.m2, a.n, b.mean, b.m2, b.n)
                a.n += b.n

    def count(self, slot: int) -> int:
        self._check_slot(slot)
        return self._vectors(slot)[2]

    def _read(self, slot, what, first, count):
        mean, m2, n = self._vectors(slot)
        if mean is None:
            raise ValueError(f"ensemble: {self._describe(slot)} has never taken a sample")
        if what == 2:
            if n < 2:
                raise ValueError(f"ensemble: the standard error needs at least two samples; slot {slot} has {n}")
            with np.errstate(invalid="ignore"):
                return np.sqrt(m2[first:first + count] / (float(n) * float(n - 1)))
        return (mean if what == 0 else m2)[first:first + count].copy()

    def _summarize(self, slot, n, ranges):
        mean, m2, _ = self._vectors(slot)
        return [summary_of(mean[first:first + count], m2[first:first + count], n, floor_frac, tol) for first, count, floor_frac, tol in ranges]

    def _summarize_merged(self, others, slot, n, ranges):
        out = []
        es = [self] + others
        if (self.is_products(slot) or self.is_escape(slot)) and any(self._windows_differ(a, b) for k, a in enumerate(es) for b in es[:k]):
            raise ValueError("ensemble: a merged summary of ensembles whose slope windows differ")
        if self._has_photon_vector(slot) and any(self._photon_layouts_differ(a, b) for k, a in enumerate(es) for b in es[:k]):
            raise ValueError("ensemble: a merged summary of ensembles whose photon layouts differ")
        if self.is_angles(slot) and any(self._angle_windows_differ(a, b) for k, a in enumerate(es) for b in es[:k]):
            raise ValueError("ensemble: a merged summary of ensembles whose angle windows differ")
        if self.is_tcuts(slot) and any(self._tcuts_differ(a, b) for k, a in enumerate(es) for b in es[:k]):
            raise ValueError("ensemble: a merged summary of ensembles whose tcuts samples differ in the number of time cuts")
        if self.is_profile(slot) and any(self._profiles_differ(a, b) for k, a in enumerate(es) for b in es[:k]):
            raise ValueError("ensemble: a merged summary of ensembles whose profile samples differ in their settings")
        if self.is_detectors(slot) and any(self._detectors_differ(a, b) for k, a in enumerate(es) for b in es[:k]):
            raise ValueError("ensemble: a merged summary of ensembles whose detectors samples differ in their settings")
        for first, count, floor_frac, tol in ranges:
            m, q, na = None, None, 0
            for e in [self] + others:
                mean_e, m2_e, nb = e._vectors(slot)
                if nb == 0:
                    continue
                mb, qb = mean_e[first:first + count], m2_e[first:first + count]
                m, q = (mb, qb) if na == 0 else _chan(m, q, na, mb, qb, nb)
                na += nb
            out.append(summary_of(m, q, n, floor_frac, tol))
        return out

    def _compare(self, other, slot, other_slot, n_a, n_b, ranges):
        if (self.is_products(slot) or self.is_escape(slot)) and self._windows_differ(self, other):
            raise ValueError("ensemble: a comparison of ensembles whose slope windows differ")
        if self._has_photon_vector(slot) and self._photon_layouts_differ(self, other):
            raise ValueError("ensemble: a comparison of ensembles whose photon layouts differ")
        if self.is_angles(slot) and self._angle_windows_differ(self, other):
            raise ValueError("ensemble: a comparison of ensembles whose angle windows differ")
        if self.is_tcuts(slot) and self._tcuts_differ(self, other):
            raise ValueError("ensemble: a comparison of ensembles whose tcuts samples differ in the number of time cuts")
        if self.is_profile(slot) and self._profiles_differ(self, other):
            raise ValueError("ensemble: a comparison of ensembles whose profile samples differ in their settings")
        if self.is_detectors(slot) and self._detectors_differ(self, other):
            raise ValueError("ensemble: a comparison of ensembles whose detectors samples differ in their settings")
        (ma, qa, _), (mb, qb, _) = self._vectors(slot), other._vectors(other_slot)
        return [difference_of(ma[first:first + count], qa[first:first + count], n_a, mb[first:first + count], qb[first:first + count], n_b,
                              floor_frac, zcut) for first, count, floor_frac, zcut in ranges]

    def load_mean(self, slot: int, backend):
        """The mean of a species slot written into the backend's per-species sections (num_crossings rounded to nearest)."""
        if slot == self.iteration_slot:
            raise ValueError(f"ensemble: slot {slot} is the iteration slot; only a species slot has histograms")
        if self.is_photons_all(slot):
            raise ValueError("ensemble: the source slot is no species slot; only a species slot has histograms")
        self._species_slot(slot, "histograms")
        L, o = self.layout.tally, self.layout.tally.offsets
        f, i = backend.read_tallies()
        m = self._slots[slot].mean
        n1 = o["esc_flux"] - o["psd"]
        f[o["psd"]:o["esc_flux"]] = m[:n1]
        L.view(f, "energy_recv_pool")[...] = m[n1:n1 + L.n_grid]
        i[:L.n_grid] = np.rint(m[n1 + L.n_grid:n1 + 2 * L.n_grid]).astype(np.int64)
        backend.write_tallies(f, i)


class HipEnsemble(Ensemble):
    """ctypes wrapper of the device accumulator (the ensemble calls of include/mcs.h).  `home`: a created HipBackend; it gives the
    device, the layout and the stream that merge and read use, and must be destroyed after the ensemble.  The contexts sampled
    from may be any on that device with that layout."""

    def __init__(self, home: HipBackend, n_species: int):
        super().__init__(home.P, n_species)
        self.lib, self.home = home.lib, home
        self.h = ct.c_void_p(None)
        self._chk(self.lib.mcs_ens_create(home.h, self.n_species, ct.byref(self.h)))

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError("libmcs_hip: " + self.lib.mcs_last_error().decode())

    def destroy(self):
        if self.h:
            self.lib.mcs_ens_destroy(self.h)
            self.h = ct.c_void_p(None)

    def begin_iteration(self, backend: HipBackend):
        self._chk(self.lib.mcs_ens_begin_iteration(self.h, backend.h))

    def add_species(self, backend: HipBackend, slot: int):
        self._chk(self.lib.mcs_ens_add_species(self.h, backend.h, int(slot)))

    def add_iteration(self, backend: HipBackend):
        self._chk(self.lib.mcs_ens_add_iteration(self.h, backend.h))

    def _set_slope_window(self, l_lo, l_hi, x_log):
        self._chk(self.lib.mcs_ens_set_slope_window(self.h, l_lo, l_hi, x_log.ctypes.data_as(capi.c_double_p)))

    def add_products(self, backend: HipBackend, slot: int, ion_final=None):
        """One products sample of species slot `slot` from what mcs_dndp_cr and mcs_thermo_calcs (consumers.ion_finalize) left on
        the backend's device (mcs_ens_add_products); nothing crosses to the host, ion_final is not read."""
        self._chk(self.lib.mcs_ens_add_products(self.h, backend.h, int(slot)))

    def add_escape(self, backend: HipBackend, slot: int, spectra=None):
        """One escape sample of species slot `slot` from what mcs_dndp_esc (consumers.escape_spectra) left on the backend's device
        (mcs_ens_add_escape); nothing crosses to the host, `spectra` is not read."""
        self._chk(self.lib.mcs_ens_add_escape(self.h, backend.h, int(slot)))

    def _set_angle_windows(self, l_lo, l_hi):
        lo, hi = np.asarray(l_lo, dtype=np.int32), np.asarray(l_hi, dtype=np.int32)
        self._chk(self.lib.mcs_ens_set_angle_windows(self.h, len(lo), lo.ctypes.data_as(capi.c_int32_p), hi.ctypes.data_as(capi.c_int32_p)))

    def add_angles(self, backend: HipBackend, slot: int, angles=None):
        """One angles sample of species slot `slot` from what mcs_angle_dist (consumers.angle_distributions) left on the backend's
        device (mcs_ens_add_angles); nothing crosses to the host, `angles` is not read."""
        self._chk(self.lib.mcs_ens_add_angles(self.h, backend.h, int(slot)))

    def add_tcuts(self, backend: HipBackend, slot: int, spectra=None):
        """One tcuts sample of species slot `slot` from what mcs_tcut_spectra (consumers.tcut_spectra) left on the backend's device
        (mcs_ens_add_tcuts); nothing crosses to the host, `spectra` is not read."""
        self._chk(self.lib.mcs_ens_add_tcuts(self.h, backend.h, int(slot)))
        if self.tcuts_n is None:
            self.tcuts_n = int(backend.n_tcuts)      # (as the library does: the first sample fixes it)

    def add_detectors(self, backend: HipBackend, slot: int, spectra=None):
        """One detectors sample of species slot `slot` from what mcs_detector_spectra (consumers.detector_spectra) left on the backend's
        device (mcs_ens_add_detectors); nothing crosses to the host, of `spectra` only the settings are noted."""
        self._chk(self.lib.mcs_ens_add_detectors(self.h, backend.h, int(slot)))
        if self.detectors_settings is None and spectra is not None:
            self.detectors_settings = spectra.settings()      # (as the library does: the first sample fixes them)

    def add_profile(self, backend: HipBackend, update=None):
        """One profile sample from what mcs_profile_update (consumers.profile_update) left on the backend's device
        (mcs_ens_add_profile); nothing crosses to the host, of `update` only the settings are noted."""
        self._chk(self.lib.mcs_ens_add_profile(self.h, backend.h))
        if self.profile_settings is None and update is not None:
            self.profile_settings = np.array(update.settings, dtype=np.float64)      # (as the library does: the first sample fixes them)

    def _set_photon_layout(self, layout):
        self._chk(self.lib.mcs_ens_set_photon_layout(self.h, *layout.args()))

    def add_photons(self, backend: HipBackend, slot: int, observed=None, deposit: bool = False):
        """One photons sample of species slot `slot` from what mcs_photon_observe (consumers.observed_spectra) left on the backend's
        device (mcs_ens_add_photons); nothing crosses to the host, `observed` is not read.  deposit: the same launch also adds the
        sample to the pending vector of the source slot (mcs_ens_add_photons_deposit)."""
        if not deposit:
            self._chk(self.lib.mcs_ens_add_photons(self.h, backend.h, int(slot)))
            return
        self._chk(self.lib.mcs_ens_add_photons_deposit(self.h, backend.h, int(slot)))
        self._deposited.append(int(slot))      # (what the library keeps, mirrored: it has refused a second deposit of the slot)

    def add_photons_all(self):
        """The take: one sample of the source slot from the pending vector on the device (mcs_ens_add_photons_all)."""
        self._chk(self.lib.mcs_ens_add_photons_all(self.h))
        self._deposited.clear()

    def drop_pending_photons(self):
        self._chk(self.lib.mcs_ens_drop_pending_photons(self.h))
        self._deposited.clear()

    def merge(self, other: "HipEnsemble"):
        if not isinstance(other, HipEnsemble):
            raise ValueError("ensemble: merge needs an ensemble of the same kind, slots and layout")
        self._chk(self.lib.mcs_ens_merge(self.h, other.h))
        if self.photon_layout is None and other.photon_layout is not None and (
                other.count(PHOTONS_ALL) or any(other.count(other.photons_slot(s)) for s in range(other.n_species))):
            self.photon_layout = other.photon_layout      # (as the library does)
        if self.window is None and other.window is not None and any(
                other.count(other.products_slot(s)) or other.count(other.escape_slot(s)) for s in range(other.n_species)):
            self.window = other.window      # (as the library does: an accumulator without a window takes the one its samples were made with)
        if self.angle_windows is None and other.angle_windows is not None and any(other.count(other.angles_slot(s)) for s in range(other.n_species)):
            self.angle_windows = other.angle_windows      # (likewise)
        if self.tcuts_n is None and other.tcuts_n is not None and any(other.count(other.tcuts_slot(s)) for s in range(other.n_species)):
            self.tcuts_n = other.tcuts_n      # (likewise)
        if self.profile_settings is None and other.profile_settings is not None and other.count(PROFILE_SLOT):
            self.profile_settings = other.profile_settings      # (likewise)
        if self.detectors_settings is None and other.detectors_settings is not None and any(other.count(other.detectors_slot(s)) for s in range(other.n_species)):
            self.detectors_settings = other.detectors_settings      # (likewise)

    def count(self, slot: int) -> int:
        n = ct.c_int64(0)
        self._chk(self.lib.mcs_ens_count(self.h, int(slot), ct.byref(n)))
        return int(n.value)

    def _read(self, slot, what, first, count):
        out = np.zeros(count)
        self._chk(self.lib.mcs_ens_read(self.h, int(slot), int(what), int(first), int(count), out.ctypes.data_as(capi.c_double_p)))
        return out

    def _summarize(self, slot, n, ranges):
        rs = (capi.McsEnsRange * len(ranges))(*[capi.McsEnsRange(*r) for r in ranges])
        out = (capi.McsEnsSummary * len(ranges))()
        self._chk(self.lib.mcs_ens_summarize(self.h, int(slot), len(ranges), rs, out))
        return [Summary(o.amax, o.max_rel, o.sum_se, o.sum_abs_mean, o.sum_rel2, int(o.n_selected), int(o.n_over), int(o.n_nonfinite),
                        int(o.argmax), n) for o in out]

    def _check_merged(self, others):
        # (the library refuses a duplicate, another device, other slots or layouts)
        if 1 + len(others) > MAX_MERGED:
            raise ValueError(f"ensemble: a merged summary of {1 + len(others)} ensembles; at most {MAX_MERGED}")
        if not all(isinstance(o, HipEnsemble) for o in others):
            raise ValueError("ensemble: a merged summary needs ensembles of the same kind, slots and layout")

    def _summarize_merged(self, others, slot, n, ranges):
        hs = (ct.c_void_p * (1 + len(others)))(*[e.h.value for e in [self] + others])
        rs = (capi.McsEnsRange * len(ranges))(*[capi.McsEnsRange(*r) for r in ranges])
        out = (capi.McsEnsSummary * len(ranges))()
        total = ct.c_int64(0)
        self._chk(self.lib.mcs_ens_summarize_merged(len(hs), hs, int(slot), len(ranges), rs, out, ct.byref(total)))
        return [Summary(o.amax, o.max_rel, o.sum_se, o.sum_abs_mean, o.sum_rel2, int(o.n_selected), int(o.n_over), int(o.n_nonfinite),
                        int(o.argmax), int(total.value)) for o in out]

    def _compare(self, other, slot, other_slot, n_a, n_b, ranges):
        rs = (capi.McsEnsCmpRange * len(ranges))(*[capi.McsEnsCmpRange(*r) for r in ranges])
        out = (capi.McsEnsDifference * len(ranges))()
        self._chk(self.lib.mcs_ens_compare(self.h, int(slot), other.h, int(other_slot), len(ranges), rs, out))
        return [Difference(o.amax, o.max_abs_z, o.sum_z, o.sum_abs_z, o.sum_z2, o.sum_abs_diff, o.sum_scale, int(o.n_selected), int(o.n_over),
                           int(o.n_nonfinite), int(o.n_degenerate), int(o.argmax), n_a, n_b) for o in out]

    def load_mean(self, slot: int, backend: HipBackend):
        self._chk(self.lib.mcs_ens_load_mean(self.h, int(slot), backend.h))


@dataclasses.dataclass
class ProfileConsistency:
    """How far the current profile is from the one its own fluxes predict (profile_consistency)."""
    n: int                   # samples
    z: np.ndarray            # [n_grid]: mean(shift) / stderr(shift); 0 where both vanish (a pinned zone), inf where only the error does
    chi2_upstream: float     # sum of z^2 over the upstream zones that have a finite z and a positive error
    n_upstream: int          # how many zones that sum has


def profile_consistency(ens: Ensemble, x_grid_cm=None, i_shock: Optional[int] = None) -> ProfileConsistency:
    """Per zone z = mean(shift) / stderr(shift) of the ensemble's profile slot, from its mean and M2 on the host (no new reduction),
    and the sum of z^2 over the upstream zones -- those with x_grid_cm[1..n_grid] < 0, or zones 1..i_shock (default: the i_shock of
    the ensemble's parameters).  A self-consistent profile has z of order one; refused below two samples."""
    n = ens.count(PROFILE_SLOT)
    if n < 2:
        raise ValueError(f"ensemble: profile_consistency needs at least two profile samples; the slot has {n}")
    mean, m2 = ens.mean(PROFILE_SLOT, "shift"), ens.m2(PROFILE_SLOT, "shift")
    ng = mean.size
    if x_grid_cm is not None:
        up = np.asarray(x_grid_cm, dtype=np.float64)[1:ng + 1] < 0
    else:
        up = np.arange(ng) < int(ens.i_shock if i_shock is None else i_shock)
    with np.errstate(all="ignore"):
        se = np.sqrt(m2 / (float(n) * float(n - 1)))
        z = np.where((mean == 0) & (se == 0), 0.0, mean / se)
    used = up & np.isfinite(z) & (se > 0)
    return ProfileConsistency(n, z, float(np.sum(z[used] * z[used])), int(np.count_nonzero(used)))
