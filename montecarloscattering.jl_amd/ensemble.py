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

`HipEnsemble` keeps the vectors on the device and updates them with the kernels of csrc/mcs_ensemble.hip: the 22 MB histograms
never cross to the host (it costs device memory: two vectors of the sample length per slot, about twice the tally buffer per
species slot).  `HostEnsemble` does the same arithmetic in numpy, in the same order, on read_tallies() buffers: it lets the driver
path run with the CPU test backends (driver.accumulate_tallies_host is the precedent).  `Ensemble.for_backend` picks one.
"""
from __future__ import annotations

import ctypes as ct
from typing import Dict, Tuple

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
# what run_overlapped(ensemble=True) adds from the per-iteration ion_finalize of the last species
FINALIZE_NAMES = ("dNdp_cr", "P_psd_par", "P_psd_perp", "energy_density_psd")


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


def stats_over(samples):
    """(mean, standard error of the mean, count) of a list of equally shaped arrays, by the update above, in list order."""
    mean, m2, n = np.zeros_like(samples[0], dtype=np.float64), np.zeros_like(samples[0], dtype=np.float64), 0
    for x in samples:
        n = welford_update(mean, m2, n, np.asarray(x, dtype=np.float64))
    err = np.sqrt(m2 / (float(n) * float(n - 1))) if n >= 2 else np.full_like(mean, np.nan)
    return mean, err, n


class Ensemble:
    """What both kinds have in common: the slots, the named views of a slot's vectors."""

    def __init__(self, P: capi.McsParams, n_species: int):
        self.layout = EnsLayout(P)
        self.n_species = int(n_species)
        self.iteration_slot = self.n_species
        # run_overlapped(ensemble=True): mean / standard error / count over the iterations of ion_finalize's FINALIZE_NAMES
        self.finalize_mean: Dict[str, np.ndarray] = {}
        self.finalize_stderr: Dict[str, np.ndarray] = {}
        self.finalize_count = 0

    @staticmethod
    def for_backend(backend, n_species: int) -> "Ensemble":
        """A device accumulator beside a HIP context, the numpy one for every other backend."""
        if isinstance(backend, HipBackend):
            return HipEnsemble(backend, n_species)
        return HostEnsemble(backend.P, n_species)

    def names(self, slot: int):
        self._check_slot(slot)
        return ITERATION_NAMES if slot == self.iteration_slot else SPECIES_NAMES

    def _check_slot(self, slot: int):
        if not 0 <= slot <= self.n_species:
            raise ValueError(f"ensemble: slot {slot} outside 0..{self.n_species}")

    def _where(self, slot: int, name: str):
        self._check_slot(slot)
        table = self.layout.iteration if slot == self.iteration_slot else self.layout.species
        if name not in self.names(slot):
            kind = "the iteration slot" if slot == self.iteration_slot else f"species slot {slot}"
            raise KeyError(f"ensemble: {kind} has no {name!r}; it has: {', '.join(self.names(slot))}")
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

    def destroy(self):
        pass


class HostEnsemble(Ensemble):
    """The arithmetic of the device accumulator in numpy, word for word, on read_tallies() buffers."""

    def __init__(self, P: capi.McsParams, n_species: int):
        super().__init__(P, n_species)
        lens = [self.layout.species_total] * self.n_species + [self.layout.iteration_total]
        self._mean = [np.zeros(n) for n in lens]
        self._m2 = [np.zeros(n) for n in lens]
        self._n = [0] * len(lens)
        self._snapshot = None          # (backend, words [esc_flux, energy_recv_pool))

    def begin_iteration(self, backend):
        o = self.layout.tally.offsets
        f, _ = backend.read_tallies()
        self._snapshot = (backend, f[o["esc_flux"]:o["energy_recv_pool"]].copy())

    def add_species(self, backend, slot: int):
        self._check_slot(slot)
        if slot == self.iteration_slot:
            raise ValueError(f"ensemble: slot {slot} is the iteration slot; it takes no species sample")
        f, i = backend.read_tallies()
        self._n[slot] = welford_update(self._mean[slot], self._m2[slot], self._n[slot], self.layout.species_sample(f, i))

    def add_iteration(self, backend):
        if self._snapshot is None or self._snapshot[0] is not backend:
            raise ValueError("ensemble: add_iteration without a begin_iteration of this backend since the last iteration sample")
        f, _ = backend.read_tallies()
        s = self.iteration_slot
        self._n[s] = welford_update(self._mean[s], self._m2[s], self._n[s], self.layout.iteration_sample(f, self._snapshot[1]))
        self._snapshot = None

    def merge(self, other: "HostEnsemble"):
        if other is self:
            raise ValueError("ensemble: merge of an ensemble into itself")
        if not isinstance(other, HostEnsemble) or other.n_species != self.n_species or other.layout.fields != self.layout.fields:
            raise ValueError("ensemble: merge needs an ensemble of the same kind, slots and layout")
        for s in range(self.n_species + 1):
            na, nb = self._n[s], other._n[s]
            if nb == 0:
                continue
            if na == 0:
                self._mean[s][...] = other._mean[s]
                self._m2[s][...] = other._m2[s]
            else:
                n = float(na + nb)
                d = other._mean[s] - self._mean[s]
                self._mean[s][...] = self._mean[s] + d * (float(nb) / n)
                self._m2[s][...] = (self._m2[s] + other._m2[s]) + (d * d) * (float(na) * float(nb) / n)
            self._n[s] = na + nb

    def count(self, slot: int) -> int:
        self._check_slot(slot)
        return self._n[slot]

    def _read(self, slot, what, first, count):
        if what == 2:
            n = self._n[slot]
            if n < 2:
                raise ValueError(f"ensemble: the standard error needs at least two samples; slot {slot} has {n}")
            return np.sqrt(self._m2[slot][first:first + count] / (float(n) * float(n - 1)))
        return (self._mean if what == 0 else self._m2)[slot][first:first + count].copy()

    def load_mean(self, slot: int, backend):
        """The mean of a species slot written into the backend's per-species sections (num_crossings rounded to nearest)."""
        self._check_slot(slot)
        if slot == self.iteration_slot:
            raise ValueError(f"ensemble: slot {slot} is the iteration slot; only a species slot has histograms")
        L, o = self.layout.tally, self.layout.tally.offsets
        f, i = backend.read_tallies()
        m = self._mean[slot]
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

    def merge(self, other: "HipEnsemble"):
        if not isinstance(other, HipEnsemble):
            raise ValueError("ensemble: merge needs an ensemble of the same kind, slots and layout")
        self._chk(self.lib.mcs_ens_merge(self.h, other.h))

    def count(self, slot: int) -> int:
        n = ct.c_int64(0)
        self._chk(self.lib.mcs_ens_count(self.h, int(slot), ct.byref(n)))
        return int(n.value)

    def _read(self, slot, what, first, count):
        out = np.zeros(count)
        self._chk(self.lib.mcs_ens_read(self.h, int(slot), int(what), int(first), int(count), out.ctypes.data_as(capi.c_double_p)))
        return out

    def load_mean(self, slot: int, backend: HipBackend):
        self._chk(self.lib.mcs_ens_load_mean(self.h, int(slot), backend.h))
