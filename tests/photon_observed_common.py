"""What the tests of the observed shell spectra (K9) share: a serial restatement of the definition in include/mcs.h in Python floats,
crafted emission arrays that reach every branch of it, and the host tables of a call."""
import math

import numpy as np

from conftest import mcs

cons = mcs.consumers
MEV = cons.MEV_ERG
BETAS = (0.0, 0.3, 0.6, 0.9, math.sqrt(24.0 / 25.0))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def serial_restatement(process, emis, energy_div, energy_grid, area, dlog, last_mid_ratio, cos_edge, gam_ef, beta_ef, gam3_ef, shell_ends):
    """include/mcs.h, "observed shell spectra", steps 1-4, one Python float operation per rounding, every loop in the stated order.
    The Doppler step is written as the host's scatter: slices ascending, within a slice the energies ascending."""
    emis = np.asarray(emis, dtype=np.float64)
    nz, n_photon = emis.shape
    n = n_photon - 1
    E = [float(v) for v in energy_grid]
    nb = [[1.0e-99] * n for _ in range(nz)]
    for z in range(nz):
        g = []
        for j in range(n):
            x = float(emis[z, j])
            if process == "synch":
                e = x / area
                e = e if e > 1.0e-99 else 1.0e-99
                e = e / MEV if e > 1.0e-99 else 1.0e-99
            elif process == "ic":
                e = x / MEV if x > 1.0e-99 else 1.0e-99
            else:
                e = x / area
                e = e if e >= 1.0e-99 else 1.0e-99
            f = 1.0e-99 if e <= 1.0e-99 else e / float(energy_div[j])
            g.append(f * dlog if f > 1.0e-90 else f)
        if process == "ic":
            nb[z] = g
            continue
        num = [v / 180 for v in g]
        mid = [math.sqrt(E[j] * E[j + 1]) for j in range(n - 1)]
        mid.append(mid[n - 2] * last_mid_ratio)
        gam, beta = float(gam_ef[z]), float(beta_ef[z])
        acc = [1.0e-99] * n
        for l in range(180):
            fac = gam * math.sqrt((1 - beta * float(cos_edge[l])) * (1 - beta * float(cos_edge[l + 1])))
            for j in range(n):
                t = mid[j] * fac
                m = 1
                while m < n and not E[m] >= t:
                    m += 1
                if num[j] > 1.0e-99 and m < n:
                    acc[m - 1] = acc[m - 1] + num[j]
        nb[z] = [a * float(gam3_ef[z]) if a > 1.0e-95 else 1.0e-99 for a in acc]
    n_shells = len(shell_ends) - 1
    out = np.full((n_shells + 1, n), 1.0e-99)
    for k in range(n):
        tot = 0.0
        for s in range(n_shells):
            lo, hi = int(shell_ends[s]), int(shell_ends[s + 1]) - 1
            sh = 1.0e-99
            if lo >= 1 and hi >= lo:
                a = 0.0
                for z in range(lo, hi + 1):
                    v = nb[z - 1][k]
                    a = a + (v if v > 1.0e-95 else 0.0)
                sh = a if a > 1.0e-99 else 1.0e-99
            out[s, k] = sh
            tot = tot + (sh if sh > 1.0e-99 else 0.0)
        out[n_shells, k] = tot if tot > 1.0e-99 else 1.0e-99
    return out


def tables(process, n_grid, n_photon, betas, shell_ends, e_min_mev=1.0e-3, area=4 * math.pi * (3.0e24) ** 2):
    """The host tables of one call for a grid of 10 energies per decade, as consumers.observe_tables builds them."""
    E_MeV = e_min_mev * 10.0 ** (np.arange(n_photon) / 10)
    beta = np.ascontiguousarray(np.resize(np.asarray(betas, dtype=np.float64), n_grid))
    gam = 1.0 / np.sqrt(1.0 - beta * beta)
    dlog = 1.0 / 10
    return dict(energy_div=E_MeV * MEV if process == "pion" else E_MeV, energy_grid=E_MeV, area=area, dlog=dlog, last_mid_ratio=10.0 ** dlog,
                cos_edge=np.linspace(-1.0, 1.0, 181), gam_ef=gam, beta_ef=beta, gam3_ef=gam ** 3, shell_ends=np.asarray(shell_ends, dtype=np.int64))


def emis_for_flux(process, flux, tabs):
    """An emission whose photon flux is about `flux` (the conversions of step 1 undone, not bit for bit)."""
    e = np.asarray(flux, dtype=np.float64) * tabs["energy_div"][None, :]
    return e * MEV if process == "ic" else e * tabs["area"] * (MEV if process == "synch" else 1.0)


def crafted_emis(process, n_grid, n_photon, tabs, seed=0):
    """[n_grid][n_photon]: zone by zone the cases of the definition, then (from zone 6 on) dark, line and dense zones again, so that
    every shell layout of the tests finds all of them under every beta of `BETAS`:
      0 dark | 1 a single line | 2 a dense random row | 3 lines in the top two bins (shifted beyond the grid: dropped) |
      4 one flux between 1e-99 and 1e-90 (no bin-width factor) beside a line | 5 a line in the lowest bin (a red shift clamps at m = 1)"""
    rng = np.random.default_rng(seed)
    flux = np.full((n_grid, n_photon), 1.0e-99)
    for z in range(n_grid):
        kind = z % 6 if z >= 6 else z
        if kind == 1:
            flux[z, n_photon // 2] = 2.5e-6
        elif kind == 2:
            flux[z] = 10.0 ** rng.uniform(-12, -3, n_photon)
        elif kind == 3:
            flux[z, n_photon - 2] = 1.0e-5; flux[z, n_photon - 3] = 3.0e-7
        elif kind == 4:
            flux[z, 5] = 4.0e-95; flux[z, 9] = 1.0e-8
        elif kind == 5:
            flux[z, 0] = 7.0e-7; flux[z, 1] = 2.0e-7
    emis = emis_for_flux(process, flux, tabs)
    # (the floor applies to the energy flux in erg: the smallest lit one gives a photon flux of 6e-94 / E[MeV], below 1e-90 at E[5])
    for z in range(n_grid):
        if (z % 6 if z >= 6 else z) == 4:
            emis[z, 5] = 2.0e-99 * (1.0 if process == "ic" else tabs["area"])
    return emis


def flux_classes(process, emis, tabs):
    """How many words of step 1's flux lie on the floor, between the floor and 1e-90, and above."""
    f = cons.photon_flux_host(process, emis, tabs["energy_div"], tabs["area"])[:, :-1]
    return int((f <= 1.0e-99).sum()), int(((f > 1.0e-99) & (f <= 1.0e-90)).sum()), int((f > 1.0e-90).sum())
