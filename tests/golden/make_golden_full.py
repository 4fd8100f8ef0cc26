#!/usr/bin/env python3
"""Generate tests/golden/full_1e6.npz: BASELINE config[1] at FULL size -- 10^6 protons, single
unmodified gamma0 = 5 shock, all 45 stock pcuts, one iteration -- run once on the CPU oracle
(det math, OpenMP over particles; ~1.4e10 steps, about ten minutes on 8 cores), reduced to
binned spectra small enough to commit:

  *_mom[zone][k]   = sum over angle bins of psd / therm_sf / therm_pf   (dN(p) per zone, shock frame:
                     what get_dNdp_cr sums, src/particle_counter.jl:81-85)
  *_tht[zone][j]   = sum over momentum bins                             (angular distribution per zone)
  esc_psd_*_mom/_tht  the two marginals of the escape spectra
  every small tally array in full (fluxes, escape scalars and efficiencies, coupled weights and
  spectra, pools, scalars), the int64 tallies (crossings per zone, exits by reason, step and draw
  counts) and the per-pcut population sizes (n_pts_use, n_saved, i_mult).

Like every fixture here it is the ORACLE's output (the reference holds no vectors and cannot run):
oracle parity, not reference parity.  The GPU test (tests/test_gpu_full_size.py) runs the same
iteration through the C ABI and requires the integers to be equal and every fp64 array to agree
within 1e-11 of its maximum (order of the atomic adds; the threaded oracle has the same freedom).

--mixed writes tests/golden/mixed_1e5.npz instead: the species mix of `bench.py --mixed` (BASELINE
config[4]: protons + He + electrons, radiative losses, ion -> electron energy transfer) at 10^5
particles per species, one iteration, all pcuts, the same reduction of the tallies after the last
species, plus what the GPU test pins between the species: `stats` with i_ion in front, the
energy_transfer_pool and the int64 tallies at every species end (the pool is an fp64 sum whose
last bits depend on the order of the adds, and the electrons read it: the GPU test compares its
own pool with these and then continues from the oracle's bits).

    python tests/golden/make_golden_full.py [--mixed] [N] [threads]
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mcs_loader
mcs = _mcs_loader.load()

BIG = ("psd", "therm_sf", "therm_pf")
ESC = ("esc_psd_up", "esc_psd_down")


def mixed_problem(N, **kw):
    """The species mix of bench.py --mixed at N particles per species (kw: further Config fields, e.g. state_fp32)."""
    me_mp = mcs.constants.ME / mcs.constants.MP
    cfg = mcs.inputs.Config(N_PTS_INJ=N, N_PTS_PCUT=N, N_PTS_PCUT_HI=N,
                            species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(4.0, 2.0, 1e6, 0.1),
                                     mcs.inputs.Species(me_mp, -1.0, 1e6, 1.2)],
                            energy_transfer_frac=0.1, radiation_losses=True, **kw)
    return mcs.inputs.build_problem(cfg)


def reduce_tallies(L, T, I, stats, with_ion=False):
    """The committed reduction; the GPU test applies the same function to the HIP tallies.  with_ion: `stats` rows start
    with the species index (several species)."""
    out = {}
    for name in BIG:
        a = L.view(T, name)                       # [zone][tht][mom]
        out[name + "_mom"] = a.sum(axis=1)
        out[name + "_tht"] = a.sum(axis=2)
    for name in ESC:
        a = L.view(T, name)                       # [tht][mom]
        out[name + "_mom"] = a.sum(axis=0)
        out[name + "_tht"] = a.sum(axis=1)
    for name in L.offsets:
        if name in BIG or name in ESC:
            continue
        a = L.view(T, name)
        if a.size > 4096:                         # spectra_coupled, spectra_sf/pf: sparse
            nz = np.flatnonzero(a.ravel())
            out[name + "_idx"] = nz.astype(np.int64)
            out[name + "_val"] = a.ravel()[nz].copy()
        else:
            out[name] = a.copy()
    out["tallies_i64"] = I.copy()
    out["stats"] = np.array([([s.i_ion] if with_ion else []) + [s.i_pcut, s.n_pts_use, s.n_saved, s.i_mult] for s in stats], dtype=np.int64)
    return out


def main():
    import orc
    mixed = "--mixed" in sys.argv[1:]
    argv = [a for a in sys.argv[1:] if a != "--mixed"]
    N = int(argv[0]) if argv else (100_000 if mixed else 1_000_000)
    threads = int(argv[1]) if len(argv) > 1 else (os.cpu_count() or 1)
    orc.build()
    if mixed:
        prob = mixed_problem(N)
    else:
        cfg = mcs.inputs.Config(N_PTS_INJ=N, N_PTS_PCUT=N, N_PTS_PCUT_HI=N)
        prob = mcs.inputs.build_problem(cfg)
    be = orc.OracleBackend(mcs.capi, "det", nthreads=threads)
    be.create(prob)
    L = mcs.capi.Layout(prob.params)
    pools, ints = [], []

    def species_end(i_iter, i_ion, f, i):
        pools.append(L.view(f, "energy_transfer_pool").copy())
        ints.append(i.copy())
    t0 = time.perf_counter()
    res = mcs.driver.run(prob, be, None, n_itrs=1, verbose=True, on_species_end=species_end if mixed else None)
    dt = time.perf_counter() - t0
    out = reduce_tallies(L, res.tallies_f64, res.tallies_i64, res.stats, with_ion=mixed)
    steps = f"{res.steps_helix + res.steps_retro} steps in {dt:.0f} s"
    if mixed:
        out["species_energy_transfer_pool"] = np.array(pools)
        out["species_tallies_i64"] = np.array(ints)
        out["meta"] = np.array(f"N={N} per species (p, He, e-; bench.py --mixed), 45 stock pcuts, 1 iteration, oracle det math, "
                               f"{threads} threads, {steps}")
        name = "mixed_1e5.npz" if N == 100_000 else f"mixed_{N}.npz"
    else:
        out["meta"] = np.array(f"N={N} protons, 45 stock pcuts, 1 iteration, oracle det math, {threads} threads, {steps}")
        name = "full_1e6.npz" if N == 1_000_000 else f"full_{N}.npz"
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB; {out['meta']}")


if __name__ == "__main__":
    main()
