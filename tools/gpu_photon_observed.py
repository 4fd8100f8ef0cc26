"""What the photon spectra at Earth cost per species end, on the device and the way they were made before (profiles/photon_observed.txt).
The species mix of bench.py --mixed (protons + He + electrons, radiative losses, energy transfer) at N particles per species, one
iteration through driver.run for real tallies; then, per species, on its own tallies written back to the context:

  new   consumers.observed_spectra (the species' folds K5-K7 as they are, emission download included, each followed by
        mcs_photon_observe, K9, on what the fold left on the device) and one Ensemble.add_photons (mcs_ens_add_photons), ended by a
        device synchronise
  old   the same folds with their emission downloaded, then consumers.summed_emission: doppler_to_ism and the shell sums in numpy

The two alternate inside one loop of --calls rounds; ion_finalize (K4), which both need first, is timed on its own.  Also: K9 alone
(HipBackend.photon_observe(emis=None, download=False) on what the fold left), the sample alone, and that the two paths give the same
bits.  Times are host clocks (time.perf_counter) around calls that end in a device synchronise; median and range over the rounds.
--bench-json FILE: the JSON line of `python bench.py --gpus 1 --mixed ...` taken in another process; the cost per iteration (all
species) is then printed as a share of its ms_per_step.
Run on the GPU: python tools/gpu_photon_observed.py [-N 20000] [--calls 20] [--bench-json FILE]."""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from conftest import mcs, hip_backend  # noqa: E402

cons = mcs.consumers


def ms(ts):
    ts = [t * 1e3 for t in ts]
    return f"{statistics.median(ts):8.3f} ms  ({min(ts):.3f} .. {max(ts):.3f})"


def folds_of(prob, hb, i_ion, fin, setup):
    sp = prob.cfg.species[i_ion - 1]
    kw = dict(jet_dist_kpc=setup.jet_dist_kpc, redshift=setup.redshift)
    if sp.aa < 1:
        return dict(synch=cons.photon_synch(prob, hb, fin, i_ion, **kw), ic=cons.photon_ic(prob, hb, i_ion, jet_sph_frac=setup.jet_sph_frac, **kw))
    return dict(pion=cons.photon_pion(prob, hb, fin, i_ion, **kw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=20000, help="particles per species and pcut")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--bench-json", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    me_mp = mcs.constants.ME / mcs.constants.MP
    cfg = mcs.inputs.Config(N_PTS_INJ=args.N, N_PTS_PCUT=args.N, N_PTS_PCUT_HI=args.N, num_iterations=2, energy_transfer_frac=0.1, radiation_losses=True,
                            JETFR=(0.0, 20.0), species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(4.0, 2.0, 1e6, 0.1),
                                                        mcs.inputs.Species(me_mp, -1.0, 1e6, 1.2)])
    prob = mcs.inputs.build_problem(cfg)
    hb = hip_backend(prob)
    setup = cons.PhotonSetup(3, 3, jet_dist_kpc=1.0e3)
    _, zones = cons.photon_shells(prob, 3, 3)
    n_sp = len(cfg.species)
    t0 = time.perf_counter()
    res = mcs.driver.run(prob, hb, n_itrs=1, species_tallies="full")
    print(f"one iteration of p + He + e-, N = {args.N} per species: {time.perf_counter() - t0:.2f} s; n_grid {prob.params.n_grid}, 6 photon shells at zones {[int(z) for z in zones]}")
    e = mcs.ensemble.Ensemble.for_backend(hb, n_sp)
    e.set_photon_layout(cons.stock_photon_layout(setup.n_shells))
    T = {k: {i: [] for i in range(1, n_sp + 1)} for k in ("fin", "new", "old", "k9", "sample", "numpy")}
    same = True
    for i_iter, i_ion, f, i in res.per_species:
        hb.write_tallies(f, i)
        for r in range(args.calls + 2):                  # (two warm-up rounds)
            hb.sync(); t0 = time.perf_counter()
            fin = cons.ion_finalize(prob, hb, i_ion)
            hb.sync(); t1 = time.perf_counter()
            obs = cons.observed_spectra(prob, hb, i_ion, setup, fin)
            e.add_photons(hb, i_ion - 1)
            hb.sync(); t2 = time.perf_counter()
            folds = folds_of(prob, hb, i_ion, fin, setup)
            t2b = time.perf_counter()
            se = cons.summed_emission(prob, zones, **folds)
            t3 = time.perf_counter()
            # K9 alone on what the folds left, and one sample alone
            k9 = 0.0
            for p, ph in folds.items():
                tabs = cons.observe_tables(prob, setup, p, ph.energy_MeV)
                if p == "pion":
                    tabs["energy_div"] = np.ascontiguousarray(ph.energy_erg)
                hb.sync(); a = time.perf_counter()
                hb.photon_observe(p, download=False, **tabs)
                k9 += time.perf_counter() - a
            hb.sync(); a = time.perf_counter()
            e.add_photons(hb, i_ion - 1)
            hb.sync(); t_sample = time.perf_counter() - a
            if r >= 2:
                for k, v in (("fin", t1 - t0), ("new", t2 - t1), ("old", t3 - t2), ("numpy", t3 - t2b), ("k9", k9), ("sample", t_sample)):
                    T[k][i_ion].append(v)
        # the two paths give the same numbers: log10(sh / dlog) against summed_emission's per-process arrays, bit for bit
        for p, sh in obs.per_process.items():
            want = se.per_process[p][1]
            got = np.where(sh[:-1] > 1e-99, np.log10(np.maximum(sh[:-1], 1e-300) / obs.dlog), -99.0)
            ok = np.array_equal(got.view(np.uint64), want.view(np.uint64))
            same = same and ok
            print(f"  species {i_ion} {p:<6}: {(want > -99).sum():5d} lit words of {want.size}; device path == numpy path bit for bit: {ok}")
    print(f"per species end, {args.calls} rounds after 2 warm-up rounds, the two paths alternating; median (min .. max)")
    names = dict(fin="ion_finalize (K4; both paths need it)", new="NEW folds + K9 + sample", old="OLD folds + download + numpy",
                 numpy="  of which doppler_to_ism + shell sums (numpy)", k9="  K9 alone (mcs_photon_observe, emis = NULL)", sample="  mcs_ens_add_photons alone")
    for i_ion in range(1, n_sp + 1):
        sp = cfg.species[i_ion - 1]
        print(f"species {i_ion} (aa = {sp.aa:.4g}: {'synch + ic' if sp.aa < 1 else 'pion'})")
        for k in ("fin", "new", "old", "numpy", "k9", "sample"):
            print(f"  {names[k]:<48}{ms(T[k][i_ion])}")
    new_it = sum(statistics.median(T["new"][i]) for i in T["new"]) * 1e3
    old_it = sum(statistics.median(T["old"][i]) for i in T["old"]) * 1e3
    fin_it = sum(statistics.median(T["fin"][i]) for i in range(1, n_sp)) * 1e3      # (the last species' ion_finalize is the finalize step's)
    print(f"per iteration (all species): new {new_it:.2f} ms, old {old_it:.2f} ms, + {fin_it:.2f} ms for the ion_finalize of species 1..{n_sp - 1} that photons= adds")
    print(f"the two paths agree bit for bit everywhere: {same}")
    if args.bench_json:
        line = [ln for ln in open(args.bench_json).read().splitlines() if ln.startswith("{")][-1]
        b = json.loads(line)
        it = b["ms_per_step"]
        print(f"bench.py: {b['config']['workload']}: {it:.1f} ms per iteration; photons= adds {new_it + fin_it:.2f} ms = {100 * (new_it + fin_it) / it:.2f} % of it "
              f"(the old path would add {old_it + fin_it:.2f} ms = {100 * (old_it + fin_it) / it:.2f} %)")
    e.destroy(); hb.destroy()


if __name__ == "__main__":
    main()
