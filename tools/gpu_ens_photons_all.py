"""What the source sample -- the photon spectrum summed over species, sampled once per iteration -- adds to a run
(profiles/ensemble_photons_all.txt).  At the stock layout (6 photon shells; 179 / 139 / 119 energy words on 250 points: a sample vector
of 4809 words) and the species of bench.py --mixed (p and He: pion decay; e-: synchrotron + inverse Compton), on crafted emission that
mcs_photon_observe turns into shell spectra on the context, it times three calls:

  plain   mcs_ens_add_photons: the species' photons sample alone (Ensemble.add_photons)
  fused   mcs_ens_add_photons_deposit: the same sample and, in the same launch, its deposit into the pending vector (deposit=True)
  take    mcs_ens_add_photons_all: the pending vector as one sample of the source slot (Ensemble.add_photons_all)

Every call follows an mcs_photon_observe, which waits for the device, as at a species end of driver.run: the stream is idle when the
call is queued.  The context works on a stream of the caller's; an event recorded on it before the call and one after give the time
the device saw (launch latency and kernel), and a host clock around the call and a synchronise gives what the host waited.  After
--warmup calls of each kind, --calls timed calls per species; the three kinds alternate inside one loop.  Median (min .. max).
--only-plain: the first call alone, with nothing this tool's commit added -- the same file run in a checkout of the parent commit
times its mcs_ens_add_photons in the same session.
--bench-json FILE: the JSON line of `python bench.py --gpus 1 --mixed ...` taken in another process; what an iteration of
p + He + e- pays more than before -- three times (fused - plain) and one take -- is then printed as a share of its ms_per_step.
Run on the GPU: python tools/gpu_ens_photons_all.py [--calls 300] [--warmup 20] [--only-plain] [--bench-json FILE]."""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from conftest import mcs  # noqa: E402

cons = mcs.consumers
SPECIES = (("p", ("pion",)), ("He", ("pion",)), ("e-", ("synch", "ic")))


def fmt(ts):
    return f"{statistics.median(ts) * 1e3:8.2f} us  ({min(ts) * 1e3:.2f} .. {max(ts) * 1e3:.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only-plain", action="store_true")
    ap.add_argument("--bench-json", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from mcs_amd import hip_backend as hbm
    me_mp = mcs.constants.ME / mcs.constants.MP
    cfg = mcs.inputs.Config(N_PTS_INJ=1000, N_PTS_PCUT=1000, N_PTS_PCUT_HI=1000, num_iterations=2, energy_transfer_frac=0.1, radiation_losses=True,
                            JETFR=(0.0, 20.0), species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(4.0, 2.0, 1e6, 0.1),
                                                        mcs.inputs.Species(me_mp, -1.0, 1e6, 1.2)])
    prob = mcs.inputs.build_problem(cfg)
    stream = torch.cuda.Stream()
    hb = hbm.HipBackend(0, stream=int(stream.cuda_stream))
    hb.create(prob)
    setup = cons.PhotonSetup(3, 3, jet_dist_kpc=1.0e3)
    layout = cons.stock_photon_layout(setup.n_shells)
    ng = prob.params.n_grid
    print(f"n_grid {ng}; layout {layout.args()}: {layout.offsets()['_total']} words per sample vector; species {[name for name, _ in SPECIES]}")
    # crafted emission per process: seven words in ten lit, over twelve decades of photon flux
    rng = np.random.default_rng(0)
    calls = {}
    for p in cons.PHOTON_PROCESSES:
        n_photon = cons.photon_n_photon(p)
        E_MeV = cons.photon_e_min(p) * 10.0 ** (np.arange(n_photon) / cons.PHOTON_BINS_PER_DEC)
        tabs = cons.observe_tables(prob, setup, p, E_MeV)
        flux = np.where(rng.random((ng, n_photon)) < 0.7, 10.0 ** rng.uniform(-14, -2, (ng, n_photon)), 1e-99)
        emis = flux * tabs["energy_div"][None, :] * (cons.MEV_ERG if p == "ic" else tabs["area"] * (cons.MEV_ERG if p == "synch" else 1.0))
        calls[p] = dict(tabs, emis=emis)

    def observe(processes):
        for p in processes:
            hb.photon_observe(p, download=False, **calls[p])

    e = mcs.ensemble.Ensemble.for_backend(hb, len(SPECIES))
    e.set_photon_layout(layout)

    def timed(call):
        """-> (ms between two events on the stream around the call, ms of a host clock around the call and a synchronise)"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hb.sync()
        t0 = time.perf_counter()
        a.record(stream)
        call()
        b.record(stream)
        hb.sync()
        t1 = time.perf_counter()
        b.synchronize()
        return a.elapsed_time(b), (t1 - t0) * 1e3

    kinds = ("plain",) if args.only_plain else ("plain", "fused", "take")
    T = {k: {s: ([], []) for s in range(len(SPECIES))} for k in kinds}
    for r in range(args.warmup + args.calls):
        for s, (_, processes) in enumerate(SPECIES):
            got = {}
            observe(processes)
            got["plain"] = timed(lambda: e.add_photons(hb, s))
            if not args.only_plain:
                observe(processes)
                got["fused"] = timed(lambda: e.add_photons(hb, s, deposit=True))
                got["take"] = timed(e.add_photons_all)
            if r >= args.warmup:
                for k in kinds:
                    T[k][s][0].append(got[k][0]); T[k][s][1].append(got[k][1])
    names = dict(plain="mcs_ens_add_photons", fused="mcs_ens_add_photons_deposit", take="mcs_ens_add_photons_all")
    print(f"{args.calls} calls per kind and species after {args.warmup} warm-up calls, the kinds alternating; median (min .. max)")
    for k in kinds:
        for s, (name, processes) in enumerate(SPECIES):
            print(f"  {names[k]:<30}{name:>3} ({' + '.join(processes):<10}) events {fmt(T[k][s][0])}   host, with the wait {fmt(T[k][s][1])}")
    if not args.only_plain:
        med = lambda k, s, j: statistics.median(T[k][s][j])
        for j, what in ((0, "events"), (1, "host clock")):
            fused_more = sum(med("fused", s, j) - med("plain", s, j) for s in range(len(SPECIES)))
            take = med("take", len(SPECIES) - 1, j)           # (one take per iteration, after the last species)
            added = fused_more + take
            ratio = [med("fused", s, j) / med("plain", s, j) for s in range(len(SPECIES))]
            print(f"{what}: fused / plain per species {', '.join(f'{x:.3f}' for x in ratio)}; a launch of its own for the deposit would cost about a take more "
                  f"per species ({take * 1e3:.2f} us)")
            print(f"{what}: added per iteration of p + He + e-: 3 x (fused - plain) = {fused_more * 1e3:.2f} us, + one take {take * 1e3:.2f} us = {added * 1e3:.2f} us")
            if args.bench_json:
                line = [ln for ln in open(args.bench_json).read().splitlines() if ln.startswith("{")][-1]
                b = json.loads(line)
                it = b["ms_per_step"]
                print(f"{what}: bench.py: {it:.1f} ms per iteration of 10^6 particles per species; the source sample adds {added:.4f} ms = {100 * added / it:.4f} % of it")
    counts = [e.count(e.photons_slot(s)) for s in range(len(SPECIES))]
    print(f"samples taken: photons slots {counts}" + ("" if args.only_plain else f", source slot {e.count(e.photons_all_slot)}"))
    e.destroy(); hb.destroy()


if __name__ == "__main__":
    main()
