"""What the time-cut spectra cost per species end (profiles/tcut_spectra.txt): K12, mcs_tcut_spectra, and the tcuts sample of the
ensemble statistics, mcs_ens_add_tcuts, at the stock binning and the stock ten time cuts, beside mcs_dndp_esc (K10) on the same context.
One iteration of N protons through driver.run for real tallies; then on that context, --calls rounds after two warm-up rounds:

  mcs_dndp_esc         HipBackend.dndp_esc on the run's escape slabs (table upload, two launches, download, wait)
  mcs_tcut_spectra     HipBackend.tcut_spectra on the run's coupled spectra over a zero base (table upload, two launches, two
                       downloads, wait)
  mcs_ens_add_tcuts    Ensemble.add_tcuts on what that call left, ended by a device synchronise

and mcs_tcut_spectra again with EVERY word of the species' block lit over a base other than zero, at the stock ten cuts and at 99 cuts
(the most the library takes).  Times are host clocks (time.perf_counter) around calls that end in a device synchronise; median and
range over the rounds.  Two calls on the same buffers must give the same bits; that is checked on every set.
--bench-json FILE: the JSON line of `python bench.py --gpus 1 ...` taken in another process; the cost per species end is then
printed as a share of its ms_per_step.
Run on the GPU: python tools/gpu_tcut_spectra.py [-N 20000] [--calls 40] [--bench-json FILE]."""
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


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a[0]).view(np.uint64), np.ascontiguousarray(b[0]).view(np.uint64)) and np.array_equal(a[1], b[1])


def timed(hb, calls, fn):
    out, ts = None, []
    for r in range(calls + 2):                       # (two warm-up rounds)
        hb.sync(); t0 = time.perf_counter()
        out = fn()
        hb.sync(); t1 = time.perf_counter()
        if r >= 2:
            ts.append(t1 - t0)
    return out, ts


def light_every_word(hb, prob, n_cuts, seed):
    """A base other than zero under begin_species, then every word of the species' block above it."""
    L, P = hb.layout, prob.params
    rng = np.random.default_rng(seed)
    top = 20.0 * P.age_max
    prob.tcuts = np.array([top]) if n_cuts == 1 else np.logspace(2.0, np.log10(top), n_cuts)
    hb.set_cuts(prob)
    base = rng.uniform(0.0, 5.0, L.shapes["spectra_coupled"])
    hb.write_tally("spectra_coupled", base)
    sp = prob.cfg.species[0]
    hb.begin_species(1, 1, sp.aa, abs(sp.zz), prob.pmax, sp.density, 1.0)
    hb.write_tally("spectra_coupled", base + 10.0 ** rng.uniform(-12, 2, base.shape))
    hb.write_tally("weight_coupled", rng.uniform(0.1, 1.0, L.shapes["weight_coupled"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=20000, help="particles per pcut")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--bench-json", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    prob = mcs.inputs.build_problem(mcs.inputs.Config(N_PTS_INJ=args.N, N_PTS_PCUT=args.N, N_PTS_PCUT_HI=args.N, num_iterations=2))
    P = prob.params
    nm, nt, n_cuts = P.num_psd_mom_bins, P.num_psd_tht_bins, len(prob.tcuts)
    hb = hip_backend(prob)
    t0 = time.perf_counter()
    mcs.driver.run(prob, hb, n_itrs=1)
    print(f"one iteration of {args.N} protons: {time.perf_counter() - t0:.2f} s; stock binning nmom {nm}, ntht {nt}, n_grid {P.n_grid}, {n_cuts} time cuts")
    tabs = cons.consumer_tables(prob, 1)
    gam_pf = cons.escape_gam_pf(prob)
    L = hb.layout
    f, _ = hb.read_tallies()
    block = L.view(f, "spectra_coupled")[0][:n_cuts, :nm + 1]
    print(f"lit words (> 0) of the run's coupled spectra: {int((block > 0).sum())} of {block.size} in {n_cuts} rows")
    e = mcs.ensemble.Ensemble.for_backend(hb, 1)
    _, t_esc = timed(hb, args.calls, lambda: hb.dndp_esc(tabs, gam_pf))
    first, t_tc = timed(hb, args.calls, lambda: hb.tcut_spectra(tabs))
    again = hb.tcut_spectra(tabs)
    spec = cons.tcut_spectra(prob, hb, 1)
    print(f"the run's tallies: number {spec.number.tolist()}, diag {first[1].tolist()}; two calls, the same bits: {same_bits(first, again)}")
    print(f"  median momentum reached (log10 p, cgs) per cut {spec.quantile[0].tolist()}, index {spec.index.tolist()}")
    t_add = []
    for r in range(args.calls + 2):
        hb.tcut_spectra(tabs)
        hb.sync(); a = time.perf_counter()
        e.add_tcuts(hb, 0)
        hb.sync(); b = time.perf_counter()
        if r >= 2:
            t_add.append(b - a)
    dense = {}
    for cuts in (n_cuts, 99):
        light_every_word(hb, prob, cuts, cuts)
        out, ts = timed(hb, args.calls, lambda: hb.tcut_spectra(tabs))
        again = hb.tcut_spectra(tabs)
        dense[cuts] = ts
        print(f"every word lit, {cuts} cuts: diag {out[1].tolist()}; two calls, the same bits: {same_bits(out, again)}")
    print(f"{args.calls} rounds after 2 warm-up rounds; median (min .. max)")
    print(f"  mcs_dndp_esc (K10), the run's slabs                 {ms(t_esc)}")
    print(f"  mcs_tcut_spectra (K12), the run's tallies, {n_cuts} cuts   {ms(t_tc)}")
    print(f"  mcs_tcut_spectra (K12), every word lit, {n_cuts} cuts      {ms(dense[n_cuts])}")
    print(f"  mcs_tcut_spectra (K12), every word lit, 99 cuts      {ms(dense[99])}")
    print(f"  mcs_ens_add_tcuts + synchronise                     {ms(t_add)}")
    per_end = (statistics.median(t_tc) + statistics.median(t_add)) * 1e3
    worst = (statistics.median(dense[n_cuts]) + statistics.median(t_add)) * 1e3
    print(f"per species end: {per_end:.3f} ms (every word lit: {worst:.3f} ms)")
    if args.bench_json:
        line = [ln for ln in open(args.bench_json).read().splitlines() if ln.startswith("{")][-1]
        b = json.loads(line)
        it = b["ms_per_step"]
        print(f"bench.py: {b['config']['workload']}: {it:.1f} ms per iteration (one species); tcuts=True adds {per_end:.3f} ms = {100 * per_end / it:.3f} % of it "
              f"(every word lit: {100 * worst / it:.3f} %)")
    e.destroy(); hb.destroy()


if __name__ == "__main__":
    main()
