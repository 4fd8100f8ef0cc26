"""What the detector spectra cost per species end (profiles/detector_spectra.txt): K14, mcs_detector_spectra, and the detectors sample
of the ensemble statistics, mcs_ens_add_detectors, at the stock binning with five detectors at (-0.5, -0.3, -0.1, 0.05, 2.0) rg0,
beside mcs_tcut_spectra (K12) on the same context.  One iteration of N protons through driver.run for real tallies; then on that
context, --calls rounds after two warm-up rounds:

  mcs_tcut_spectra        HipBackend.tcut_spectra on the run's coupled spectra (table upload, two launches, two downloads, wait)
  mcs_detector_spectra    HipBackend.detector_spectra on the run's detector rows over a zero base (table upload, two launches, two
                          downloads, wait)
  mcs_ens_add_detectors   Ensemble.add_detectors on what that call left, ended by a device synchronise

and mcs_detector_spectra again with EVERY word of the detectors' rows lit over a base other than zero, at the five detectors and at
n_grid detectors (the most the library takes).  Times are host clocks (time.perf_counter) around calls that end in a device
synchronise; median and range over the rounds.  Two calls on the same buffers must give the same bits; that is checked on every set.
--bench-json FILE: the JSON line of `python bench.py --gpus 1 ...` taken in another process; the cost per species end is then
printed as a share of its ms_per_step.
Run on the GPU: python tools/gpu_detector_spectra.py [-N 20000] [--calls 40] [--bench-json FILE]."""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from conftest import mcs, hip_backend  # noqa: E402

cons = mcs.consumers
XSPEC_RG = (-0.5, -0.3, -0.1, 0.05, 2.0)


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


def light_every_word(hb, prob, x_rg, seed):
    """A base other than zero under begin_species, then every word of the detectors' rows above it."""
    L = hb.layout
    rng = np.random.default_rng(seed)
    prob.x_spec = np.asarray(x_rg, dtype=np.float64) * prob.rg0
    hb.set_cuts(prob)
    base = {name: rng.uniform(0.0, 5.0, L.shapes[name]) for name in ("spectra_sf", "spectra_pf")}
    for name, b in base.items():
        hb.write_tally(name, b)
    sp = prob.cfg.species[0]
    hb.begin_species(1, 1, sp.aa, abs(sp.zz), prob.pmax, sp.density, 1.0)
    for name, b in base.items():
        hb.write_tally(name, b + 10.0 ** rng.uniform(-12, 2, b.shape))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=20000, help="particles per pcut")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--bench-json", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    mk = lambda **kw: mcs.inputs.build_problem(mcs.inputs.Config(N_PTS_INJ=args.N, N_PTS_PCUT=args.N, N_PTS_PCUT_HI=args.N, num_iterations=2, **kw))
    rg0 = mk().rg0
    prob = mk(XSPEC=tuple(x * rg0 for x in XSPEC_RG))
    P = prob.params
    nm, nd = P.num_psd_mom_bins, len(prob.x_spec)
    hb = hip_backend(prob)
    t0 = time.perf_counter()
    res = mcs.driver.run(prob, hb, n_itrs=1, finalize=True, detectors=True)
    print(f"one iteration of {args.N} protons: {time.perf_counter() - t0:.2f} s; stock binning nmom {nm}, n_grid {P.n_grid}, {nd} detectors at "
          f"{list(XSPEC_RG)} rg0")
    spec = res.detectors[0][2]
    print(f"the run's tallies: diag {spec.diag.tolist()} (live rows, words with now < base, finite gradient words)")
    print(f"  number, shock frame {spec.number[0].tolist()}")
    print(f"  number, plasma frame {spec.number[1].tolist()}")
    print(f"  slope over all bins {spec.slope.tolist()}")
    fin = np.isfinite(spec.gradient)
    print(f"  gradient (1/rg0) at log10 p (cgs) {(0.5 * (spec.mom_log_cgs[:-1] + spec.mom_log_cgs[1:]))[fin[:-1]].round(2).tolist()}: {spec.gradient[fin].tolist()}")
    tabs = cons.consumer_tables(prob, 1)
    call = lambda: hb.detector_spectra(tabs, 0, nm + 1, prob.rg0)
    e = mcs.ensemble.Ensemble.for_backend(hb, 1)
    _, t_tc = timed(hb, args.calls, lambda: hb.tcut_spectra(tabs))
    first, t_det = timed(hb, args.calls, call)
    again = call()
    lit = cons.detector_base(hb, nd)[:, :, :nm + 1]
    print(f"lit words (!= 0) of the run's detector rows: {int((lit != 0).sum())} of {lit.size} in {2 * nd} rows; two calls, the same bits: {same_bits(first, again)}")
    t_add = []
    for r in range(args.calls + 2):
        call()
        hb.sync(); a = time.perf_counter()
        e.add_detectors(hb, 0)
        hb.sync(); b = time.perf_counter()
        if r >= 2:
            t_add.append(b - a)
    dense = {}
    for n_det in (nd, P.n_grid):
        x_rg = XSPEC_RG if n_det == nd else [-3.0 + 0.07 * k for k in range(n_det)]
        light_every_word(hb, prob, x_rg, n_det)
        out, ts = timed(hb, args.calls, call)
        again = call()
        dense[n_det] = ts
        print(f"every word lit, {n_det} detectors: diag {out[1].tolist()}; two calls, the same bits: {same_bits(out, again)}")
    print(f"{args.calls} rounds after 2 warm-up rounds; median (min .. max)")
    print(f"  mcs_tcut_spectra (K12), the run's tallies, {len(prob.tcuts)} cuts          {ms(t_tc)}")
    print(f"  mcs_detector_spectra (K14), the run's tallies, {nd} detectors  {ms(t_det)}")
    print(f"  mcs_detector_spectra (K14), every word lit, {nd} detectors     {ms(dense[nd])}")
    print(f"  mcs_detector_spectra (K14), every word lit, {P.n_grid} detectors    {ms(dense[P.n_grid])}")
    print(f"  mcs_ens_add_detectors + synchronise                         {ms(t_add)}")
    per_end = (statistics.median(t_det) + statistics.median(t_add)) * 1e3
    worst = (statistics.median(dense[nd]) + statistics.median(t_add)) * 1e3
    print(f"per species end: {per_end:.3f} ms (every word lit: {worst:.3f} ms)")
    if args.bench_json:
        line = [ln for ln in open(args.bench_json).read().splitlines() if ln.startswith("{")][-1]
        b = json.loads(line)
        it = b["ms_per_step"]
        print(f"bench.py: {b['config']['workload']}: {it:.1f} ms per iteration (one species, no detector); detectors=True adds {per_end:.3f} ms = "
              f"{100 * per_end / it:.3f} % of it (every word lit: {100 * worst / it:.3f} %)")
    e.destroy(); hb.destroy()


if __name__ == "__main__":
    main()
