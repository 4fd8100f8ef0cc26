"""What the escape spectra cost per species end (profiles/escape_spectra.txt): K10, mcs_dndp_esc, and the escape sample of the
ensemble statistics, mcs_ens_add_escape, at the stock binning, beside mcs_dndp_cr (K4) in the same run.
One iteration of N protons through driver.run for real tallies; then on that context, --calls rounds after two warm-up rounds:

  mcs_dndp_cr          consumers' get_dNdp_cr of all zones (HipBackend.dndp_cr: table upload, one launch, download, wait)
  mcs_dndp_esc         HipBackend.dndp_esc on the run's own escape slabs (table upload, two launches, download, wait)
  mcs_ens_add_escape   Ensemble.add_escape on what that call left, ended by a device synchronise

and mcs_dndp_esc again on slabs with EVERY cell of the written extent lit (the most a run can ask of it: the row walk costs per lit
cell).  Times are host clocks (time.perf_counter) around calls that end in a device synchronise; median and range over the rounds.
Two calls on the same tallies must give the same bits; that is checked on both sets of slabs.
--bench-json FILE: the JSON line of `python bench.py --gpus 1 ...` taken in another process; the cost per species end is then
printed as a share of its ms_per_step.
Run on the GPU: python tools/gpu_escape_spectra.py [-N 20000] [--calls 40] [--bench-json FILE]."""
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
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)) for x, y in zip(a[:2], b[:2])) \
        and np.array_equal(a[2], b[2])


def timed(hb, calls, fn):
    out, ts = None, []
    for r in range(calls + 2):                       # (two warm-up rounds)
        hb.sync(); t0 = time.perf_counter()
        out = fn()
        hb.sync(); t1 = time.perf_counter()
        if r >= 2:
            ts.append(t1 - t0)
    return out, ts


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
    nm, nt = P.num_psd_mom_bins, P.num_psd_tht_bins
    hb = hip_backend(prob)
    t0 = time.perf_counter()
    mcs.driver.run(prob, hb, n_itrs=1)
    print(f"one iteration of {args.N} protons: {time.perf_counter() - t0:.2f} s; stock binning nmom {nm}, ntht {nt}, n_grid {P.n_grid}")
    tabs = cons.consumer_tables(prob, 1)
    gam_pf = cons.escape_gam_pf(prob)
    L = hb.layout
    f, _ = hb.read_tallies()
    slabs = [L.view(f, name)[:nt + 1, :nm + 1] for name in ("esc_psd_up", "esc_psd_down")]
    print(f"gam_pf = ({gam_pf[0]:.6g}, {gam_pf[1]:.6g}), gam0 = {P.gam0:.6g}; lit cells (>= 1e-66) of the run's slabs: up {int((slabs[0] >= 1e-66).sum())}, "
          f"down {int((slabs[1] >= 1e-66).sum())} of {(nm + 1) * (nt + 1)} each")
    e = mcs.ensemble.Ensemble.for_backend(hb, 1)
    e.set_slope_window(0, nm + 1, mcs.ensemble.bin_centres_log10(prob))
    _, t_cr = timed(hb, args.calls, lambda: hb.dndp_cr(tabs))
    first, t_esc = timed(hb, args.calls, lambda: hb.dndp_esc(tabs, gam_pf))
    again = hb.dndp_esc(tabs, gam_pf)
    print(f"the run's slabs: number {first[1].ravel().tolist()}, diag {first[2].ravel().tolist()}; two calls, the same bits: {same_bits(first, again)}")
    t_add = []
    for r in range(args.calls + 2):
        hb.dndp_esc(tabs, gam_pf)
        hb.sync(); a = time.perf_counter()
        e.add_escape(hb, 0)
        hb.sync(); b = time.perf_counter()
        if r >= 2:
            t_add.append(b - a)
    # every cell of the written extent lit
    rng = np.random.default_rng(1)
    for name in ("esc_psd_up", "esc_psd_down"):
        s = np.full(L.shapes[name], 1.0e-99)
        s[:nt + 2, :nm + 2] = 10.0 ** rng.uniform(-20, 5, (nt + 2, nm + 2))
        hb.write_tally(name, s)
    dense, t_dense = timed(hb, args.calls, lambda: hb.dndp_esc(tabs, gam_pf))
    again = hb.dndp_esc(tabs, gam_pf)
    print(f"every cell lit: diag {dense[2].ravel().tolist()}; two calls, the same bits: {same_bits(dense, again)}")
    print(f"{args.calls} rounds after 2 warm-up rounds; median (min .. max)")
    print(f"  mcs_dndp_cr (K4, {P.n_grid} zones)                  {ms(t_cr)}")
    print(f"  mcs_dndp_esc (K10), the run's slabs            {ms(t_esc)}")
    print(f"  mcs_dndp_esc (K10), every cell lit             {ms(t_dense)}")
    print(f"  mcs_ens_add_escape + synchronise               {ms(t_add)}")
    per_end = (statistics.median(t_esc) + statistics.median(t_add)) * 1e3
    worst = (statistics.median(t_dense) + statistics.median(t_add)) * 1e3
    print(f"per species end: {per_end:.3f} ms (every cell lit: {worst:.3f} ms)")
    if args.bench_json:
        line = [ln for ln in open(args.bench_json).read().splitlines() if ln.startswith("{")][-1]
        b = json.loads(line)
        it = b["ms_per_step"]
        print(f"bench.py: {b['config']['workload']}: {it:.1f} ms per iteration (one species); escape=True adds {per_end:.3f} ms = {100 * per_end / it:.3f} % of it "
              f"(every cell lit: {100 * worst / it:.3f} %)")
    e.destroy(); hb.destroy()


if __name__ == "__main__":
    main()
