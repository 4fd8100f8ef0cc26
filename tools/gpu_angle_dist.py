"""What the pitch-angle distributions cost per species end (profiles/angle_dist.txt): K11, mcs_angle_dist, and the angles sample of
the ensemble statistics, mcs_ens_add_angles, at the stock binning with four momentum windows, beside mcs_dndp_2d (K6: the same
per-cell transform for one frame, with atomics) on the same tallies.
One iteration of N protons through driver.run for real tallies; then on that context, --calls rounds after two warm-up rounds:

  mcs_dndp_2d          HipBackend.dndp_2d into the ISM frame, nothing downloaded (table upload, one launch, wait)
  mcs_angle_dist       HipBackend.angle_dist on the run's own tallies (table upload, one launch, download, wait)
  mcs_ens_add_angles   Ensemble.add_angles on what that call left, ended by a device synchronise

and the two consumer calls again on tallies with EVERY cell of every zone lit (the most a run can ask: the walk costs per lit cell).
Times are host clocks (time.perf_counter) around calls that end in a device synchronise; median and range over the rounds.
Two calls on the same tallies must give the same bits; that is checked on both sets of tallies.
The cost per species end is printed as a share of an iteration of 10^6 protons: --iteration-ms (default: the README's 310 ms), or the
ms_per_step of --bench-json FILE, the JSON line of `python bench.py --gpus 1 ...` taken in another process.
Run on the GPU: python tools/gpu_angle_dist.py [-N 20000] [--calls 40] [--bench-json FILE] [--out profiles/angle_dist.txt]."""
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from conftest import mcs, hip_backend  # noqa: E402

cons = mcs.consumers
ens = mcs.ensemble


def ms(ts):
    ts = [t * 1e3 for t in ts]
    return f"{statistics.median(ts):8.3f} ms  ({min(ts):.3f} .. {max(ts):.3f})"


def same_bits(a, b):
    def words(x):
        x = np.ascontiguousarray(x)
        return np.where(np.isnan(x), 0.0, x).view(np.uint64), np.isnan(x)
    return all(np.array_equal(p, q) for x, y in zip(a, b) for p, q in zip(words(x), words(y)))


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
    ap.add_argument("--iteration-ms", type=float, default=310.0)
    ap.add_argument("--out", default="profiles/angle_dist.txt")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    prob = mcs.inputs.build_problem(mcs.inputs.Config(N_PTS_INJ=args.N, N_PTS_PCUT=args.N, N_PTS_PCUT_HI=args.N, num_iterations=2))
    P = prob.params
    nm, nt, ng = P.num_psd_mom_bins, P.num_psd_tht_bins, P.n_grid
    hb = hip_backend(prob)
    t0 = time.perf_counter()
    mcs.driver.run(prob, hb, n_itrs=1)
    say(f"one iteration of {args.N} protons: {time.perf_counter() - t0:.2f} s; stock binning nmom {nm}, ntht {nt}, n_grid {ng}")
    tabs = cons.consumer_tables(prob, 1)
    x = 10.0 ** ens.bin_centres_log10(prob)
    windows = cons.momentum_windows(prob, [(x[0] * 0.5, x[-1] * 2), (x[nm // 4], x[nm // 2]), (x[nm // 2] * 1.0001, x[3 * nm // 4]), (x[3 * nm // 4] * 1.0001, x[-1] * 2)])
    lo, hi = [w[0] for w in windows], [w[1] for w in windows]
    L = hb.layout
    f, i = hb.read_tallies()
    cells = (nm + 1) * (nt + 1)
    lit = int(((L.view(f, "psd")[:, :nt + 1, :nm + 1] > 1e-66) | (L.view(f, "therm_sf")[:, :nt + 1, :nm + 1] > 1e-66)).sum())
    say(f"windows (momentum bins) {windows}; gam0 = {P.gam0:.6g}; lit cells of the run's tallies: {lit} of {ng} x {cells} = {ng * cells}")
    e = ens.Ensemble.for_backend(hb, 1)
    e.set_angle_windows(lo, hi)
    _, t_2d = timed(hb, args.calls, lambda: hb.dndp_2d(tabs, P.gam0, P.beta0, download=False))
    first, t_ang = timed(hb, args.calls, lambda: hb.angle_dist(tabs, lo, hi))
    again = hb.angle_dist(tabs, lo, hi)
    z = ng - 1
    say(f"the run's tallies: <mu> of the last zone over all momenta, shock / plasma / ISM frame: {first[2][:, z, 0, 0].tolist()}; "
        f"two calls, the same bits: {same_bits(first, again)}")
    t_add = []
    for r in range(args.calls + 2):
        hb.angle_dist(tabs, lo, hi)
        hb.sync(); a = time.perf_counter()
        e.add_angles(hb, 0)
        hb.sync(); b = time.perf_counter()
        if r >= 2:
            t_add.append(b - a)
    # every cell of every zone lit
    rng = np.random.default_rng(1)
    hb.write_tally("psd", 10.0 ** rng.uniform(-20, 5, L.shapes["psd"]))
    _, t_2d_dense = timed(hb, args.calls, lambda: hb.dndp_2d(tabs, P.gam0, P.beta0, download=False))
    dense, t_dense = timed(hb, args.calls, lambda: hb.angle_dist(tabs, lo, hi))
    again = hb.angle_dist(tabs, lo, hi)
    say(f"every cell lit: rows with a number {int((dense[1] > 0).sum())} of {dense[1].size}; two calls, the same bits: {same_bits(dense, again)}")
    say(f"{args.calls} rounds after 2 warm-up rounds; median (min .. max)")
    say(f"  mcs_dndp_2d (K6, one frame), the run's tallies       {ms(t_2d)}")
    say(f"  mcs_angle_dist (K11, three frames), the run's tallies {ms(t_ang)}")
    say(f"  mcs_dndp_2d (K6), every cell lit                     {ms(t_2d_dense)}")
    say(f"  mcs_angle_dist (K11), every cell lit                 {ms(t_dense)}")
    say(f"  mcs_ens_add_angles + synchronise                     {ms(t_add)}")
    per_end = (statistics.median(t_ang) + statistics.median(t_add)) * 1e3
    worst = (statistics.median(t_dense) + statistics.median(t_add)) * 1e3
    say(f"per species end: {per_end:.3f} ms (every cell lit: {worst:.3f} ms)")
    it, what = args.iteration_ms, "the README's iteration of 10^6 protons"
    if args.bench_json:
        line = [ln for ln in open(args.bench_json).read().splitlines() if ln.startswith("{")][-1]
        it, what = json.loads(line)["ms_per_step"], "bench.py's ms_per_step"
    say(f"{what}: {it:.1f} ms (one species); angles=[...] adds {per_end:.3f} ms = {100 * per_end / it:.3f} % of it (every cell lit: {100 * worst / it:.3f} %)")
    e.destroy(); hb.destroy()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
