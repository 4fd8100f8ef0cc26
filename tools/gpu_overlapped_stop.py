"""What the stop rule of an overlapped run costs (profiles/overlapped_stop.txt), on the GPU, in two steps that each run under a time
limit of their own:

  timeout -k 10 600 python tools/gpu_overlapped_stop.py --part rounds && timeout -k 10 300 python tools/gpu_overlapped_stop.py --part summary

rounds    ms per iteration of driver.run_overlapped at 10^6 protons on the stock binning with K = 3 contexts: free-running (every
          iteration submitted up front) against in rounds of K with a barrier and one check per round -- a trigger on psd whose
          threshold cannot be met, so the run goes to its cap.  Both with ensemble=True (the rounds need it; the accumulators are
          created inside the timed call in both legs); free-running without an ensemble is printed beside them.  The legs take
          turns, in an order that rotates from one repetition to the next (a drift of clocks or of the growing never-reset tallies is
          then charged to every leg alike), every leg runs the same iterations, the median over --reps is reported.
summary   one mcs_ens_summarize_merged of the psd part over 3 accumulators against what it replaces: the three merged into a spare
          accumulator (one device copy and two mcs_ens_merge) followed by mcs_ens_summarize.  Host clocks around calls that end in
          a device synchronise.  "cold": 512 MB are written on the device before every call, so that the vectors come from HBM, as
          they do in a run, where a round of transport lies between two checks.  The spare accumulator of the old way is created
          outside the clock (a run would keep it: 123 MB per species slot)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from conftest import mcs, make_problem, hip_backend  # noqa: E402

K = 3


def rounds_part(args):
    import torch
    ens = mcs.ensemble
    n, warm = args.rounds * K, K
    prob = make_problem(args.particles, num_iterations=warm + n)
    bes = [hip_backend(prob) for _ in range(K)]
    never = ens.Trigger(0, "psd", "max", 1e-12)
    mcs.driver.run_overlapped(prob, bes, n_itrs=warm)                # warm every context
    legs = {"free-running, no ensemble": dict(), "free-running, ensemble=True": dict(ensemble=True),
            "rounds of 3, one check per round": dict(ensemble=True, triggers=[never])}
    ms = {name: [] for name in legs}
    order = list(legs)
    for rep in range(args.reps):
        for name in order[rep % len(order):] + order[:rep % len(order)]:
            kw = legs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = mcs.driver.run_overlapped(prob, bes, n_itrs=n, first_iter=warm + 1, **kw)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / n * 1e3)
            if res.convergence is not None:
                c = res.convergence
                assert c.stopped_at == warm + n and not c.satisfied and len(c.checks) == args.rounds
            if res.ensemble is not None:
                res.ensemble.destroy()
            print(f"rep {rep}  {name}: {ms[name][-1]:.1f} ms per iteration", flush=True)
    print(f"{args.particles} protons, stock binning, K = {K} contexts, {n} iterations per run ({args.rounds} rounds), {args.reps} runs per leg")
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name, v in ms.items():
        print(f"{name}: median {med[name]:.1f} ms per iteration (min {min(v):.1f}, max {max(v):.1f})")
    free, rnd = med["free-running, ensemble=True"], med["rounds of 3, one check per round"]
    print(f"the round barrier and its check cost {rnd - free:.1f} ms per iteration, {(rnd / free - 1) * 100:.1f} % of the free-running figure")
    for be in bes:
        be.destroy()


def summary_part(args):
    import torch
    ens = mcs.ensemble
    prob = make_problem(64)
    hb = hip_backend(prob)
    L = hb.layout
    parts = [ens.HipEnsemble(hb, 1) for _ in range(K)]
    for k in range(2 * K):
        rng = np.random.default_rng(k)
        f = rng.uniform(1.0, 10.0, L.total) * 10.0 ** rng.integers(-60, 40, L.total)
        hb.write_tallies(f, rng.integers(0, 2 ** 50, L.n_i64))
        parts[k % K].add_species(hb, 0)
    reqs = [ens.Request("psd", None, 1e-3, 0.05)]
    words = parts[0].word_range(0, "psd")[1]
    total = parts[0].layout.species_total
    print(f"psd: {words} words of a species slot of {total}.  The merged summary over {K} accumulators reads {3 * K * 8 * words / 1e6:.0f} MB in its "
          f"two sweeps and writes block partials only; the old way moves {(4 + 2 * 6) * 8 * total / 1e6:.0f} MB for the copy and the two merges of "
          f"the whole slot and reads {3 * 8 * words / 1e6:.0f} MB in the summary")
    flush = torch.empty(512 * 2 ** 20, dtype=torch.uint8, device="cuda")

    def clock(call, cold, before=None):
        if before is not None:
            before()
        if cold:
            flush.add_(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = call()
        return (time.perf_counter() - t0) * 1e6, got
    for cold in (False, True):
        ts = [clock(lambda: parts[0].summarize_merged(parts[1:], 0, reqs), cold) for _ in range(5 + args.calls)][5:]
        us = [t for t, _ in ts]
        new = ts[-1][1]
        print(f"merged summary, {'cold' if cold else 'warm'}: median {statistics.median(us):.1f} us, min {min(us):.1f}, max {max(us):.1f} over {len(us)} calls")
        spare = []

        def fresh():
            while spare:
                spare.pop().destroy()
            spare.append(ens.HipEnsemble(hb, 1))

        def old_way():
            for e in parts:
                spare[0].merge(e)
            return spare[0].summarize(0, reqs)
        ts = [clock(old_way, cold, fresh) for _ in range(2 + args.old_calls)][2:]
        us = [t for t, _ in ts]
        print(f"copy + 2 merges into a spare accumulator + summarize, {'cold' if cold else 'warm'}: median {statistics.median(us):.1f} us, "
              f"min {min(us):.1f}, max {max(us):.1f} over {len(us)} calls")
        assert ts[-1][1] == new, "the two ways differ"
        while spare:
            spare.pop().destroy()
    print("both ways give the same summary, bit for bit")
    for e in parts:
        e.destroy()
    hb.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("rounds", "summary"), required=True)
    ap.add_argument("--particles", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--old-calls", type=int, default=8)
    args = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    try:
        commit = subprocess.run(["git", "-C", here, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown (not a git checkout)"
    print(f"commit {commit}\ncommand: python {' '.join(sys.argv)}", flush=True)
    (rounds_part if args.part == "rounds" else summary_part)(args)


if __name__ == "__main__":
    main()
