"""What a convergence check costs (profiles/ensemble_summary.txt): one Ensemble.summarize of all named parts of a species slot on the
stock binning, against the same numbers obtained the way they were before there was a device summary -- mean and standard error of
every part through mcs_ens_read, reduced in numpy.  Run on the GPU: python tools/gpu_ens_summary.py [--calls N] [--no-parent].
Times are host clocks around calls that end in a device synchronise.  "cold": 512 MB are written on the device between two calls, so
that mean and M2 (123 MB, which fit the 256 MB Infinity Cache) come from HBM, as they do in a run, where an iteration of transport
lies between two checks."""
import argparse
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from conftest import mcs, make_problem, hip_backend  # noqa: E402

ITERATION_MS = 314.0          # one iteration of the headline workload (profiles/r04_bench_line.json)


def the_old_way(e, slot, reqs, n):
    out = []
    for q in reqs:
        mean, se = e.mean(slot, q.name).ravel(), e.stderr(slot, q.name).ravel()
        ok = np.isfinite(mean) & np.isfinite(se)                    # (a non-finite M2 shows in the standard error)
        a = np.abs(mean)
        amax = a[ok].max() if ok.any() else 0.0
        sel = ok & (a > 0) & (a >= q.floor_frac * amax)
        rel = se[sel] / a[sel]
        k = int(np.argmax(rel)) if rel.size else -1
        out.append((amax, rel[k] if rel.size else 0.0, int(np.flatnonzero(sel)[k]) if rel.size else -1, int(sel.sum()), int((rel > q.tol).sum()),
                    int((~ok).sum()), float(se[sel].sum()), float(a[sel].sum()), float((rel * rel).sum())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--no-parent", action="store_true")
    args = ap.parse_args()
    import torch
    ens = mcs.ensemble
    prob = make_problem(64)
    hb = hip_backend(prob)
    L = hb.layout
    e = ens.HipEnsemble(hb, 1)
    for k in range(5):
        rng = np.random.default_rng(k)
        f = rng.uniform(1.0, 10.0, L.total) * 10.0 ** rng.integers(-60, 40, L.total)
        hb.write_tallies(f, rng.integers(0, 2 ** 50, L.n_i64))
        e.add_species(hb, 0)
    reqs = [ens.Request(name, None, 1e-3, 0.05) for name in ens.SPECIES_NAMES]
    words = sum(e.word_range(0, q.name)[1] for q in reqs)
    nbytes = 3 * 8 * words            # sweep 1 reads the means, sweep 2 means and M2
    print(f"{len(reqs)} ranges, {words} words of a species slot of {e.layout.species_total}; two sweeps read {nbytes / 1e6:.1f} MB")
    flush = torch.empty(512 * 2 ** 20, dtype=torch.uint8, device="cuda")

    def timed(cold):
        ts = []
        for k in range(5 + args.calls):
            if cold:
                flush.add_(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = e.summarize(0, reqs)
            ts.append((time.perf_counter() - t0) * 1e6)
        return ts[5:], got
    for cold in (False, True):
        ts, got = timed(cold)
        med = statistics.median(ts)
        print(f"summarize, {'cold' if cold else 'warm'}: median {med:.1f} us, min {min(ts):.1f} us, max {max(ts):.1f} us over {len(ts)} calls -> "
              f"{nbytes / med / 1e3:.0f} GB/s at the median; {med / 1e3 / ITERATION_MS * 100:.4f} % of an iteration of {ITERATION_MS:.0f} ms")
    if args.no_parent:
        return
    ts = []
    for k in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        old = the_old_way(e, 0, reqs, 5)
        ts.append((time.perf_counter() - t0) * 1e3)
    print(f"mean + stderr through mcs_ens_read and numpy: {', '.join(f'{t:.1f}' for t in ts)} ms (the first call warms up); "
          f"{2 * 8 * words / 1e6:.1f} MB cross to the host; {statistics.median(ts[1:]) / ITERATION_MS * 100:.1f} % of an iteration")
    for q, s, o in zip(reqs, got, old):
        assert (s.amax, s.max_rel, s.argmax, s.n_selected, s.n_over, s.n_nonfinite) == o[:6], (q, s, o)
        assert np.allclose([s.sum_se, s.sum_abs_mean, s.sum_rel2], o[6:], rtol=1e-12)
    print("both ways give the same numbers (the exact fields equal, the sums to 1e-12)")
    e.destroy(); hb.destroy()


if __name__ == "__main__":
    main()
