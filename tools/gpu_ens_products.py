"""What a products sample and a check on a products slot cost (profiles/ensemble_products.txt): at the bench problem's shape (the
stock binning sets the sizes), one mcs_ens_add_products -- the slope kernel and the update of 3 n_grid (nmom + 2) + 6 n_grid words --
and one Ensemble.summarize of a products slot with 256 single-zone momentum windows.  Run on the GPU:
python tools/gpu_ens_products.py [--calls N] [--out FILE].
The sample is queued without a host synchronisation: its time is the host clock from the call to the end of a device synchronise
that follows it, the consumers' own synchronise having drained the stream before.  The summary ends in its own synchronise.  "cold":
512 MB are written on the device before a call, so that nothing it reads lies in the Infinity Cache."""
import argparse
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from conftest import mcs, make_problem, hip_backend  # noqa: E402

# per-iteration time of run_overlapped(ensemble=True) before the products sample existed: profiles/overlapped_stop.txt, section 1,
# "free-running, ensemble=True", 10^6 protons with three contexts
PARENT_ITERATION_MS = 236.8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    import torch
    ens = mcs.ensemble
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    prob = make_problem(64)
    P = prob.params
    ng, NM = P.n_grid, P.num_psd_mom_bins + 2
    hb = hip_backend(prob)
    L = hb.layout
    tabs = mcs.consumers.consumer_tables(prob, 1)
    e = ens.HipEnsemble(hb, 1)
    l_lo, l_hi, x_log = 0, NM - 1, ens.bin_centres_log10(prob)
    e.set_slope_window(l_lo, l_hi, x_log)
    ps = e.products_slot(0)
    total = e.layout.products_total
    say(f"n_grid {ng}, nmom + 2 = {NM}: a products sample has {total} words ({total * 8 / 1e3:.0f} kB; mean and M2 {2 * total * 8 / 1e3:.0f} kB); "
        f"slope window [{l_lo}, {l_hi})")
    rng = np.random.default_rng(0)
    f = rng.uniform(1.0, 10.0, L.total) * 10.0 ** rng.integers(-20, 20, L.total)
    hb.write_tallies(f, rng.integers(0, 2 ** 20, L.n_i64))
    flush = torch.empty(512 * 2 ** 20, dtype=torch.uint8, device="cuda")

    def sample(cold):
        ts = []
        for k in range(5 + args.calls):
            hb.dndp_cr(tabs); hb.thermo_calcs(tabs)          # (each ends in a synchronise of the context's stream)
            if cold:
                flush.add_(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.add_products(hb, 0)
            hb.sync()
            ts.append((time.perf_counter() - t0) * 1e6)
        return ts[5:]
    for cold in (False, True):
        ts = sample(cold)
        med = statistics.median(ts)
        say(f"mcs_ens_add_products + synchronise, {'cold' if cold else 'warm'}: median {med:.1f} us, min {min(ts):.1f}, max {max(ts):.1f} over {len(ts)} calls; "
            f"{med / 1e3 / PARENT_ITERATION_MS * 100:.4f} % of an iteration of {PARENT_ITERATION_MS:.1f} ms")
    # 256 single-zone momentum windows: dNdp_pf and dNdp_sf, bins 60..110 of the zones that fit
    reqs = [ens.Request(name, (z, z + 1), 1e-3, 0.05, (60, 110)) for name in ("dNdp_pf", "dNdp_sf") for z in range(ng)][:ens.MAX_RANGES]
    reqs += [ens.Request("dNdp_isf", (z, z + 1), 1e-3, 0.05, (60, 110)) for z in range(ens.MAX_RANGES - len(reqs))]
    assert len(reqs) == ens.MAX_RANGES
    words = sum(e.word_range(ps, q.name, q.zones, q.bins)[1] for q in reqs)
    say(f"{len(reqs)} ranges of {reqs[0].bins[1] - reqs[0].bins[0]} words each, {words} words in all, of a products slot with {e.count(ps)} samples")
    for cold in (False, True):
        ts = []
        for k in range(5 + args.calls):
            if cold:
                flush.add_(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = e.summarize(ps, reqs)
            ts.append((time.perf_counter() - t0) * 1e6)
        ts = ts[5:]
        med = statistics.median(ts)
        say(f"summarize of 256 momentum windows, {'cold' if cold else 'warm'}: median {med:.1f} us, min {min(ts):.1f}, max {max(ts):.1f} over {len(ts)} calls; "
            f"{med / 1e3 / PARENT_ITERATION_MS * 100:.4f} % of an iteration of {PARENT_ITERATION_MS:.1f} ms")
    say(f"(selected words over the 256 ranges: {sum(s.n_selected for s in got)}; non-finite: {sum(s.n_nonfinite for s in got)})")
    # the library call alone, its arguments built beforehand: what of the figure above is Python (256 word ranges, 256 Summary objects)
    rs = (mcs.capi.McsEnsRange * len(reqs))(*[mcs.capi.McsEnsRange(*(e.word_range(ps, q.name, q.zones, q.bins) + (q.floor_frac, q.tol))) for q in reqs])
    out = (mcs.capi.McsEnsSummary * len(reqs))()
    ts = []
    for k in range(5 + args.calls):
        flush.add_(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = e.lib.mcs_ens_summarize(e.h, ps, len(reqs), rs, out)
        ts.append((time.perf_counter() - t0) * 1e6)
        assert rc == 0
    ts = ts[5:]
    say(f"mcs_ens_summarize of the same 256 ranges alone, cold: median {statistics.median(ts):.1f} us, min {min(ts):.1f}, max {max(ts):.1f} over {len(ts)} calls")
    assert [o.n_selected for o in out] == [s.n_selected for s in got] and [o.max_rel for o in out] == [s.max_rel for s in got]
    say(f"reference: {PARENT_ITERATION_MS:.1f} ms per iteration of run_overlapped(ensemble=True) before this sample existed "
        f"(profiles/overlapped_stop.txt, 10^6 protons, three contexts)")
    e.destroy(); hb.destroy()
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
