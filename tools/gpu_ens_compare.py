"""Does run B agree with run A within their error bars?  (profiles/ensemble_compare.txt)  Three fixed-profile ensembles of K
iterations each at N particles per species: fp64 over iterations 1..K, fp64 over iterations K+1..2K -- a null pair: the same
configuration, other random numbers -- and the fp32-state variant over iterations 1..K.  Prints the Difference
(ensemble.Ensemble.compare, one mcs_ens_compare call per slot) of the marginals and of the products for the null pair and for
fp64 against fp32, and what one comparison of a whole species slot costs beside what it replaces: the mean and M2 of both slots
through four mcs_ens_read calls, compared in numpy.
Run on the GPU: python tools/gpu_ens_compare.py [-N 20000] [-K 5] [--pcuts P] [--calls C].
Times are host clocks around calls that end in a device synchronise.  "cold": 512 MB are written on the device between two calls, so
that the four vectors (246 MB on the stock binning, about the size of the 256 MB Infinity Cache) come from HBM."""
import argparse
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from conftest import mcs, make_problem, hip_backend  # noqa: E402


def the_old_way(a, b, slot, reqs):
    """The same numbers from the vectors read back: plain numpy, its pairwise sums."""
    total = a._len(slot)
    ma, qa, mb, qb = a._read(slot, 0, 0, total), a._read(slot, 1, 0, total), b._read(slot, 0, 0, total), b._read(slot, 1, 0, total)
    n_a, n_b = a.count(slot), b.count(slot)
    out = []
    for q in reqs:
        first, count = a.word_range(slot, q.name, q.zones, q.bins)
        s_ = slice(first, first + count)
        with np.errstate(all="ignore"):
            s2 = qa[s_] / (float(n_a) * float(n_a - 1)) + qb[s_] / (float(n_b) * float(n_b - 1))
            d = ma[s_] - mb[s_]
            scale = np.maximum(np.abs(ma[s_]), np.abs(mb[s_]))
            ok = np.isfinite(ma[s_]) & np.isfinite(qa[s_]) & np.isfinite(mb[s_]) & np.isfinite(qb[s_]) & np.isfinite(d) & np.isfinite(s2)
            amax = scale[ok].max() if ok.any() else 0.0
            sel = ok & (scale > 0) & (scale >= q.floor_frac * amax)
            keep = sel & ~((s2 == 0) & (d != 0))
            z = np.where(s2[keep] == 0, 0.0, d[keep] / np.sqrt(s2[keep]))
        az = np.abs(z)
        out.append((amax, az.max() if az.size else 0.0, int(np.flatnonzero(keep)[np.argmax(az)]) if az.size else -1, int(sel.sum()),
                    int((az > q.zcut).sum()), int((~ok).sum()), int(sel.sum() - keep.sum()), float(z.sum()), float(az.sum()), float((z * z).sum()),
                    float(np.abs(d[sel]).sum()), float(scale[sel].sum())))
    return out


def show(title, reqs, diffs):
    print(title)
    print(f"  {'part':<20}{'selected':>9}{'degen':>6}{'nonfin':>7}{'max |z|':>10}{'at':>8}{'over':>7}{'chi2/word':>11}{'mean z':>9}{'sum|d|/sum scale':>18}")
    for q, d in zip(reqs, diffs):
        n = d.n_selected - d.n_degenerate
        chi2, mean_z = (d.sum_z2 / n, d.sum_z / n) if n > 0 else (float("nan"), float("nan"))
        wd = d.sum_abs_diff / d.sum_scale if d.n_selected else float("nan")
        name = q.name + ("" if q.zones is None else f"[{q.zones[0]}:{q.zones[1]}]")
        print(f"  {name:<20}{d.n_selected:>9}{d.n_degenerate:>6}{d.n_nonfinite:>7}{d.max_abs_z:>10.3f}{d.argmax:>8}{d.n_over:>7}{chi2:>11.3f}{mean_z:>9.3f}{wd:>18.4e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=20000, help="particles per species and pcut")
    ap.add_argument("-K", type=int, default=5, help="iterations of every ensemble")
    ap.add_argument("--pcuts", type=int, default=None, help="pcuts per species (all by default)")
    ap.add_argument("--calls", type=int, default=30)
    args = ap.parse_args()
    import torch
    ens = mcs.ensemble
    K = args.K
    runs = {}
    for name, fp32, first in (("fp64, iterations 1..K", False, 1), ("fp64, iterations K+1..2K", False, K + 1), ("fp32 state, iterations 1..K", True, 1)):
        prob = make_problem(args.N, state_fp32=fp32, num_iterations=2 * K)
        hb = hip_backend(prob)
        e = ens.Ensemble.for_backend(hb, 1)
        t0 = time.perf_counter()
        mcs.driver.run(prob, hb, n_itrs=K, max_pcuts=args.pcuts, ensemble=e, first_iter=first, finalize=True)
        print(f"{name}: N = {args.N}, K = {K}, {time.perf_counter() - t0:.1f} s")
        runs[name] = (prob, hb, e)
    (prob, hb_a, a), (_, _, b), (_, _, c) = runs.values()
    ng = prob.params.n_grid
    ps = a.products_slot(0)
    marg = [ens.CompareRequest(name, None, 1e-3, 3.0) for name in ens.MARGINALS] + [ens.CompareRequest("psd_mom", (ng - 10, ng), 1e-6, 3.0)]
    prod = [ens.CompareRequest(name, None, 1e-6 if name.startswith("dNdp") else 0.0, 3.0) for name in ens.PRODUCT_NAMES]
    print(f"z = (mean_a - mean_b) / sqrt(se_a^2 + se_b^2) per word; with {K} samples a side z follows Welch's t: under the null E[z^2] = nu / (nu - 2), "
          f"nu between {K - 1} and {2 * K - 2}; zcut = 3, floor_frac = 1e-3 (marginals), 1e-6 (dN/dp), 0 (the rest)")
    for title, other in (("== the null pair: fp64 1..K against fp64 K+1..2K ==", b), ("== fp64 1..K against fp32 state 1..K ==", c)):
        show(title + " marginals (species slot 0)", marg, a.compare(other, 0, marg))
        show(title + " products", prod, a.compare(other, ps, prod))
    # the cost of one comparison of a whole species slot
    reqs = [ens.CompareRequest(name, None, 1e-3, 3.0) for name in ens.SPECIES_NAMES]
    words = sum(a.word_range(0, q.name)[1] for q in reqs)
    assert words == a.layout.species_total
    nbytes = 2 * 32 * words            # both sweeps read mean and M2 of both slots
    print(f"== cost == {len(reqs)} ranges, the {words} words of a species slot; two sweeps read {nbytes / 1e6:.1f} MB")
    flush = torch.empty(512 * 2 ** 20, dtype=torch.uint8, device="cuda")
    for cold in (False, True):
        ts = []
        for k in range(5 + args.calls):
            if cold:
                flush.add_(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = a.compare(b, 0, reqs)
            ts.append((time.perf_counter() - t0) * 1e6)
        ts = ts[5:]
        med = statistics.median(ts)
        print(f"compare, {'cold' if cold else 'warm'}: median {med:.1f} us, min {min(ts):.1f} us, max {max(ts):.1f} us over {len(ts)} calls -> "
              f"{nbytes / med / 1e3:.0f} GB/s at the median")
    ts = []
    for k in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        old = the_old_way(a, b, 0, reqs)
        ts.append((time.perf_counter() - t0) * 1e3)
    print(f"four mcs_ens_read calls and numpy: {', '.join(f'{t:.1f}' for t in ts)} ms (the first call warms up); {4 * 8 * words / 1e6:.1f} MB cross to the host")
    for q, d, o in zip(reqs, got, old):
        assert (d.amax, d.max_abs_z, d.argmax, d.n_selected, d.n_over, d.n_nonfinite, d.n_degenerate) == o[:7], (q, d, o)
        assert np.allclose([d.sum_z, d.sum_abs_z, d.sum_z2, d.sum_abs_diff, d.sum_scale], o[7:], rtol=1e-9, atol=1e-9 * d.sum_abs_z)
    print("both ways give the same numbers (the exact fields equal, the sums to 1e-9)")
    for _, hb, e in runs.values():
        e.destroy(); hb.destroy()


if __name__ == "__main__":
    main()
