"""One iteration of bench.py --mixed (p + He + e-, radiative losses, ion -> electron energy transfer) with the species one after the
other on one context, and with He on a second context beside the protons (driver.run(..., species_backends=[...])), alternated in
one process after a warm-up of both: median ms per iteration of each path, kernel ms per species, and how long the two ions overlapped.
usage: python tools/gpu_species_concurrent.py [N per species, default 1000000] [fp32]"""
import statistics
import sys
import time

sys.path.insert(0, "tests")
from conftest import mcs
from mcs_amd import hip_backend


def main(N, fp32, warm=1, reps=5):
    me_mp = mcs.constants.ME / mcs.constants.MP
    cfg = mcs.inputs.Config(N_PTS_INJ=N, N_PTS_PCUT=N, N_PTS_PCUT_HI=N, num_iterations=2 * (warm + reps),
                            species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(4.0, 2.0, 1e6, 0.1),
                                     mcs.inputs.Species(me_mp, -1.0, 1e6, 1.2)],
                            energy_transfer_frac=0.1, radiation_losses=True, state_fp32=fp32)
    prob = mcs.inputs.build_problem(cfg)
    prim, sec = hip_backend.HipBackend(0), hip_backend.HipBackend(0)
    prim.create(prob); sec.create(prob)
    rows = {"sequential": [], "concurrent": []}
    it = 1
    for k in range(warm + reps):
        for path in ("sequential", "concurrent"):
            t0 = time.perf_counter()
            res = mcs.driver.run(prob, prim, None, n_itrs=1, first_iter=it, species_tallies="light", final_full_read=False,
                                 species_backends=[sec] if path == "concurrent" else None)
            ms = (time.perf_counter() - t0) * 1e3
            it += 1
            if k < warm:
                continue
            kern = [sum(s.kernel_ms for s in res.stats if s.i_ion == ion) for ion in (1, 2, 3)]
            sp = {ion: (t0, t1) for _, ion, _, t0, t1 in res.species_spans}
            ov = max(0.0, min(sp[1][1], sp[2][1]) - max(sp[1][0], sp[2][0])) * 1e3 if sp else 0.0
            rows[path].append((ms, kern, ov, [(t1 - t0) * 1e3 for t0, t1 in sp.values()]))
    prim.destroy(); sec.destroy()
    med = lambda xs: statistics.median(xs)
    out = {}
    for path, r in rows.items():
        out[path] = med([x[0] for x in r])
        kern = [med([x[1][j] for x in r]) for j in range(3)]
        line = (f"{'fp32' if fp32 else 'fp64'} N={N} {path:10s}: {out[path]:7.1f} ms per iteration (median of {len(r)}; all "
                f"{', '.join(f'{x[0]:.0f}' for x in r)}); kernel ms p {kern[0]:.1f}, He {kern[1]:.1f}, e- {kern[2]:.1f}")
        if path == "concurrent":
            spans = [med([x[3][j] for x in r]) for j in range(3)]
            line += (f"; p and He overlapped {med([x[2] for x in r]):.1f} ms; host spans p {spans[0]:.1f}, He {spans[1]:.1f}, "
                     f"e- {spans[2]:.1f} ms")
        print(line, flush=True)
    print(f"{'fp32' if fp32 else 'fp64'} N={N}: concurrent / sequential = {out['concurrent'] / out['sequential']:.3f}", flush=True)
    return out


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1000000, "fp32" in sys.argv[2:])
