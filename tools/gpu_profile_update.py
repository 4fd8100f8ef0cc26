"""What the shock-profile update costs per iteration (profiles/profile_update.txt): K13, mcs_profile_update, and the profile sample of
the ensemble statistics, mcs_ens_add_profile, at the stock grid, beside the numpy iter_finalize on the same inputs in the same run.
One iteration of N protons through driver.run(finalize=True) for real tallies and pressures; then on that context, --calls rounds
after two warm-up rounds:

  mcs_profile_update            HipBackend.profile_update on the run's fluxes, scalars and resident pressures (table upload, one
                                launch of one workgroup, two downloads, wait)
  mcs_profile_update, classical the same call on the classical crafted base case of tests/profile_common.py through the pressures
                                pointer, on a context of that problem (Newton iterations, lanes diverging by step count)
  mcs_ens_add_profile           Ensemble.add_profile on what the call left, ended by a device synchronise
  iter_finalize (numpy)         iter_finalize.iter_finalize with smooth_shocks on a copy of the problem, on the tallies read back

Times are host clocks (time.perf_counter) around calls that end in a device synchronise; median and range over the rounds.  Two
calls on the same buffers must give the same bits; that is checked.  The call is bound by its launch, its copies and its wait,
not by arithmetic: one workgroup, 99 zones.
--bench-json FILE: the JSON line of `python bench.py --gpus 1 ...` taken in another process; the cost per iteration is then printed
as a share of its ms_per_step.
Run on the GPU: python tools/gpu_profile_update.py [-N 20000] [--calls 40] [--bench-json FILE]."""
import argparse
import copy
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, "tests")
from conftest import mcs, hip_backend  # noqa: E402
import profile_common as pc  # noqa: E402

cons = mcs.consumers
itf = mcs.iter_finalize


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=20000, help="particles per pcut")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--bench-json", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    prob = mcs.inputs.build_problem(mcs.inputs.Config(N_PTS_INJ=args.N, N_PTS_PCUT=args.N, N_PTS_PCUT_HI=args.N))
    P = prob.params
    hb = hip_backend(prob)
    t0 = time.perf_counter()
    res = mcs.driver.run(prob, hb, n_itrs=1, finalize=True)
    print(f"one iteration of {args.N} protons: {time.perf_counter() - t0:.2f} s; stock grid n_grid {P.n_grid}, i_shock {P.i_shock}")
    (_, fin, ion), = res.iter_finals
    pres = (ion.P_psd_par, ion.P_psd_perp, ion.energy_density_psd)
    sm = itf.SmoothingConfig(smooth_shocks=True, SMMOE=0.4)
    pin = cons.profile_in(prob, res.iter_state, sm, 1)
    first, t_call = timed(hb, args.calls, lambda: hb.profile_update(pin, None))
    again = hb.profile_update(pin, None)
    upd = cons._profile_from_words(first[0], first[1], P.n_grid, pin.settings())
    print(f"the run's tallies: diag {first[1].tolist()}, shift_rms {upd.shift_rms:.6e}, gamma_down {upd.gamma_down:.6f}; two calls, the same bits: {same_bits(first, again)}")
    e = mcs.ensemble.Ensemble.for_backend(hb, 1)
    t_add = []
    for r in range(args.calls + 2):
        hb.profile_update(pin, None)
        hb.sync(); a = time.perf_counter()
        e.add_profile(hb)
        hb.sync(); b = time.perf_counter()
        if r >= 2:
            t_add.append(b - a)
    f, _ = hb.read_tallies()
    t_host = []
    for r in range(args.calls + 2):
        mine, st = copy.deepcopy(prob), itf.IterState.create(prob, sm, 1)
        a = time.perf_counter()
        itf.iter_finalize(mine, st, sm, 1, f, hb.layout, *pres)
        b = time.perf_counter()
        if r >= 2:
            t_host.append(b - a)
    d = float(np.max(np.abs(upd.ux_next / mine.ux[1:P.n_grid + 1] - 1)))
    print(f"ux_next against the numpy iter_finalize on the same inputs: largest relative difference {d:.3e}")
    e.destroy(); hb.destroy()
    # the classical crafted case, on a context of that problem
    cprob = pc.classical_problem()
    hc = hip_backend(cprob)
    hc.begin_iteration(1)
    hc.begin_species(1, 1, 1.0, 1.0, cprob.pmax, 1.0, 1.0)
    c = pc.make_cases(cprob)[0][1]
    _, i = hc.read_tallies()
    hc.write_tallies(pc.crafted_tallies(hc.layout, c), i)
    cpin = cons.ProfileIn(**{k: c[k] for k in cons.PROFILE_SETTINGS}, hist_q_px=(), hist_q_en=(), pxx_EM=c["pxx_EM"], en_EM=c["en_EM"], atan_x=c["atan_x"])
    cpres = (c["P_par"], c["P_perp"], c["e_dens"])
    cfirst, t_cls = timed(hc, args.calls, lambda: hc.profile_update(cpin, cpres))
    print(f"classical crafted case: diag {cfirst[1].tolist()} (largest Newton step count {int(cfirst[1][2])}); two calls, the same bits: "
          f"{same_bits(cfirst, hc.profile_update(cpin, cpres))}")
    hc.destroy()
    print(f"{args.calls} rounds after 2 warm-up rounds; median (min .. max)")
    print(f"  mcs_profile_update (K13), the run's tallies, resident pressures  {ms(t_call)}")
    print(f"  mcs_profile_update (K13), classical crafted case, pointer path    {ms(t_cls)}")
    print(f"  mcs_ens_add_profile + synchronise                                 {ms(t_add)}")
    print(f"  iter_finalize (numpy, smooth_shocks) on the same inputs           {ms(t_host)}")
    per_it = (statistics.median(t_call) + statistics.median(t_add)) * 1e3
    print(f"per iteration: {per_it:.3f} ms (call + sample)")
    if args.bench_json:
        line = [ln for ln in open(args.bench_json).read().splitlines() if ln.startswith("{")][-1]
        b = json.loads(line)
        it = b["ms_per_step"]
        print(f"bench.py: {b['config']['workload']}: {it:.1f} ms per iteration; profile=True adds {per_it:.3f} ms = {100 * per_it / it:.3f} % of it")


if __name__ == "__main__":
    main()
