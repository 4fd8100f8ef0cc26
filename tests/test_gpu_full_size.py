"""BASELINE configs at their full sizes on the GPU, through the C ABI.

config[1] (10^6 protons, one iteration, all 45 pcuts): against the committed reduction of ONE full
run of the CPU oracle (tests/golden/full_1e6.npz, made by tests/golden/make_golden_full.py): integer
tallies and population sizes equal, every binned spectrum within 1e-11 of its maximum (1e-10 for the flux vectors and
scalar accumulators that sum 1e7..1e8 terms per entry, see LONG_SUM_RTOL).

config[2]'s population (10^7 particles) and config[1]'s again: size-independent properties checked in
EVERY pcut the iteration reaches -- the late ones included, where the whole population is 10^5..10^7
replicas of one or two saved particles piling onto single histogram bins.
"""
import os
import time

import numpy as np
import pytest

from conftest import ROOT, mcs, make_problem, oracle_backend, hip_backend, start_species, bits, assert_pop_equal, assert_tallies_close

pytestmark = pytest.mark.gpu
TALLY_RTOL = 1e-11
# Arrays whose entries are sums of 1e7..1e8 terms at this size: the three flux vectors (signed terms per zone: upstream-
# and downstream-going crossings cancel to a tenth of their gross sum) and the per-species / per-time-cut / per-momentum-
# bin accumulators (esc_flux: 1.6e7 IDENTICAL weights, whose rounding errors do not average out but add up along whatever
# order the adds take -- one serial sum in the oracle, per-block partial sums in LDS on the GPU).
# A-priori bound, not a fitted one: a sum of n non-negative fp64 terms differs between two summation orders by at most
# ~n * 2^-53 of the sum (each add rounds by <= half an ulp of the running total); n = 1.6e7 gives 1.8e-9, and for the flux
# vectors the cancellation multiplies it by ten.  The bound used, 1e-10, is TIGHTER than that worst case (rounding errors of
# unequal terms mostly average out: measured 1.5e-11 .. 2.7e-11); 1e-11 holds for every array that sums < 1e6 terms per
# entry.  A compensated reference sum would not tighten it: the GPU's own order-dependent rounding is the same size.
# (The reference rounds its fluxes to 13 digits for the same reason, src/iter_finalize.jl:46-54.)
LONG_SUM_RTOL = 1e-10
LONG_SUMS = ("pxx_flux", "pxz_flux", "energy_flux", "esc_flux", "px_esc_feb", "energy_esc_feb", "esc_energy_eff", "esc_num_eff",
             "weight_coupled", "spectra_coupled_val", "scalars")


def _fixture_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_full", os.path.join(ROOT, "tests", "golden", "make_golden_full.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _load_reducer():
    return _fixture_module().reduce_tallies


def _binned_vs_fixture(got, fix, skip=()):
    """Every binned array of a reduced run against the fixture's: *_idx equal, the rest within TALLY_RTOL of the array's
    maximum (LONG_SUM_RTOL for LONG_SUMS).  Returns (worst array, its error) and the number of arrays compared."""
    worst, n = ("", 0.0), 0
    for k in fix.files:
        if k in ("stats", "tallies_i64", "meta") or k in skip:
            continue
        n += 1
        a, b = got[k], fix[k]
        assert a.shape == b.shape, k
        if k.endswith("_idx"):
            assert np.array_equal(a, b), k
            continue
        scale = float(np.max(np.abs(b))) if b.size else 0.0
        if scale == 0.0:
            assert not np.any(a), k
            continue
        err = float(np.max(np.abs(a - b))) / scale
        if err > worst[1]:
            worst = (k, err)
        tol = LONG_SUM_RTOL if k in LONG_SUMS else TALLY_RTOL
        assert err <= tol, f"{k}: max|gpu - oracle| / max|oracle| = {err:.3e}"
    return worst, n


def test_config1_full_size_vs_oracle_fixture():
    fix = np.load(os.path.join(ROOT, "tests", "golden", "full_1e6.npz"))
    N = 1_000_000
    prob = make_problem(N)
    hb = hip_backend(prob)
    res = mcs.driver.run(prob, hb, None, n_itrs=1)
    hb.destroy()
    got = _load_reducer()(mcs.capi.Layout(prob.params), res.tallies_f64, res.tallies_i64, res.stats)
    assert np.array_equal(got["stats"], fix["stats"])                 # n_pts_use, n_saved, i_mult of all pcuts
    assert np.array_equal(got["tallies_i64"], fix["tallies_i64"])     # crossings per zone, exits by reason, steps, draws
    assert int(fix["stats"][:, 2].min()) == 0 and len(fix["stats"]) >= 30
    worst, n = _binned_vs_fixture(got, fix)
    print(f"config[1] at 1e6: {n} binned arrays within {TALLY_RTOL}; worst {worst[0]} {worst[1]:.2e}; {fix['meta']}")


def test_long_sum_tolerance_is_the_gpu_add_order_noise(monkeypatch):
    """Where LONG_SUM_RTOL comes from, measured instead of asserted: the SAME iteration (same particles, bit for bit) twice on the
    GPU with two different add orders -- the default (16 tally replicas, per-block LDS staging of the fluxes) and one replica with
    a different number of blocks -- and a pairwise (numpy) re-summation of the long per-bin accumulators of the fixture's
    reducer.  The two GPU runs differ from each other in the long sums by as much as either differs from the oracle's serial
    sum: the bound is order noise of the GPU's own adds, not an error of the serial reference, and a compensated reference would
    not tighten it.  (History: round 2 set 1e-11 for everything, the run gpurun_out/r2_t2.log failed on energy_flux at 2.7e-11 and
    esc_flux at 1.5e-11; the a-priori bound n * 2^-53 for n = 1.6e7 adds is 1.8e-9.)"""
    fix = np.load(os.path.join(ROOT, "tests", "golden", "full_1e6.npz"))
    N = 1_000_000
    red = _load_reducer()
    runs = []
    for env in ({}, {"MCS_TALLY_REPLICAS_OFF": "1", "MCS_FUSED_PCUTS": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        prob = make_problem(N)
        hb = hip_backend(prob)
        if env:
            hb.set_launch(300, 256)          # another block -> particle mapping: other partial sums
        res = mcs.driver.run(prob, hb, None, n_itrs=1)
        hb.destroy()
        runs.append(red(mcs.capi.Layout(prob.params), res.tallies_f64, res.tallies_i64, res.stats))
    a, b = runs
    assert np.array_equal(a["tallies_i64"], b["tallies_i64"]) and np.array_equal(a["stats"], b["stats"])      # the same particles
    worst_gg = worst_go = 0.0
    for k in LONG_SUMS:
        if k not in fix.files:
            continue
        scale = float(np.max(np.abs(fix[k])))
        if scale == 0.0:
            continue
        gg = float(np.max(np.abs(a[k] - b[k]))) / scale
        go = max(float(np.max(np.abs(a[k] - fix[k]))), float(np.max(np.abs(b[k] - fix[k])))) / scale
        assert gg <= LONG_SUM_RTOL and go <= LONG_SUM_RTOL, (k, gg, go)
        worst_gg, worst_go = max(worst_gg, gg), max(worst_go, go)
    # the GPU disagrees with ITSELF by the same order as with the oracle (within a factor of a few either way), above 1e-12
    assert worst_gg > 1e-13 and worst_go > 1e-13
    assert worst_gg > worst_go / 20, (worst_gg, worst_go)
    print(f"long sums: GPU vs GPU (another add order) {worst_gg:.2e}, GPU vs oracle fixture {worst_go:.2e}, bound {LONG_SUM_RTOL}")


def _begin(be, prob, i_iter, i_ion, pop=None):
    """Start species i_ion of iteration i_iter as driver.run does: the first species opens the iteration (begin_iteration
    clears the pools), a later one keeps what the earlier species left.  pop: a caller's population instead of the injection."""
    if i_ion == 1:
        start_species(be, prob, i_iter)
    else:
        cfg = prob.cfg
        sp = cfg.species[i_ion - 1]
        inj = mcs.inputs.init_pop_host(prob, i_ion)
        pmax = mcs.inputs.get_pmax_cutoff(prob.Emax_keV, prob.Emax_per_aa_keV, prob.pmax, sp.aa)
        ewf = 1.0 / cfg.species[-1].density if cfg.species[-1].density else float("inf")
        be.begin_species(i_iter, i_ion, sp.aa, abs(sp.zz), pmax, sp.density, ewf)
        be.set_fluxes(inj.pxx_flux, inj.pxz_flux, inj.energy_flux)
        be.init_pop(inj, 0, inj.n_pts_use, inj.n_pts_use)
    if pop is not None:
        be.set_population(pop)


def _property_run(N, n_prefix=4096, prefix_pcuts=5, prob=None, i_iter=1, i_ion=1, pop=None, hb=None, ob=None, twin=None,
                  kernel=None, twin_kernel=None, min_pcuts=30):
    """One species through every pcut it reaches.  Per pcut: (i) every particle ends in exactly one way and the
    saved flags are the reason-0 particles; (ii) the counters' exits equal the particles that ended, the step counters
    the finals; (iii) the first n_prefix particles equal the oracle's bit for bit while the prefix stays aligned (pcuts 1-4
    save everybody); (iv) the split population is i_mult copies of each saved particle, in order, with weight / i_mult;
    (v) `kernel`: the K1 kernel that ran (mcs_last_kernel).  At the end: weight is conserved through all splits, the
    upstream-escape tallies of this species carry exactly the weight of the particles that escaped upstream (LDS-staged and
    wave-reduced tallies at full size), no zone search failed.

    Species i_ion of a multi-species problem: the caller passes the contexts (hb, and ob for the prefix) and runs the species
    in order; the tallies are cumulative over the iteration, so the end checks take this species' deltas.  Before a later
    species starts the oracle context gets the GPU's whole tally buffer: the electrons read energy_recv_pool, which
    begin_species copies from the ions' energy_transfer_pool -- an fp64 atomic sum whose last bits depend on the order of the
    adds --, and with both sides reading the same bits the electron prefix is compared bit for bit, not by luck.
    pop: a caller's population (set_population) instead of the injection.  n_prefix = 0: no oracle.
    twin: a second context (another kernel of the same statements, chosen by an environment knob at its creation) run in
    lockstep: finals, saved arrays, l_save and the int64 tallies equal after every pcut, the binned tallies to TALLY_RTOL at
    the species end; its energy_transfer_pool is pinned to hb's as the oracle's is.
    state_fp32: the kernels hold the weight as a float (`p.w = (float)in.weight[k]`), so the weight they end, save and tally
    is the population's rounded to fp32; the sums take those weights, and what the rounding removes at each pcut's load is
    counted (w_round) -- the saved weights and the split must still account for every bit of the rest.
    Returns the species' record: pcuts reached, exits, population, i_mult per split, exit reasons, int64 tally deltas."""
    prob = make_problem(N) if prob is None else prob      # (a caller's problem: e.g. one whose profile an iteration has updated)
    fp32 = bool(prob.params.state_fp32)
    caller_pop = pop
    own = hb is None
    if own:
        hb = hip_backend(prob)
        ob = oracle_backend(prob, nthreads=8) if n_prefix > 0 else None
    if ob is not None and i_ion > 1:
        ob.write_tallies(*hb.read_tallies())
    if twin is not None and i_ion > 1:
        twin.write_tally("energy_transfer_pool", hb.layout.view(hb.read_tallies()[0], "energy_transfer_pool"))
    _begin(hb, prob, i_iter, i_ion, caller_pop)
    ng, IC = prob.n_grid, mcs.capi.IC
    L = hb.layout
    pop = hb.get_population()
    n_in = pop.n
    w_in = float(pop.weight.sum())
    if ob is not None:
        _begin(ob, prob, i_iter, i_ion)
        ob.set_population(pop.slice(0, n_prefix))
    if twin is not None:
        _begin(twin, prob, i_iter, i_ion, caller_pop)
    w_out = w_esc_up = w_round = 0.0
    n_done = n_up = 0
    reached = 0
    n_checked = []          # particles compared with the oracle in each of the first pcuts
    mults = []
    reasons = np.zeros(5, dtype=np.int64)
    T0, I0 = hb.read_tallies()
    I_prev = I0
    for ip in range(1, len(prob.pcuts) + 1):
        n_use = pop.n
        ns = hb.run_pcut(ip, 0)
        reached = ip
        if kernel is not None:
            assert hb.last_kernel() == kernel, f"ion {i_ion} pcut {ip}: K1 kernel {hb.last_kernel()}, expected {kernel}"
        f = hb.finals()
        saved, l_save = hb.get_saved()
        assert int(l_save.sum()) == ns and np.array_equal(f["reason"] == 0, l_save == 1), f"pcut {ip}"
        assert f["reason"].min() >= 0 and f["reason"].max() <= 4
        reasons += np.bincount(f["reason"], minlength=5)
        wk = pop.weight.astype(np.float32).astype(np.float64) if fp32 else pop.weight      # the weights the kernel held
        w_round += float(pop.weight.sum()) - float(wk.sum())
        assert np.array_equal(bits(saved.weight[l_save == 1]), bits(wk[l_save == 1])), f"pcut {ip}: saved weights"
        ended = f["reason"] != 0
        w_out += float(wk[ended].sum())
        up = f["reason"] == 2
        w_esc_up += float(wk[up].sum()); n_up += int(up.sum())
        n_done += int(ended.sum())
        I = hb.read_counters()
        d = I - I_prev; I_prev = I
        assert sum(int(d[ng + IC[f"REASON{r}"]]) for r in range(1, 5)) == int(ended.sum()), f"pcut {ip}"
        assert int(d[ng + IC["REASON0"]]) == ns and int(ended.sum()) + ns == n_use
        assert int(d[ng + IC["STEPS_HELIX"]]) == int(np.minimum(f["helix"], 10000).astype(np.int64).sum())
        assert int(d[ng + IC["STEPS_RETRO"]]) == int(f["retro"].astype(np.int64).sum())
        if twin is not None:
            assert twin.run_pcut(ip, 0) == ns, f"ion {i_ion} pcut {ip}: n_saved of the twin"
            if twin_kernel is not None:
                assert twin.last_kernel() == twin_kernel, f"ion {i_ion} pcut {ip}: twin's K1 kernel {twin.last_kernel()}, expected {twin_kernel}"
            ft = twin.finals()
            for k in f:
                assert np.array_equal(bits(f[k]), bits(ft[k])), f"ion {i_ion} pcut {ip}: final {k} differs for {(f[k] != ft[k]).sum()} particles"
            st, lt = twin.get_saved()
            assert np.array_equal(l_save, lt), f"ion {i_ion} pcut {ip}: l_save"
            assert_pop_equal(saved, st, f"ion {i_ion} pcut {ip}: saved arrays")
            assert np.array_equal(twin.read_counters(), I), f"ion {i_ion} pcut {ip}: int64 tallies"
        nso = 0
        if ip <= prefix_pcuts and n_prefix > 0:
            nso = ob.run_pcut(ip, 0)
            fo = ob.finals()
            for k in fo:
                assert np.array_equal(bits(f[k][:n_prefix]), bits(fo[k])), f"ion {i_ion} pcut {ip}: prefix {k}"
            n_checked.append(n_prefix)
        if ns == 0:
            break
        im = max(N // ns, 1)
        mults.append(im)
        if ip < prefix_pcuts and n_prefix > 0:
            # the children of the prefix's saved particles are the first nso * im particles of the next population, with the
            # same global indices (the split keeps the order): the oracle follows with ITS split of the prefix
            n_prefix = ob.new_pcut(im) if nso > 0 else 0
            assert n_prefix == nso * im
        assert hb.new_pcut(im) == ns * im
        if twin is not None:
            assert twin.new_pcut(im) == ns * im
        pop = hb.get_population()
        src = np.flatnonzero(l_save)
        o = np.unique(np.concatenate([np.arange(0, pop.n, 7), np.arange(max(pop.n - 1000, 0), pop.n)]))   # a sample of the new indices
        par = src[o // im]
        for fld in pop.fields():
            want = getattr(saved, fld)[par]
            if fld == "weight":
                want = want / float(im)
            assert np.array_equal(bits(getattr(pop, fld)[o]), bits(want)), f"pcut {ip}: split field {fld} (i_mult {im}, {ns} parents)"
    assert reached >= min_pcuts, f"ion {i_ion}: {reached} pcuts reached, expected at least {min_pcuts}"
    if n_checked:
        assert len(n_checked) >= min(3, reached) and min(n_checked[:3]) >= 256, n_checked
    w_left = float(pop.weight.sum()) if ns else 0.0
    assert abs(w_out + w_left + w_round - w_in) < 1e-9 * w_in
    T, I = hb.read_tallies()
    dI = I - I0
    assert int(I[ng + IC["ZONE_FAIL"]]) == 0 and int(I[ng + IC["RETRO_CAP"]]) == 0
    assert sum(int(dI[ng + IC[f"REASON{r}"]]) for r in range(1, 5)) == n_done
    assert int(dI[ng + IC["REASON2"]]) == n_up
    # reason-2 weight reaches esc_flux (LDS scalar staging) and esc_num_eff (LDS per-bin staging) exactly once, in this species' row
    ion = i_ion - 1
    d_flux = L.view(T, "esc_flux") - L.view(T0, "esc_flux")
    d_num = L.view(T, "esc_num_eff") - L.view(T0, "esc_num_eff")
    assert abs(float(d_flux[ion]) - w_esc_up) <= 1e-10 * max(w_esc_up, 1e-300)
    assert abs(float(d_num[ion].sum()) - w_esc_up) <= 1e-10 * max(w_esc_up, 1e-300)
    assert not np.any(np.delete(d_flux, ion)) and not np.any(np.delete(d_num, ion, axis=0)), f"ion {i_ion}: escape tallied in another species' row"
    if twin is not None:
        Tt, It = twin.read_tallies()
        assert np.array_equal(It, I), f"ion {i_ion}: int64 tallies of the twin"
        assert_tallies_close(L, Tt, T, TALLY_RTOL)
    if own:
        hb.destroy()
        if ob is not None:
            ob.destroy()
    return dict(reached=reached, n_done=n_done, n_in=n_in, i_mult=mults, reasons=reasons, dI=dI)


def test_config1_properties_every_pcut_1e6():
    r = _property_run(1_000_000)
    print(f"1e6 protons: {r['reached']} pcuts reached, {r['n_done']} exits")


def test_config2_population_properties_every_pcut_1e7():
    r = _property_run(10_000_000)
    print(f"1e7 protons: {r['reached']} pcuts reached, {r['n_done']} exits")


def test_config3_per_gpu_size_properties_5e7():
    """BASELINE config[3] (1e8 particles over 2 / 4 / 8 GPUs) at its LARGEST per-GPU size, 5e7 particles on one GPU: the same
    per-pcut properties (every particle ends once, counters equal exits, splits are i_mult copies in order, weight conserved,
    the first 4096 particles equal the oracle's bit for bit) with 10 GB of population buffers resident.  The multi-GPU run
    itself cannot be tested on a one-GPU box; what a rank of it computes is this."""
    r = _property_run(50_000_000)
    print(f"5e7 protons: {r['reached']} pcuts reached, {r['n_done']} exits")


def test_config2_1e7_second_iteration_on_the_updated_profile():
    """BASELINE config[2] at its own size WITH its own loop: iteration 1 of 10^7 protons through driver.run with smoothing on
    (K4 consumers on the device, iter_finalize, smooth_grid_par, new tables through mcs_set_grid), then iteration 2 -- on the
    modified profile every zone crossing takes the frame transform -- through the per-pcut property checks of _property_run,
    the first 4096 particles against the oracle on the same updated tables."""
    N = 10_000_000
    itf = mcs.iter_finalize
    cfg = mcs.inputs.Config(N_PTS_INJ=N, N_PTS_PCUT=N, N_PTS_PCUT_HI=N, num_iterations=2)
    prob = mcs.inputs.build_problem(cfg)
    u_before = prob.ux.copy()
    hb = hip_backend(prob)
    res = mcs.driver.run(prob, hb, None, n_itrs=1, smoothing=itf.SmoothingConfig(smooth_shocks=True), species_tallies="light")
    hb.destroy()
    (_, fin, ion), = res.iter_finals
    P, n = prob.params, prob.n_grid
    assert fin.profile_changed and not np.array_equal(prob.ux, u_before)
    u = prob.ux[1:n + 1]
    assert np.all(np.diff(u) <= 1e-12 * P.u0) and u.max() <= P.u0 * (1 + 1e-12) and u.min() >= P.u2 * (1 - 1e-12)
    assert prob.ux[P.i_shock - 3] < 0.999 * P.u0                      # a precursor has formed
    assert 4.0 / 3.0 - 0.02 < fin.Gamma_downstream < 5.0 / 3.0 + 0.02
    assert np.all(np.isfinite(ion.P_psd_par)) and ion.P_psd_par.max() > 0
    ng, IC = n, mcs.capi.IC
    I = res.tallies_i64
    assert int(I[ng + IC["ZONE_FAIL"]]) == 0 and int(I[ng + IC["RETRO_CAP"]]) == 0
    st = [(s.n_pts_use, s.n_saved, s.i_mult) for s in res.stats]
    assert all(b[0] == a[1] * a[2] for a, b in zip(st, st[1:])) and len(st) >= 30      # every population is the split of the previous one
    assert sum(int(I[ng + IC[f"REASON{r}"]]) for r in range(1, 5)) == sum(a[0] - a[1] for a in st)
    r = _property_run(N, prob=prob, i_iter=2)
    print(f"config[2], 1e7 protons: iteration 1 {res.steps_helix + res.steps_retro} steps, profile updated "
          f"(u_x at shock-3: {prob.ux[P.i_shock - 3] / P.u0:.4f} u0); iteration 2 on it: {r['reached']} pcuts, {r['n_done']} exits")


# ---- BASELINE config[4], the species mix of `bench.py --mixed` (protons + He + electrons, radiative losses, ion -> electron energy
# transfer), at the bench's size: 10^6 particles per species.  K1 kernel per species (mcs_last_kernel, the K1Kernel enum): the ions
# run PLAIN with the energy-transfer flag (6; its wave-specialised form 8), the electrons the lossy kernel (2); with state_fp32 the
# organised fp32 kernels (3 for ions, 5 for electrons) and, under MCS_F32_LOOP=1, the plain per-lane loop (4) for every species.
MIX_KERNELS = {False: (6, 6, 2), True: (3, 3, 5)}


def _mixed_problem(N, **kw):
    return _fixture_module().mixed_problem(N, **kw)


def _check_transfer_pool(prob, hb, i_ion):
    """After an ion species: the energy it handed the electrons is finite, >= 0, only in zones with eps_target > 0 and somewhere."""
    pool = hb.layout.view(hb.read_tallies()[0], "energy_transfer_pool")
    eps = np.asarray(prob.eps_target)
    assert np.all(np.isfinite(pool)) and pool.min() >= 0.0, f"ion {i_ion}: energy_transfer_pool {pool}"
    assert not np.any(pool[eps <= 0]), f"ion {i_ion}: energy transferred in zones {np.flatnonzero((pool != 0) & (eps <= 0)) + 1} without eps_target"
    assert np.any(pool[eps > 0] > 0), f"ion {i_ion}: no energy transferred"
    return pool


def _thermal_electrons_q5(prob, r):
    """Quirk Q5 at size: every thermal electron of the mix ends at the helix cap in its first pcut, nobody is saved."""
    IC, ng = mcs.capi.IC, prob.n_grid
    assert r["reached"] == 1 and r["i_mult"] == [] and r["n_done"] == r["n_in"], r
    assert int(r["dI"][ng + IC["HELIX_CAP"]]) == r["n_in"]
    assert int(r["dI"][ng + IC["REASON1"]]) == r["n_in"]


def test_config4_species_properties_every_pcut_1e6(monkeypatch):
    """The bench mix, fp64, 10^6 particles per species, each species through the per-pcut properties of _property_run in order:
    protons and He on kernel 6 into the late pcuts (10^5..10^6 replicas of a few parents, the energy-transfer flag under the tail
    loop, LDS-staged escape tallies of a Z = 2, A = 4 ion), the first 4096 particles against the oracle; the energy_transfer_pool
    after each ion species; the thermal electrons on kernel 2 against the oracle with the ions' pool pinned (see _property_run),
    and their Q5 outcome -- one pcut, nobody saved, every electron at the helix cap -- which is the bench's electron workload."""
    t0 = time.perf_counter()
    monkeypatch.delenv("MCS_K1_WS", raising=False)
    N = 1_000_000
    prob = _mixed_problem(N)
    hb, ob = hip_backend(prob), oracle_backend(prob, nthreads=8)
    rs = []
    for i_ion, kernel in enumerate(MIX_KERNELS[False], 1):
        ion = i_ion < 3
        rs.append(_property_run(N, prob=prob, i_ion=i_ion, hb=hb, ob=ob, kernel=kernel, min_pcuts=30 if ion else 1))
        if ion:
            _check_transfer_pool(prob, hb, i_ion)
    _thermal_electrons_q5(prob, rs[2])
    hb.destroy(); ob.destroy()
    print(f"config[4] fp64 at 1e6 per species: pcuts reached {[r['reached'] for r in rs]}, exits {[r['n_done'] for r in rs]}, "
          f"max i_mult {[max(r['i_mult'], default=0) for r in rs]}; {time.perf_counter() - t0:.0f} s")


def test_config4_fp32_organised_kernels_equal_plain_loop_1e6(monkeypatch):
    """test_fp32_kernels_agree at the bench size: the fp32-state mix at 10^6 per species through the organised kernels (3, 3, 5)
    and, in lockstep on a second context, through the plain per-lane loop (MCS_F32_LOOP=1: 4).  The hardware fp32 primitives have
    no CPU equal, so the check at size is bit identity between the two forms -- particles, saved arrays, l_save and int64 tallies
    in every pcut, binned tallies to TALLY_RTOL -- plus the per-pcut properties of _property_run (no oracle prefix)."""
    t0 = time.perf_counter()
    N = 1_000_000
    prob = _mixed_problem(N, state_fp32=True)
    monkeypatch.setenv("MCS_F32_LOOP", "0")
    hb = hip_backend(prob)
    monkeypatch.setenv("MCS_F32_LOOP", "1")
    tw = hip_backend(prob)
    rs = []
    for i_ion, kernel in enumerate(MIX_KERNELS[True], 1):
        ion = i_ion < 3
        rs.append(_property_run(N, n_prefix=0, prob=prob, i_ion=i_ion, hb=hb, twin=tw, kernel=kernel, twin_kernel=4,
                                min_pcuts=30 if ion else 1))
        if ion:
            _check_transfer_pool(prob, hb, i_ion)
    _thermal_electrons_q5(prob, rs[2])
    hb.destroy(); tw.destroy()
    print(f"config[4] fp32 at 1e6 per species, organised == plain loop: pcuts reached {[r['reached'] for r in rs]}; "
          f"{time.perf_counter() - t0:.0f} s")


def test_config4_wave_specialised_ion_kernel_1e6(monkeypatch):
    """The ions of the bench mix at 10^6 through the wave-specialised form of their kernel (MCS_K1_WS=1: 8) in lockstep with the
    default choice (6 at this size): every particle, saved array and int64 tally bit for bit in every pcut, binned tallies to
    TALLY_RTOL.  test_wave_specialised_kernel_is_bit_identical covers 8 at 4000 particles only."""
    t0 = time.perf_counter()
    N = 1_000_000
    prob = _mixed_problem(N)
    monkeypatch.delenv("MCS_K1_WS", raising=False)
    hb = hip_backend(prob)
    monkeypatch.setenv("MCS_K1_WS", "1")
    tw = hip_backend(prob)
    rs = [_property_run(N, n_prefix=0, prob=prob, i_ion=i_ion, hb=hb, twin=tw, kernel=6, twin_kernel=8) for i_ion in (1, 2)]
    hb.destroy(); tw.destroy()
    print(f"config[4] ions at 1e6, kernel 8 == kernel 6: pcuts reached {[r['reached'] for r in rs]}; {time.perf_counter() - t0:.0f} s")


# The crafted relativistic electrons of the golden case electrons_crafted_n64 (make_golden.crafted_population) at 10^6, with the
# stock momentum cuts but two changes, chosen on the oracle at N = 2000 and 20000: with the stock cuts every electron ends in pcut
# 17 (1e5 m_p c: the losses in the 3 G field stop them below it), the largest split is i_mult 8 and no exit has reason 3.  Cut 17
# lowered to 5.623e4 m_p c (between its neighbours 3.162e4 and 3.162e5): 1.5 % of pcut 17 is saved, i_mult ~66 there, 18 pcuts
# reached.  maximum_age 3e5 s, inside the crafted ages (10^0..10^6 s): the oldest ~9 % leave by age (reason 3) in pcut 1.
CRAFTED_CUT17 = 5.623e4
CRAFTED_AGE_MAX = 3e5


def _crafted_electron_problem(N, **kw):
    from golden_common import make_golden
    c = dict(make_golden.CASES["electrons_crafted_n64"]["cfg"])
    c["species"] = [mcs.inputs.Species(**sp) for sp in c["species"]]
    cuts = list(mcs.inputs.STOCK_PCUTS)
    assert cuts[16] == 1e5
    cuts[16] = CRAFTED_CUT17
    c.update(momentum_cutoffs=tuple(cuts), maximum_age=CRAFTED_AGE_MAX, **kw)
    return mcs.inputs.build_problem(mcs.inputs.Config(N_PTS_INJ=N, N_PTS_PCUT=N, N_PTS_PCUT_HI=N, **c)), make_golden


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_crafted_electrons_lossy_kernel_every_pcut_1e6(monkeypatch, precision):
    """Electrons that live: the lossy kernels' multi-pcut path at size -- splits of electrons up to i_mult ~66, PRP shortening,
    losses inside the retro walk -- where the thermal electrons of the mix die in pcut 1 (Q5).  fp64: kernel 2 through the
    per-pcut properties, the first 4096 particles against the oracle.  fp32: the organised lossy kernel (5) in lockstep with the
    plain loop (4), bit for bit.  Both: at least 5 pcuts, a split by >= 10, exit reasons 0-3 all present, > 100 helix steps per
    particle (the losses act in the helix loop)."""
    t0 = time.perf_counter()
    N = 1_000_000
    fp32 = precision == "fp32"
    prob, make_golden = _crafted_electron_problem(N, state_fp32=fp32)
    pop = make_golden.crafted_population("electrons", prob, N)
    if fp32:
        monkeypatch.setenv("MCS_F32_LOOP", "0")
        hb = hip_backend(prob)
        monkeypatch.setenv("MCS_F32_LOOP", "1")
        tw = hip_backend(prob)
        r = _property_run(N, n_prefix=0, prob=prob, pop=pop, hb=hb, twin=tw, kernel=5, twin_kernel=4, min_pcuts=5)
        tw.destroy()
    else:
        hb, ob = hip_backend(prob), oracle_backend(prob, nthreads=8)
        r = _property_run(N, prob=prob, pop=pop, hb=hb, ob=ob, kernel=2, min_pcuts=5)
        ob.destroy()
    hb.destroy()
    IC = mcs.capi.IC
    ng = prob.n_grid
    assert max(r["i_mult"]) >= 10, r["i_mult"]
    assert np.all(r["reasons"][:4] > 0), r["reasons"]
    assert int(r["dI"][ng + IC["STEPS_HELIX"]]) > 100 * N
    print(f"crafted electrons {precision} at 1e6: {r['reached']} pcuts, i_mult {r['i_mult']}, reasons {r['reasons'].tolist()}, "
          f"{int(r['dI'][ng + IC['STEPS_HELIX']]) / N:.0f} helix steps per particle; {time.perf_counter() - t0:.0f} s")


def test_config4_mixed_iteration_vs_oracle_fixture():
    """The bench mix at 10^5 per species, one whole iteration through driver.run, against the committed run of the oracle
    (tests/golden/mixed_1e5.npz, make_golden_full.py --mixed): per-pcut populations of every species, int64 tallies at every
    species end and at the end equal, every binned array of the reduction within TALLY_RTOL (LONG_SUM_RTOL for LONG_SUMS).  The
    electrons read the ions' energy_transfer_pool, an fp64 atomic sum whose last bits depend on the add order: at each species end
    the GPU's pool is compared with the oracle's to LONG_SUM_RTOL and then replaced by the oracle's bits, so that the electrons
    start from the same pool as the oracle's did -- pinning, not a looser tolerance."""
    t0 = time.perf_counter()
    fix = np.load(os.path.join(ROOT, "tests", "golden", "mixed_1e5.npz"))
    m = _fixture_module()
    prob = m.mixed_problem(100_000)
    hb = hip_backend(prob)
    L = hb.layout
    pools, ints = fix["species_energy_transfer_pool"], fix["species_tallies_i64"]
    kernels, pool_err = [], []

    def species_end(i_iter, i_ion, f, i):
        kernels.append(hb.last_kernel())
        assert np.array_equal(i, ints[i_ion - 1]), f"ion {i_ion}: int64 tallies at the species end"
        got, want = L.view(f, "energy_transfer_pool"), pools[i_ion - 1]
        err = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
        assert err <= LONG_SUM_RTOL, f"ion {i_ion}: energy_transfer_pool off by {err:.3e}"
        pool_err.append(err)
        if i_ion < len(prob.cfg.species):
            got[...] = want
            hb.write_tallies(f, i)
    res = mcs.driver.run(prob, hb, None, n_itrs=1, on_species_end=species_end)
    hb.destroy()
    assert kernels == list(MIX_KERNELS[False]), kernels
    got = m.reduce_tallies(L, res.tallies_f64, res.tallies_i64, res.stats, with_ion=True)
    assert np.array_equal(got["stats"], fix["stats"])                 # i_ion, i_pcut, n_pts_use, n_saved, i_mult of all pcuts
    assert np.array_equal(got["tallies_i64"], fix["tallies_i64"])
    assert sorted({int(s) for s in fix["stats"][:, 0]}) == [1, 2, 3]
    worst, n = _binned_vs_fixture(got, fix, skip=("species_energy_transfer_pool", "species_tallies_i64"))
    print(f"config[4] at 1e5 per species: kernels {kernels}, pools within {max(pool_err):.2e}; {n} binned arrays, worst "
          f"{worst[0]} {worst[1]:.2e} (bound {LONG_SUM_RTOL if worst[0] in LONG_SUMS else TALLY_RTOL}); {fix['meta']}; "
          f"{time.perf_counter() - t0:.0f} s")
