"""The independent species of an iteration on secondary contexts (driver.run(..., species_backends=[...])) against the one-context
run, on the CPU oracle; the tally-section lists of capi; mcs_accumulate_tallies' refusals without a GPU.

The species of a secondary start their running sums from zero and are merged into the primary afterwards, so the sums that
several species add to (energy_transfer_pool, spectra_sf / _pf, scalars) are the sequential run's up to the association of the
adds.  Each species' own slices, the int64 tallies and the populations are the sequential run's bits.  The electrons read the
ions' energy_transfer_pool; at every species end the hook pins it to the sequential run's bits, as the GPU fixture test pins it
to the oracle's, so that the electrons start from the same pool."""
import ctypes as ct
import threading

import numpy as np
import pytest

from conftest import mcs, oracle_backend, start_species, bits, assert_pop_equal

ME_MP = mcs.constants.ME / mcs.constants.MP
S = mcs.inputs.Species
N = 200
N_PCUTS = 8
SHARED = ("energy_transfer_pool", "spectra_sf", "spectra_pf", "scalars")
PER_ION = ("esc_flux", "px_esc_feb", "energy_esc_feb", "esc_energy_eff", "esc_num_eff", "weight_coupled", "spectra_coupled")


def mixed(species=None, etf=0.1, **kw):
    """The mixed_n96 golden's optional branches (energy transfer, losses, x_spec detectors, injection fraction < 1) with p, He, e-."""
    species = species or [S(1.0, 1.0, 1e6, 1.0), S(4.0, 2.0, 1e6, 0.1), S(ME_MP, -1.0, 1e6, 1.2)]
    injfr = [0.7] + [1.0] * (len(species) - 1)
    cfg = mcs.inputs.Config(N_PTS_INJ=N, N_PTS_PCUT=N, N_PTS_PCUT_HI=N, species=species, energy_transfer_frac=etf, radiation_losses=True,
                            INJFR=injfr, b_field_turbulence=1.0, shock_speed=3.0, num_iterations=2, **kw)
    rg0 = mcs.inputs.build_problem(cfg).rg0
    cfg.XSPEC = tuple(x * rg0 for x in (-0.5, 0.05, 2.0))
    return mcs.inputs.build_problem(cfg)


def stat_keys(res):
    return [(s.i_iter, s.i_ion, s.i_pcut, s.n_pts_use, s.n_saved, s.i_mult, s.n_use_max) for s in res.stats]


def sequential(make, pin="pool", **kw):
    """The one-context run; records what every species end handed out."""
    prob = make()
    be = oracle_backend(prob)
    ends = {}

    def hook(i_iter, i_ion, f, i):
        ends[(i_iter, i_ion)] = (f.copy(), i.copy())
    res = mcs.driver.run(prob, be, None, max_pcuts=N_PCUTS, on_species_end=hook, **kw)
    return res, ends


def concurrent(make, ends, n_sec=1, pin="pool", prob=None, backends=None, **kw):
    """The same with n_sec secondaries: int64 tallies equal at every species end, then the pinned sections written back."""
    prob = prob or make()
    ctxs = backends or [oracle_backend(prob) for _ in range(1 + n_sec)]
    L = ctxs[0].layout
    seen = []

    def hook(i_iter, i_ion, f, i):
        seen.append((i_iter, i_ion))
        wf, wi = ends[(i_iter, i_ion)]
        assert np.array_equal(i, wi), f"iteration {i_iter}, species {i_ion}: int64 tallies at the species end"
        names = ("energy_transfer_pool",) if pin == "pool" else mcs.capi.RUNNING_F64
        for name in names:
            L.view(f, name)[...] = L.view(wf, name)
        ctxs[0].write_tallies(f, i)
    res = mcs.driver.run(prob, ctxs[0], None, max_pcuts=N_PCUTS, on_species_end=hook, species_backends=ctxs[1:], **kw)
    its = sorted({it for it, _, _, _, _ in res.species_spans})
    assert seen == [k for k in sorted(ends) if k[0] in its], seen      # every species end, in species order
    return res, ctxs


def assert_same_run(L, r1, r2, first_iter=1, rtol=1e-12):
    assert stat_keys(r1) == stat_keys(r2)
    assert r1.local_steps == r2.local_steps
    assert np.array_equal(r1.tallies_i64, r2.tallies_i64)
    assert [(a, b) for a, b, _, _ in r1.per_species] == [(a, b) for a, b, _, _ in r2.per_species]
    on_secondary = {(it, ion) for it, ion, k, _, _ in r2.species_spans if k > 0}
    for (it, ion, f1, i1), (_, _, f2, i2) in zip(r1.per_species, r2.per_species):
        assert np.array_equal(i1, i2)
        for name in mcs.capi.PER_SPECIES_F64:
            if name == "energy_recv_pool" and (it, ion) in on_secondary:
                # (a secondary's pool holds nothing to hand on: the ion reads none of it -- the premise test below)
                assert not np.any(L.view(f2, name)), (it, ion)
                continue
            assert np.array_equal(bits(L.view(f1, name)), bits(L.view(f2, name))), (it, ion, name)
        for name in PER_ION + SHARED:
            a, b = L.view(f1, name), L.view(f2, name)
            if name in PER_ION and it == first_iter:
                # (a species' own slices: one species adds to them in the iteration.  Later iterations add onto the earlier ones'
                # sums, which the secondary's species do only at their merge: the same sums, associated differently)
                assert np.array_equal(bits(a), bits(b)), (it, ion, name)
            scale = float(np.max(np.abs(a))) or 1.0
            assert float(np.max(np.abs(a - b))) <= rtol * scale, (it, ion, name)


def assert_finals_close(r1, r2, rtol=1e-12):
    import dataclasses
    assert len(r1.iter_finals) == len(r2.iter_finals)
    for (it1, f1, g1), (it2, f2, g2) in zip(r1.iter_finals, r2.iter_finals):
        assert it1 == it2
        for a_obj, b_obj in ((f1, f2), (g1, g2)):
            for fld in dataclasses.fields(a_obj):
                a, b = getattr(a_obj, fld.name), getattr(b_obj, fld.name)
                if isinstance(a, (bool, str)) or a is None:
                    assert a == b, fld.name
                    continue
                a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
                scale = float(np.max(np.abs(a))) if a.size and np.all(np.isfinite(a)) else 1.0
                assert np.allclose(a, b, rtol=0, atol=rtol * (scale or 1.0), equal_nan=True), (it1, fld.name)


def test_mix_with_one_secondary_matches_sequential():
    r1, ends = sequential(mixed, n_itrs=2, finalize=True)
    r2, ctxs = concurrent(mixed, ends, n_itrs=2, finalize=True)
    L = ctxs[0].layout
    assert_same_run(L, r1, r2)
    assert_finals_close(r1, r2)
    assert sorted(r1.stats[0].__dict__) == sorted(r2.stats[0].__dict__)
    for it in (1, 2):
        sp = {ion: (k, t0, t1) for i, ion, k, t0, t1 in r2.species_spans if i == it}
        assert [sp[ion][0] for ion in (1, 2, 3)] == [0, 1, 0]
        assert sp[3][1] >= max(sp[1][2], sp[2][2]), "the electrons started before both ions had ended"
    assert r1.species_spans == []


@pytest.mark.parametrize("n_sec", [2, 1])
def test_three_ions_and_electrons(n_sec):
    sp4 = [S(1.0, 1.0, 1e6, 1.0), S(4.0, 2.0, 1e6, 0.1), S(16.0, 8.0, 1e6, 0.01), S(ME_MP, -1.0, 1e6, 1.2)]
    make = lambda: mixed(sp4)
    r1, ends = sequential(make, n_itrs=1)
    r2, ctxs = concurrent(make, ends, n_sec=n_sec, n_itrs=1)
    assert_same_run(ctxs[0].layout, r1, r2)
    sp = {ion: (k, t0, t1) for _, ion, k, t0, t1 in r2.species_spans}
    assert [sp[ion][0] for ion in (1, 2, 3, 4)] == ([0, 1, 2, 0] if n_sec == 2 else [0, 1, 1, 0])
    if n_sec == 1:
        assert sp[3][1] >= sp[2][2], "O started on the secondary before He was merged"
    assert sp[4][1] >= max(sp[j][2] for j in (1, 2, 3)), "the electrons started before every ion had ended"


def test_mix_without_energy_transfer():
    make = lambda: mixed(etf=0.0)
    r1, ends = sequential(make, n_itrs=1)
    r2, ctxs = concurrent(make, ends, n_itrs=1)
    assert_same_run(ctxs[0].layout, r1, r2)
    assert [k for _, _, k, _, _ in r2.species_spans] == [0, 1, 0]


def test_smoothing_updates_every_context():
    """smooth_shocks over two iterations: the second iteration runs every species on the updated profile -- also He on the
    secondary.  Every running sum is pinned to the sequential run's bits, so the profile update is the same bit for bit."""
    sm = mcs.iter_finalize.SmoothingConfig(smooth_shocks=True)
    r1, ends = sequential(mixed, n_itrs=2, smoothing=sm)
    r2, ctxs = concurrent(mixed, ends, pin="running", n_itrs=2, smoothing=sm)
    assert_same_run(ctxs[0].layout, r1, r2, rtol=0.0)
    assert_finals_close(r1, r2, rtol=0.0)
    assert any(f.profile_changed for _, f, _ in r1.iter_finals[:1])


def test_secondary_reused_across_calls():
    """Iteration 1 and iteration 2 in two run() calls (first_iter / iter_state) with the same secondary, whose running sums hold
    stale values before the second call: they are zeroed at its start."""
    r1, ends = sequential(mixed, n_itrs=2, finalize=True)
    prob = mixed()
    ctxs = [oracle_backend(prob), oracle_backend(prob)]
    a, _ = concurrent(mixed, ends, prob=prob, backends=ctxs, n_itrs=1, finalize=True)
    L = ctxs[0].layout
    f, i = ctxs[1].read_tallies()
    for name in mcs.capi.RUNNING_F64:
        L.view(f, name)[...] = 7.0
    i[mcs.capi.running_i64(L)] = 7
    ctxs[1].write_tallies(f, i)
    b, _ = concurrent(mixed, ends, prob=prob, backends=ctxs, n_itrs=1, finalize=True, first_iter=2, iter_state=a.iter_state)
    assert np.array_equal(b.tallies_i64, r1.tallies_i64)
    assert stat_keys(r1) == stat_keys(a) + stat_keys(b)
    r2 = mcs.driver.RunResult(b.tallies_f64, b.tallies_i64, a.per_species + b.per_species, a.stats + b.stats, b.steps_helix,
                              b.steps_retro, a.iter_finals + b.iter_finals, b.iter_state, a.local_steps + b.local_steps,
                              species_spans=a.species_spans + b.species_spans)
    assert_same_run(L, r1, r2)
    assert_finals_close(r1, r2)


def test_section_lists_partition_the_layout():
    prob = mixed()
    L = mcs.capi.Layout(prob.params)
    names = mcs.capi.PER_SPECIES_F64 + mcs.capi.RUNNING_F64
    assert sorted(names) == sorted(L.offsets) and len(set(names)) == len(names)
    cover = np.zeros(L.total, dtype=np.int64)
    for name in names:
        o = L.offsets[name]
        cover[o:o + int(np.prod(L.shapes[name]))] += 1
    assert np.all(cover == 1)
    # the table beside mcs_tally_layout: running sums [esc_flux, energy_recv_pool) and scalars
    run = np.zeros(L.total, dtype=bool)
    for name in mcs.capi.RUNNING_F64:
        o = L.offsets[name]
        run[o:o + int(np.prod(L.shapes[name]))] = True
    want = np.zeros(L.total, dtype=bool)
    want[L.offsets["esc_flux"]:L.offsets["energy_recv_pool"]] = True
    want[L.offsets["scalars"]:] = True
    assert np.array_equal(run, want)
    ps, rs = mcs.capi.per_species_i64(L), mcs.capi.running_i64(L)
    assert (ps.start, ps.stop, rs.start, rs.stop) == (0, L.n_grid, L.n_grid, L.n_i64)


def test_host_fallback_moves_the_running_sums():
    prob = mixed()
    a, b = oracle_backend(prob), oracle_backend(prob)
    L = a.layout
    rng = np.random.default_rng(5)
    fa, fb = rng.standard_normal(L.total), rng.standard_normal(L.total)
    ia, ib = rng.integers(-2 ** 40, 2 ** 40, L.n_i64), rng.integers(-2 ** 40, 2 ** 40, L.n_i64)
    a.write_tallies(fa, ia); b.write_tallies(fb, ib)
    mcs.driver.accumulate_tallies_host(L, a, b)
    ga, ja = a.read_tallies(); gb, jb = b.read_tallies()
    r = mcs.capi.running_i64(L)
    for name in mcs.capi.RUNNING_F64:
        assert np.array_equal(bits(L.view(ga, name)), bits(L.view(fa, name) + L.view(fb, name)))
        assert not np.any(L.view(gb, name))
    for name in mcs.capi.PER_SPECIES_F64:
        assert np.array_equal(bits(L.view(ga, name)), bits(L.view(fa, name)))
        assert np.array_equal(bits(L.view(gb, name)), bits(L.view(fb, name)))
    assert np.array_equal(ja[r], ia[r] + ib[r]) and not np.any(jb[r])
    assert np.array_equal(ja[:L.n_grid], ia[:L.n_grid]) and np.array_equal(jb[:L.n_grid], ib[:L.n_grid])


class _Raising:
    """An oracle context that raises in the third pcut of one species."""

    def __init__(self, inner, ion):
        self._inner, self._ion, self._cur = inner, ion, None

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def begin_species(self, i_iter, i_ion, *a):
        self._cur = i_ion
        return self._inner.begin_species(i_iter, i_ion, *a)

    def run_pcut(self, i_pcut, *a, **k):
        if self._cur == self._ion and i_pcut == 3:
            raise RuntimeError("species 2 failed")
        return self._inner.run_pcut(i_pcut, *a, **k)


def test_a_raising_species_is_reraised_and_no_thread_is_left():
    prob = mixed()
    before = set(threading.enumerate())
    prim = oracle_backend(prob)
    ended = []
    with pytest.raises(RuntimeError, match="species 2 failed"):
        mcs.driver.run(prob, prim, None, n_itrs=1, max_pcuts=N_PCUTS, species_backends=[_Raising(oracle_backend(prob), 2)],
                       on_species_end=lambda *a: ended.append(a[:2]))
    assert set(threading.enumerate()) == before
    assert ended == [(1, 1)] or ended == []            # nothing merged after the failure: the electrons never ran
    for kw in (dict(before_pcut=lambda *a: None), dict(long_draws=4)):
        with pytest.raises(ValueError):
            mcs.driver.run(prob, prim, None, n_itrs=1, max_pcuts=2, species_backends=[oracle_backend(prob)], **kw)
    other = mcs.inputs.build_problem(mcs.inputs.Config(N_PTS_INJ=N, N_PTS_PCUT=N, N_PTS_PCUT_HI=N))     # one species: another layout
    with pytest.raises(ValueError, match="layout"):
        mcs.driver.run(prob, prim, None, n_itrs=1, max_pcuts=2, species_backends=[oracle_backend(other)])


def test_an_ion_does_not_read_what_earlier_ions_deposited():
    """The premise: He run from the protons' end state (their energy_transfer_pool copied into its energy_recv_pool) and He run
    on a fresh context give the same particles, saved arrays and int64 deltas in every pcut."""
    prob = mixed()
    a, b = oracle_backend(prob), oracle_backend(prob)
    start_species(a, prob, 1, 1)
    for ip in range(1, N_PCUTS + 1):
        ns = a.run_pcut(ip, 0)
        if ns == 0:
            break
        a.new_pcut(max(N // ns, 1))
    assert np.any(a.layout.view(a.read_tallies()[0], "energy_transfer_pool"))
    inj = mcs.inputs.init_pop_host(prob, 2)
    sp = prob.cfg.species[1]
    pmax = mcs.inputs.get_pmax_cutoff(prob.Emax_keV, prob.Emax_per_aa_keV, prob.pmax, sp.aa)
    ewf = 1.0 / prob.cfg.species[-1].density
    for be in (a, b):
        be.begin_species(1, 2, sp.aa, abs(sp.zz), pmax, sp.density, ewf)
        be.set_fluxes(inj.pxx_flux, inj.pxz_flux, inj.energy_flux)
        be.init_pop(inj, 0, inj.n_pts_use, inj.n_pts_use)
    assert np.any(a.layout.view(a.read_tallies()[0], "energy_recv_pool"))
    for ip in range(1, N_PCUTS + 1):
        i0 = [be.read_tallies()[1] for be in (a, b)]
        assert_pop_equal(a.get_population(), b.get_population(), f"pcut {ip}")
        na, nb = a.run_pcut(ip, 0), b.run_pcut(ip, 0)
        assert na == nb
        (sa, la), (sb, lb) = a.get_saved(), b.get_saved()
        assert np.array_equal(la, lb)
        assert_pop_equal(sa, sb, f"pcut {ip} saved")
        assert np.array_equal(a.read_tallies()[1] - i0[0], b.read_tallies()[1] - i0[1]), f"pcut {ip}: int64 deltas"
        if na == 0:
            break
        a.new_pcut(max(N // na, 1)); b.new_pcut(max(N // nb, 1))


def test_accumulate_tallies_refuses_null_contexts():
    lib = mcs.capi.load_library()
    assert lib.mcs_accumulate_tallies(None, None) != 0
    assert b"null" in lib.mcs_last_error()
    assert lib.mcs_k1_blocks_per_cu(None) == 0 and len(lib.mcs_last_error()) > 0
