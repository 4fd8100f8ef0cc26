"""mcs_accumulate_tallies on the device, and the species of the bench mix on two contexts (driver.run(..., species_backends=[...]))
against the committed oracle run and against the one-context run on the GPU."""
import os

import numpy as np
import pytest

from conftest import ROOT, mcs, make_problem, hip_backend, start_species, bits, assert_pop_equal
from test_gpu_full_size import (_fixture_module, _binned_vs_fixture, LONG_SUM_RTOL, LONG_SUMS, TALLY_RTOL, MIX_KERNELS)

pytestmark = pytest.mark.gpu


class _Reduced(dict):
    """A reduction of the sequential run in the shape of a fixture file (_binned_vs_fixture reads .files)."""

    @property
    def files(self):
        return list(self)


def _random_tallies(L, seed):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(L.total) * 10.0 ** rng.integers(-30, 30, L.total)
    i = rng.integers(-2 ** 40, 2 ** 40, L.n_i64)
    return f, i


def test_accumulate_tallies_kernel_against_numpy():
    prob = make_problem(64)
    a, b = hip_backend(prob), hip_backend(prob)
    L = a.layout
    fa, ia = _random_tallies(L, 1)
    fb, ib = _random_tallies(L, 2)
    a.write_tallies(fa, ia); b.write_tallies(fb, ib)
    a.accumulate_tallies_from(b)
    (ga, ja), (gb, jb) = a.read_tallies(), b.read_tallies()
    r = mcs.capi.running_i64(L)
    for name in mcs.capi.RUNNING_F64:
        assert np.array_equal(bits(L.view(ga, name)), bits(L.view(fa, name) + L.view(fb, name))), name
        assert np.array_equal(bits(L.view(gb, name)), bits(np.zeros_like(L.view(fb, name)))), name
    for name in mcs.capi.PER_SPECIES_F64:
        assert np.array_equal(bits(L.view(ga, name)), bits(L.view(fa, name))), name
        assert np.array_equal(bits(L.view(gb, name)), bits(L.view(fb, name))), name
    assert np.array_equal(ja[r], ia[r] + ib[r]) and not np.any(jb[r])
    assert np.array_equal(ja[:L.n_grid], ia[:L.n_grid]) and np.array_equal(jb[:L.n_grid], ib[:L.n_grid])
    # the host fallback on the same inputs gives the same bits
    a.write_tallies(fa, ia); b.write_tallies(fb, ib)
    mcs.driver.accumulate_tallies_host(L, a, b)
    (gc, jc), (gd, jd) = a.read_tallies(), b.read_tallies()
    assert np.array_equal(bits(ga), bits(gc)) and np.array_equal(bits(gb), bits(gd))
    assert np.array_equal(ja, jc) and np.array_equal(jb, jd)
    # refusals change nothing
    other = hip_backend(make_problem(64, species=[mcs.inputs.Species(1.0, 1.0, 1e6, 1.0), mcs.inputs.Species(4.0, 2.0, 1e6, 0.1)]))
    for dst, src in ((a, other), (other, a), (a, a)):
        with pytest.raises(RuntimeError, match="mcs_accumulate_tallies"):
            dst.accumulate_tallies_from(src)
    (ha, ka) = a.read_tallies()
    assert np.array_equal(bits(ha), bits(ga)) and np.array_equal(ka, ja)
    for be in (a, b, other):
        be.destroy()


def test_config4_concurrent_iteration_vs_oracle_fixture():
    """test_config4_mixed_iteration_vs_oracle_fixture with He on a second context beside the protons."""
    fix = np.load(os.path.join(ROOT, "tests", "golden", "mixed_1e5.npz"))
    m = _fixture_module()
    prob = m.mixed_problem(100_000)
    hb, hb2 = hip_backend(prob), hip_backend(prob)
    L = hb.layout
    pools, ints = fix["species_energy_transfer_pool"], fix["species_tallies_i64"]
    kernels = []

    def species_end(i_iter, i_ion, f, i):
        kernels.append((hb2 if i_ion == 2 else hb).last_kernel())
        assert np.array_equal(i, ints[i_ion - 1]), f"ion {i_ion}: int64 tallies at the species end"
        got, want = L.view(f, "energy_transfer_pool"), pools[i_ion - 1]
        err = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
        assert err <= LONG_SUM_RTOL, f"ion {i_ion}: energy_transfer_pool off by {err:.3e}"
        if i_ion < len(prob.cfg.species):
            got[...] = want
            hb.write_tallies(f, i)
    res = mcs.driver.run(prob, hb, None, n_itrs=1, on_species_end=species_end, species_backends=[hb2])
    hb.destroy(); hb2.destroy()
    assert kernels == list(MIX_KERNELS[False]), kernels
    got = m.reduce_tallies(L, res.tallies_f64, res.tallies_i64, res.stats, with_ion=True)
    assert np.array_equal(got["stats"], fix["stats"])
    assert np.array_equal(got["tallies_i64"], fix["tallies_i64"])
    _binned_vs_fixture(got, fix, skip=("species_energy_transfer_pool", "species_tallies_i64"))
    sp = {ion: (k, t0, t1) for _, ion, k, t0, t1 in res.species_spans}
    assert [sp[i][0] for i in (1, 2, 3)] == [0, 1, 0]
    assert min(sp[1][2], sp[2][2]) > max(sp[1][1], sp[2][1]), f"the ion species did not overlap: {sp}"
    assert sp[3][1] >= max(sp[1][2], sp[2][2])


@pytest.mark.parametrize("fp32", [False, True])
def test_config4_concurrent_vs_sequential_1e6(fp32):
    """The bench mix at 10^6 per species: the concurrent iteration against the one-context one on the GPU, the electrons' pool
    pinned to the sequential run's bits."""
    m = _fixture_module()
    prob = m.mixed_problem(1_000_000, state_fp32=fp32)
    hb = hip_backend(prob)
    L = hb.layout
    ends, kernels = {}, []

    def seq_end(i_iter, i_ion, f, i):
        ends[i_ion] = (L.view(f, "energy_transfer_pool").copy(), i.copy())
    r1 = mcs.driver.run(prob, hb, None, n_itrs=1, finalize=True, on_species_end=seq_end)
    hb.destroy()
    prob = m.mixed_problem(1_000_000, state_fp32=fp32)
    hb, hb2 = hip_backend(prob), hip_backend(prob)

    def conc_end(i_iter, i_ion, f, i):
        kernels.append((hb2 if i_ion == 2 else hb).last_kernel())
        pool, i64 = ends[i_ion]
        assert np.array_equal(i, i64), f"ion {i_ion}: int64 tallies at the species end"
        if i_ion < len(prob.cfg.species):
            L.view(f, "energy_transfer_pool")[...] = pool
            hb.write_tallies(f, i)
    r2 = mcs.driver.run(prob, hb, None, n_itrs=1, finalize=True, on_species_end=conc_end, species_backends=[hb2])
    hb.destroy(); hb2.destroy()
    assert kernels == list(MIX_KERNELS[fp32]), kernels
    k = lambda r: [(s.i_iter, s.i_ion, s.i_pcut, s.n_pts_use, s.n_saved, s.i_mult) for s in r.stats]
    assert k(r1) == k(r2)
    assert np.array_equal(r1.tallies_i64, r2.tallies_i64)
    a = m.reduce_tallies(L, r1.tallies_f64, r1.tallies_i64, r1.stats, with_ion=True)
    b = m.reduce_tallies(L, r2.tallies_f64, r2.tallies_i64, r2.stats, with_ion=True)
    worst, n = _binned_vs_fixture(b, _Reduced(a))
    import dataclasses
    for (_, f1, g1), (_, f2, g2) in zip(r1.iter_finals, r2.iter_finals):
        for x, y in ((f1, f2), (g1, g2)):
            for fld in dataclasses.fields(x):
                u, v = getattr(x, fld.name), getattr(y, fld.name)
                if isinstance(u, (bool, str)) or u is None:
                    assert u == v, fld.name
                    continue
                u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
                scale = float(np.max(np.abs(u[np.isfinite(u)]))) if np.any(np.isfinite(u)) else 1.0
                assert np.allclose(u, v, rtol=0, atol=1e-10 * (scale or 1.0), equal_nan=True), fld.name
    print(f"config[4] {'fp32' if fp32 else 'fp64'} at 1e6: kernels {kernels}; {n} binned arrays, worst {worst[0]} {worst[1]:.2e}")


def test_an_ion_does_not_read_what_earlier_ions_deposited_gpu():
    """The premise on the GPU (kernel 6): He from the protons' end state and He on a fresh context, bit for bit in every pcut."""
    m = _fixture_module()
    N = 20000
    prob = m.mixed_problem(N)
    a, b = hip_backend(prob), hip_backend(prob)
    start_species(a, prob, 1, 1)
    for ip in range(1, 9):
        ns = a.run_pcut(ip, 0)
        if ns == 0:
            break
        a.new_pcut(max(N // ns, 1))
    inj = mcs.inputs.init_pop_host(prob, 2)
    sp = prob.cfg.species[1]
    pmax = mcs.inputs.get_pmax_cutoff(prob.Emax_keV, prob.Emax_per_aa_keV, prob.pmax, sp.aa)
    for be in (a, b):
        be.begin_species(1, 2, sp.aa, abs(sp.zz), pmax, sp.density, 1.0 / prob.cfg.species[-1].density)
        be.set_fluxes(inj.pxx_flux, inj.pxz_flux, inj.energy_flux)
        be.init_pop(inj, 0, inj.n_pts_use, inj.n_pts_use)
    assert np.any(a.layout.view(a.read_tallies()[0], "energy_recv_pool"))
    for ip in range(1, 12):
        i0 = [be.read_counters() for be in (a, b)]
        assert_pop_equal(a.get_population(), b.get_population(), f"pcut {ip}")
        na, nb = a.run_pcut(ip, 0), b.run_pcut(ip, 0)
        assert na == nb and a.last_kernel() == 6 and b.last_kernel() == 6
        (sa, la), (sb, lb) = a.get_saved(), b.get_saved()
        assert np.array_equal(la, lb)
        assert_pop_equal(sa, sb, f"pcut {ip} saved")
        fa, fb = a.finals(), b.finals()
        for key in fa:
            assert np.array_equal(bits(fa[key]), bits(fb[key])), (ip, key)
        assert np.array_equal(a.read_counters() - i0[0], b.read_counters() - i0[1]), f"pcut {ip}: int64 deltas"
        if na == 0:
            break
        a.new_pcut(max(N // na, 1)); b.new_pcut(max(N // nb, 1))
    a.destroy(); b.destroy()
