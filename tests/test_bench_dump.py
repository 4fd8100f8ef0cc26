"""bench.py --dump-outputs on the CPU: what the last step of driver.run hands its caller, as bench.py collects and
writes it (the oracle backend stands in for the GPU one; both fill the same RunResult)."""
import os
import sys

import numpy as np

from conftest import ROOT, mcs, make_problem, oracle_backend

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_step_outputs_are_the_last_step_results(tmp_path):
    n_itrs = 2
    prob = make_problem(400, num_iterations=n_itrs + 3)       # room for more iterations than ran, as with --full
    be = oracle_backend(prob, nthreads=4)
    sm = mcs.iter_finalize.SmoothingConfig(smooth_shocks=True)
    res = mcs.driver.run(prob, be, None, n_itrs=n_itrs, max_pcuts=4, smoothing=sm, species_tallies="light")
    arrays = bench.step_outputs(prob, be.layout, res, n_itrs, smooth=True)
    bench.dump_outputs(str(tmp_path), arrays)
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(got) == set(arrays)
    assert all(a.dtype == np.float64 for a in got.values())
    L = be.layout
    for name in L.offsets:
        want = L.view(res.tallies_f64, name)
        if name in ("px_esc_feb", "energy_esc_feb"):
            assert got["tally_" + name].shape == (n_itrs, prob.params.n_ions)
            want = want[:n_itrs]
        assert np.array_equal(got["tally_" + name], want), name
    assert np.array_equal(got["tally_i64"], res.tallies_i64.astype(np.float64))
    _, fin, ion = res.iter_finals[-1]
    assert np.array_equal(got["ion_finalize_dNdp_cr"], ion.dNdp_cr)
    assert got["iter_finalize_Gamma_downstream"] == fin.Gamma_downstream
    assert np.array_equal(got["profile_ux"], prob.ux)


def test_dump_is_bounded_by_a_fixed_sample(tmp_path):
    big = 3 * bench.DUMP_LIMIT_BYTES // 8 // 8                 # three arrays of 3/8 of the limit each
    arrays = {f"a{k}": np.arange(big, dtype=np.float64) + k for k in range(3)}
    arrays["small"] = np.ones(10)
    bench.dump_outputs(str(tmp_path / "one"), dict(arrays))
    bench.dump_outputs(str(tmp_path / "two"), dict(arrays))
    files = sorted(os.listdir(tmp_path / "one"))
    assert files == sorted(k + ".npy" for k in arrays)
    assert sum(os.path.getsize(tmp_path / "one" / f) for f in files) <= bench.DUMP_LIMIT_BYTES
    for f in files:
        a, b = np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f)
        assert np.array_equal(a, b), f
    s = np.load(tmp_path / "one" / "a0.npy")                   # the first sample brings the total under the limit
    assert s.size == bench.DUMP_SAMPLE and np.all(np.diff(s) > 0) and np.all(np.isin(s, arrays["a0"]))
    for k in ("a1", "a2", "small"):
        assert np.array_equal(np.load(tmp_path / "one" / f"{k}.npy"), arrays[k]), k
