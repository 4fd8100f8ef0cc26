"""Plain-numpy restatement of the ensemble statistics (include/mcs.h, "ensemble statistics"), shared by test_ensemble_host.py and
test_gpu_ensemble.py.  Nothing here imports the package's ensemble module: the sample vectors, the update and the merge are
written out again from the statements of the header, so that the package's two implementations are compared with a third.

  update   n += 1; d = x - mean; mean = mean + d / n; M2 = M2 + d * (x - mean)
  merge    n = na + nb; d = mb - ma; mean = ma + d * (nb / n); M2 = (qa + qb) + (d * d) * (na * nb / n)

numpy's elementwise operations round once each and form no fma, as the library's build (-ffp-contract=off)."""
import numpy as np

HISTS = ("psd", "therm_sf", "therm_pf")
SPECIES_TALLIES = ("psd", "therm_sf", "therm_pf", "esc_psd_up", "esc_psd_down", "pxx_flux", "pxz_flux", "energy_flux")
INCREMENTS = ("esc_flux", "esc_energy_eff", "esc_num_eff", "spectra_coupled", "spectra_sf", "spectra_pf")
AS_IS = ("weight_coupled", "energy_transfer_pool", "scalars")
THREADS = 256          # block size of the elementwise kernels (csrc/mcs_ensemble.hip)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_words(a, b):
    """Bit-equal, where a NaN equals a NaN (the bits of a NaN that went through an update are nobody's promise)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def marginals(hist):
    """hist [n_grid][ntht+2][nmom+2] -> (momentum marginal [n_grid][nmom+2], angle marginal [n_grid][ntht+2]): serial sums in
    ascending index order, starting from the first term (np.sum is pairwise and would round differently)."""
    mom = hist[:, 0, :].copy()
    for j in range(1, hist.shape[1]):
        mom = mom + hist[:, j, :]
    tht = hist[:, :, 0].copy()
    for i in range(1, hist.shape[2]):
        tht = tht + hist[:, :, i]
    return mom, tht


def species_parts(L, f, i):
    """name -> array of the species sample of the tally buffers (f, i)."""
    out = {name: L.view(f, name).copy() for name in SPECIES_TALLIES}
    out["energy_recv_pool"] = L.view(f, "energy_recv_pool").copy()
    out["num_crossings"] = i[:L.n_grid].astype(np.float64)
    for h in HISTS:
        out[h + "_mom"], out[h + "_tht"] = marginals(L.view(f, h))
    return out


def iteration_parts(L, f, f_begin):
    """name -> array of the iteration sample: the never-reset sections as their growth since the buffer f_begin, the rest as it stands."""
    out = {name: L.view(f, name) - L.view(f_begin, name) for name in INCREMENTS}
    out.update({name: L.view(f, name).copy() for name in AS_IS})
    return out


class Stat:
    """n, mean, M2 of a sequence of samples (dicts name -> array)."""

    def __init__(self):
        self.n, self.mean, self.m2 = 0, None, None

    def add(self, parts):
        if self.mean is None:
            self.mean = {k: np.zeros_like(v) for k, v in parts.items()}
            self.m2 = {k: np.zeros_like(v) for k, v in parts.items()}
        self.n += 1
        n = float(self.n)
        for k, x in parts.items():
            mean, m2 = self.mean[k], self.m2[k]
            d = x - mean
            mean = mean + d / n
            m2 = m2 + d * (x - mean)
            self.mean[k], self.m2[k] = mean, m2
        return self

    def merged_with(self, other):
        """Chan's merge of other into a copy of self."""
        out = Stat()
        na, nb = self.n, other.n
        n = float(na + nb)
        out.n = na + nb
        out.mean, out.m2 = {}, {}
        for k in self.mean:
            ma, mb, qa, qb = self.mean[k], other.mean[k], self.m2[k], other.m2[k]
            d = mb - ma
            out.mean[k] = ma + d * (float(nb) / n)
            out.m2[k] = (qa + qb) + (d * d) * (float(na) * float(nb) / n)
        return out


def stat_of(samples):
    s = Stat()
    for p in samples:
        s.add(p)
    return s


def check_one_merge_of_every_kind(a, b, lens, only_b):
    """a.merge(b), once, of two ensembles of either implementation that hold samples in slots of every kind -- the keys of lens, slot ->
    length of its vectors; only_b: the slots that only b has sampled.  Every slot of a is then, bit for bit, Chan's formula restated
    here on the vectors read before the merge (a copy of b's where a had none), the counts add, and b is what it was."""
    read = lambda e, s: (e._read(s, 0, 0, lens[s]), e._read(s, 1, 0, lens[s]))
    na = {s: a.count(s) for s in lens}
    nb = {s: b.count(s) for s in lens}
    assert all(lens[s] % THREADS != 0 for s in lens), "a vector length is a multiple of the block size: the grid-stride tail would not run"
    assert all(nb[s] > 0 for s in lens) and sorted(s for s in lens if na[s] == 0) == sorted(only_b) and len({na[s] for s in lens}) == 2
    assert all(na[s] != nb[s] for s in lens)
    va = {s: read(a, s) for s in lens if na[s]}
    vb = {s: read(b, s) for s in lens}
    a.merge(b)
    for s in lens:
        assert a.count(s) == na[s] + nb[s] and b.count(s) == nb[s], s
        (mb, qb), got, still = vb[s], read(a, s), read(b, s)
        assert same_words(still[0], mb) and same_words(still[1], qb), f"slot {s}: the source of a merge is unchanged"
        if na[s] == 0:
            assert same_words(got[0], mb) and same_words(got[1], qb), f"slot {s}: a slot that only the source had is a copy"
            continue
        ma, qa = va[s]
        n = float(na[s] + nb[s])
        with np.errstate(invalid="ignore"):
            d = mb - ma
            mean, m2 = ma + d * (float(nb[s]) / n), (qa + qb) + (d * d) * (float(na[s]) * float(nb[s]) / n)
        assert np.isfinite(m2).any() and np.nanmax(m2) > 0 and not bits_equal(mean, ma), s
        assert same_words(got[0], mean), f"slot {s}: merged mean"
        assert same_words(got[1], m2), f"slot {s}: merged M2"


def crafted_buffers(L, n=5, seed=0):
    """n tally buffers (f, i): positive values over 1e-60 .. 1e40, every seventh word the floor 1e-99 in all of them, one word in
    twenty the same in all of them, num_crossings up to 2^50."""
    common = np.random.default_rng(seed + 1000)
    same = common.random(L.total) < 0.05
    same_val = common.uniform(1.0, 10.0, L.total) * 10.0 ** common.integers(-60, 40, L.total)
    out = []
    for k in range(n):
        rng = np.random.default_rng(seed + k)
        f = rng.uniform(1.0, 10.0, L.total) * 10.0 ** rng.integers(-60, 40, L.total)
        f[same] = same_val[same]
        f[::7] = 1e-99
        i = rng.integers(0, 2 ** 50, L.n_i64)
        i[0], i[1] = 2 ** 50, 0
        i[2] = 12345                   # (the same in every sample)
        out.append((f, i))
    return out


def assert_tail_is_exercised(E):
    """The lengths the kernels walk are no multiples of the block size: the grid-stride tail runs.  E: the fields of mcs_ens_layout."""
    for name in ("sp_total", "it_total", "sp_psd_mom"):
        assert E[name] % THREADS != 0, f"{name} = {E[name]} is a multiple of {THREADS}: change a bin count by one"
    assert (3 * E["sp_marg_mom_n"]) % THREADS != 0
