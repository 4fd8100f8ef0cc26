"""Plain-numpy restatement of the comparison of two ensemble slots (include/mcs.h, mcs_ens_compare), and the crafted pair of
sample sets it is tested on; shared by test_ens_compare_host.py and test_gpu_ens_compare.py.  Nothing here imports the package's
ensemble module.

For the words w of one range of slot A (mean ma, M2 qa, n_a >= 2 samples) and slot B, every operation a separate rounding:
  va = qa[w] / (float(n_a) * float(n_a - 1)), vb likewise; s2 = va + vb; d = ma[w] - mb[w]; scale = max(|ma[w]|, |mb[w]|)
  finite word      ma, qa, mb, qb, d, s2 all finite; n_nonfinite counts the others, which take part in nothing else
  amax             max scale over the finite words, 0 for an empty range
  selected word    finite, scale > 0 and scale >= floor_frac * amax
  degenerate word  selected, s2 == 0 and d != 0: in n_degenerate, sum_abs_diff, sum_scale and nothing else
  z                0 where s2 == 0 and d == 0, else d / sqrt(s2)
  over the selected words that are not degenerate: max_abs_z, argmax (the lowest w - first that attains it; -1: none), n_over
  (|z| > zcut), sum_z, sum_abs_z, sum_z2; over all selected words: sum_abs_diff, sum_scale
The sums are math.fsum, the correctly rounded ones.  No order of adding comes further from the exact sum of n non-negative terms than
(n - 1) * 2^-53 relative (to first order: every partial sum is at most the total), nor from the exact sum of n signed terms than
(n - 1) * 2^-53 times the sum of their absolute values; the bounds below are n_selected of those units.

numpy's sqrt and / are the correctly rounded elementwise operations."""
import math

import numpy as np

from ensemble_common import SPECIES_TALLIES, species_parts, stat_of
from ens_summary_common import SPECIES_ORDER, same_bits

EXACT = ("amax", "max_abs_z", "argmax", "n_selected", "n_over", "n_nonfinite", "n_degenerate")
POSITIVE_SUMS = ("sum_abs_z", "sum_z2", "sum_abs_diff", "sum_scale")
FIELDS = EXACT + ("sum_z",) + POSITIVE_SUMS
N_A, N_B = 5, 4
TIE = (1000, 21001, 21002)         # words of psd (zone 0) with the same samples: two more than 8192 words apart, the third beside the second
SHIFTED_ZONES = (40, 50)           # psd of B is 1.5 times its recipe there
UNSHIFTED_ZONES = (60, 70)


def per_word(ma, qa, n_a, mb, qb, n_b):
    """-> (finite, d, s2, scale) of every word."""
    ma, qa, mb, qb = (np.asarray(x, dtype=np.float64).ravel() for x in (ma, qa, mb, qb))
    with np.errstate(all="ignore"):
        va = qa / (float(n_a) * float(n_a - 1))
        vb = qb / (float(n_b) * float(n_b - 1))
        s2 = va + vb
        d = ma - mb
        scale = np.maximum(np.abs(ma), np.abs(mb))
    finite = np.isfinite(ma) & np.isfinite(qa) & np.isfinite(mb) & np.isfinite(qb) & np.isfinite(d) & np.isfinite(s2)
    return finite, d, s2, scale


def restate(ma, qa, n_a, mb, qb, n_b, floor_frac, zcut, with_z=False):
    """-> dict of FIELDS for the words of one range (with_z: and "z", the z of the selected non-degenerate words in word order)."""
    finite, d, s2, scale = per_word(ma, qa, n_a, mb, qb, n_b)
    out = dict(amax=0.0, max_abs_z=0.0, argmax=-1, n_selected=0, n_over=0, n_nonfinite=int((~finite).sum()), n_degenerate=0, sum_z=0.0,
               sum_abs_z=0.0, sum_z2=0.0, sum_abs_diff=0.0, sum_scale=0.0)
    if with_z:
        out["z"] = np.zeros(0)
    idx = np.flatnonzero(finite)
    if idx.size == 0:
        return out
    out["amax"] = float(np.max(scale[idx]))
    idx = idx[(scale[idx] > 0.0) & (scale[idx] >= floor_frac * out["amax"])]
    if idx.size == 0:
        return out
    degenerate = (s2[idx] == 0.0) & (d[idx] != 0.0)
    out.update(n_selected=int(idx.size), n_degenerate=int(degenerate.sum()), sum_abs_diff=math.fsum(np.abs(d[idx]).tolist()),
               sum_scale=math.fsum(scale[idx].tolist()))
    idx = idx[~degenerate]
    if idx.size == 0:
        return out
    z = np.zeros(idx.size)
    some = s2[idx] != 0.0
    with np.errstate(all="ignore"):
        z[some] = d[idx][some] / np.sqrt(s2[idx][some])
    az = np.abs(z)
    top = np.max(az)
    out.update(max_abs_z=float(top), argmax=int(idx[np.flatnonzero(az == top)[0]]), n_over=int((az > zcut).sum()), sum_z=math.fsum(z.tolist()),
               sum_abs_z=math.fsum(az.tolist()), sum_z2=math.fsum((z * z).tolist()))
    if with_z:
        out["z"] = z
    return out


def swapped(r):
    """What restate gives with A and B exchanged, from what it gave: sum_z changes its sign bit unless it is zero."""
    out = dict(r)
    out["sum_z"] = -r["sum_z"] if r["sum_z"] != 0.0 else r["sum_z"]
    return out


def value_of(statistic, r):
    """The value of an agreement from a restated difference (nan where it has none)."""
    if statistic == "weighted_diff":
        return r["sum_abs_diff"] / r["sum_scale"] if r["n_selected"] > 0 else float("nan")
    n = r["n_selected"] - r["n_degenerate"]
    if n <= 0:
        return float("nan")
    return {"max_z": lambda: r["max_abs_z"], "chi2_per_word": lambda: r["sum_z2"] / n, "fraction_over": lambda: r["n_over"] / n,
            "mean_z": lambda: r["sum_z"] / n}[statistic]()


def as_dict(d):
    """The fields of a difference object of the package (or of the ctypes struct), by the names of the header."""
    return {k: getattr(d, k) for k in FIELDS}


def assert_exact(got, want, what=""):
    for k in EXACT:
        same = same_bits(got[k], want[k]) if isinstance(want[k], float) else int(got[k]) == want[k]
        assert same, f"{what}: {k} = {got[k]!r}, the restatement has {want[k]!r}"


def assert_sums(got, want, what=""):
    """sum_z within n_selected * 2^-53 * sum_abs_z of fsum; the sums of non-negative terms within n_selected * 2^-53 relative."""
    bound = want["n_selected"] * 2.0 ** -53
    assert abs(got["sum_z"] - want["sum_z"]) <= bound * want["sum_abs_z"], \
        f"{what}: sum_z = {got['sum_z']!r}, fsum gives {want['sum_z']!r}; bound {bound * want['sum_abs_z']:.3e}"
    for k in POSITIVE_SUMS:
        assert abs(got[k] - want[k]) <= bound * abs(want[k]), f"{what}: {k} = {got[k]!r}, fsum gives {want[k]!r}; relative bound {bound:.3e}"


def assert_same_bits(a, b, what="", but_sign_of_sum_z=False):
    """Two results of the package, field by field."""
    for k in FIELDS:
        x, y = a[k], b[k]
        if k == "sum_z" and but_sign_of_sum_z and y != 0.0:
            assert same_bits(x, -y), f"{what}: sum_z = {x!r} and {y!r} differ in more than the sign bit"
        else:
            assert same_bits(x, y) if isinstance(y, float) else x == y, f"{what}: {k} = {x!r} and {y!r}"


def crafted_pair(L, seed=0):
    """(bufs_a, bufs_b): N_A and N_B tally buffers (f, i) from ONE base value per word, uniform in 1..10 times 10^k, k in -60..40:
    every sample is base * (1 + 0.1 * normal) from a seed of its own.  On top of that, in this order: one word in 25 is constant
    within A (its base) and within B (1.25 times it); psd of B is multiplied by 1.5 in SHIFTED_ZONES; every seventh word is 1e-99 in
    all samples of both; the words TIE of psd have the same samples -- near 5e40, the largest values of psd, the sets 0.2 % apart with a
    spread of 1e-9: their |z| have equal bits and are the largest by far."""
    common = np.random.default_rng(seed + 5000)
    base = common.uniform(1.0, 10.0, L.total) * 10.0 ** common.integers(-60, 40, L.total)
    const = common.random(L.total) < 0.04
    i_base = common.integers(2 ** 20, 2 ** 50, L.n_i64)
    z0, z1 = SHIFTED_ZONES
    sets = []
    for which, n in enumerate((N_A, N_B)):
        bufs = []
        for k in range(n):
            rng = np.random.default_rng(seed + 100 * which + k)
            f = base * (1.0 + 0.1 * rng.standard_normal(L.total))
            f[const] = base[const] * (1.0 if which == 0 else 1.25)
            if which == 1:
                L.view(f, "psd")[z0:z1] *= 1.5
            f[::7] = 1e-99
            psd = L.view(f, "psd").reshape(-1)
            for w in TIE:
                psd[w] = (5.0e40 if which == 0 else 4.99e40) * (1.0 + 1e-9 * k)
            i = (i_base * (1.0 + 0.1 * rng.standard_normal(L.n_i64))).astype(np.int64)
            i[0], i[1], i[2] = 2 ** 50, 0, 12345            # (the same in every sample of both sets)
            bufs.append((f, i))
        sets.append(bufs)
    return sets[0], sets[1]


def species_vectors(L, bufs):
    """(mean, M2) of the species sample vector over the buffers, by the restatement of ensemble_common.py, in SPECIES_ORDER."""
    st = stat_of([species_parts(L, f, i) for f, i in bufs])
    return (np.concatenate([st.mean[name].ravel() for name in SPECIES_ORDER]), np.concatenate([st.m2[name].ravel() for name in SPECIES_ORDER]))


def check_recipe(L, va, vb):
    """The conditions the crafted pair has to meet, on the restatement alone.  va, vb: (mean, M2) of the whole species vector of A, B."""
    assert L.offsets["psd"] == 0 and SPECIES_TALLIES[0] == "psd"        # (a word of psd is that word of the buffer and of the vector)
    r = restate(*va, N_A, *vb, N_B, 0.0, 3.0, with_z=True)
    assert 0 < r["n_over"] < r["n_selected"] - r["n_degenerate"], r
    assert r["n_degenerate"] > 0 and r["n_nonfinite"] == 0, r
    assert np.count_nonzero(r["z"] == 0.0) > 0
    per_zone = int(np.prod(L.shapes["psd"][1:]))
    chi2 = []
    for z0, z1 in (SHIFTED_ZONES, UNSHIFTED_ZONES):
        s = slice(z0 * per_zone, z1 * per_zone)
        rz = restate(va[0][s], va[1][s], N_A, vb[0][s], vb[1][s], N_B, 0.0, 3.0)
        chi2.append(value_of("chi2_per_word", rz))
    assert SHIFTED_ZONES[1] - SHIFTED_ZONES[0] == UNSHIFTED_ZONES[1] - UNSHIFTED_ZONES[0] and chi2[0] > chi2[1], chi2
    # the tie: equal bits of |z|, the largest of psd
    n_psd = int(np.prod(L.shapes["psd"]))
    p = restate(va[0][:n_psd], va[1][:n_psd], N_A, vb[0][:n_psd], vb[1][:n_psd], N_B, 0.0, 3.0)
    assert TIE[1] - TIE[0] > 8192 and p["argmax"] == TIE[0], p
    for w in TIE:
        one = restate(va[0][w:w + 1], va[1][w:w + 1], N_A, vb[0][w:w + 1], vb[1][w:w + 1], N_B, 0.0, 3.0)
        assert same_bits(one["max_abs_z"], p["max_abs_z"]) and same_bits(one["amax"], p["amax"]), w
    return r


def compare_ranges(L, sp_off, total):
    """The ranges [(first, count, floor_frac, zcut)] of the exact-fields test for the species slot, modelled on species_ranges of
    test_gpu_ens_summary.py."""
    n_psd = int(np.prod(L.shapes["psd"]))
    per_zone = n_psd // L.n_grid
    r = [(0, total, 0.0, 3.0), (0, total, 1e-3, 3.0), (0, total, 1.0, 3.0)]
    for name, (first, shape) in sp_off.items():
        n = int(np.prod(shape))
        r += [(first, n, 1e-3, 2.0), (first, n, 1.0, 2.0)]
        if 50 <= n < 100000 and not name.endswith(("_mom", "_tht")):
            r.append((first, n, 0.0, 2.0))
    r += [(12345, 1, 1e-3, 0.0), (777, 0, 1e-3, 0.0), (total, 0, 0.0, 0.0), (total - 1, 1, 0.0, 0.0),
          (4097, 300000, 1e-3, 1.0), (4097, 300001, 0.0, 1.0), (4096, 300001, 1e-3, 1.0),         # odd .. odd, odd .. even, even .. odd
          (5, 2, 0.0, 0.0), (5, 1, 0.0, 0.0), (6, 1, 1.0, 0.0), (3, 4, 0.0, 0.0),
          (SHIFTED_ZONES[0] * per_zone, (SHIFTED_ZONES[1] - SHIFTED_ZONES[0]) * per_zone, 0.0, 3.0),     # zone slices of psd
          (UNSHIFTED_ZONES[0] * per_zone, (UNSHIFTED_ZONES[1] - UNSHIFTED_ZONES[0]) * per_zone, 0.0, 3.0),
          (10 * per_zone, 27 * per_zone, 1e-3, 3.0),
          (1000, 50000, 0.0, 3.0), (30000, 50000, 0.0, 3.0),                                      # overlapping
          (0, n_psd, 0.0, 3.0),                                                                   # the tie, in different blocks
          (TIE[0], TIE[1] - TIE[0] + 1, 1.0, 3.0),                                                # ... alone by the floor
          (TIE[1], 2, 0.0, 3.0), (TIE[1], 2, 1.0, 1e9)]                                           # ... alone by the range
    return r
