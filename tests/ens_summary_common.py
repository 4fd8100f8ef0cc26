"""Plain-numpy restatement of the summary of a word range of an ensemble slot (include/mcs.h, mcs_ens_summarize), shared by
test_ens_summary_host.py and test_gpu_ens_summary.py.  Nothing here imports the package's ensemble module.

For the words w of one range of a slot with n >= 2 samples:
  finite word    mean[w] and M2[w] both finite; n_nonfinite counts the others, which take part in nothing else
  amax           max |mean[w]| over the finite words, 0 for an empty range
  selected word  finite, |mean[w]| > 0 and |mean[w]| >= floor_frac * amax
  per selected word   se = sqrt(M2[w] / (n (n - 1))), the denominator float(n) * float(n - 1); rel = se / |mean[w]|
  max_rel, argmax (the lowest w - first that attains it; -1: nothing selected), n_over (rel > tol)
  sum_se, sum_abs_mean, sum_rel2: math.fsum over the selected words -- the correctly rounded sums, which no order of adding comes
  further from than n_selected * 2^-53 relative (non-negative terms)

numpy's sqrt and / are the correctly rounded elementwise operations."""
import math

import numpy as np

from ensemble_common import HISTS, SPECIES_TALLIES

EXACT = ("amax", "max_rel", "argmax", "n_selected", "n_over", "n_nonfinite")
SUMS = ("sum_se", "sum_abs_mean", "sum_rel2")
FIELDS = EXACT + SUMS
# the parts of the two sample vectors in the order of the header: a species sample is parts 1 - 4, an iteration sample the words
# [esc_flux, energy_recv_pool) and then the scalars
SPECIES_ORDER = SPECIES_TALLIES + ("energy_recv_pool", "num_crossings") + tuple(f"{h}_{ax}" for h in HISTS for ax in ("mom", "tht"))


def restate(mean, m2, n, floor_frac, tol):
    """-> dict of FIELDS for the words of one range."""
    mean, m2 = np.asarray(mean, dtype=np.float64).ravel(), np.asarray(m2, dtype=np.float64).ravel()
    out = dict(amax=0.0, max_rel=0.0, argmax=-1, n_selected=0, n_over=0, n_nonfinite=0, sum_se=0.0, sum_abs_mean=0.0, sum_rel2=0.0)
    ok = np.isfinite(mean) & np.isfinite(m2)
    out["n_nonfinite"] = int((~ok).sum())
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return out
    absm = np.abs(mean[idx])
    out["amax"] = float(np.max(absm))
    keep = (absm > 0.0) & (absm >= floor_frac * out["amax"])
    idx, absm = idx[keep], absm[keep]
    if idx.size == 0:
        return out
    se = np.sqrt(m2[idx] / (float(n) * float(n - 1)))
    rel = se / absm
    top = np.max(rel)
    out.update(n_selected=int(idx.size), max_rel=float(top), argmax=int(idx[np.flatnonzero(rel == top)[0]]), n_over=int((rel > tol).sum()),
               sum_se=math.fsum(se.tolist()), sum_abs_mean=math.fsum(absm.tolist()), sum_rel2=math.fsum((rel * rel).tolist()))
    return out


def value_of(statistic, r, n):
    """The value of a trigger from a restated summary (nan: fewer than two samples or nothing selected)."""
    if n < 2 or r["n_selected"] == 0:
        return float("nan")
    return {"max": lambda: r["max_rel"], "rms": lambda: math.sqrt(r["sum_rel2"] / r["n_selected"]),
            "weighted": lambda: r["sum_se"] / r["sum_abs_mean"], "fraction_over": lambda: r["n_over"] / r["n_selected"]}[statistic]()


def same_bits(x, y):
    return np.array_equal(np.array([x], dtype=np.float64).view(np.uint64), np.array([y], dtype=np.float64).view(np.uint64))


def as_dict(s):
    """The fields of a summary object of the package, by the names of the header."""
    return {k: getattr(s, k) for k in FIELDS}


def assert_exact(got, want, what=""):
    for k in EXACT:
        same = same_bits(got[k], want[k]) if isinstance(want[k], float) else int(got[k]) == want[k]
        assert same, f"{what}: {k} = {got[k]!r}, the restatement has {want[k]!r}"


def assert_sums(got, want, what=""):
    """Within n_selected * 2^-53 relative of the correctly rounded sums (equal where nothing is selected)."""
    bound = want["n_selected"] * 2.0 ** -53
    for k in SUMS:
        assert abs(got[k] - want[k]) <= bound * abs(want[k]), f"{what}: {k} = {got[k]!r}, fsum gives {want[k]!r}; relative bound {bound:.3e}"


def slot_vectors(e, slot):
    """(mean, M2) of a whole slot as the accumulator holds them."""
    total = e.layout.iteration_total if slot == e.iteration_slot else e.layout.species_total
    return e._read(slot, 0, 0, total), e._read(slot, 1, 0, total)


def species_offsets(L):
    """name -> (first word, shape) in the species sample vector, from the tally layout L and SPECIES_ORDER."""
    ng, nm, nt = L.n_grid, L.shapes["psd"][2], L.shapes["psd"][1]
    shapes = {name: L.shapes[name] for name in SPECIES_TALLIES}
    shapes.update(energy_recv_pool=(ng,), num_crossings=(ng,))
    for h in HISTS:
        shapes[h + "_mom"], shapes[h + "_tht"] = (ng, nm), (ng, nt)
    out, o = {}, 0
    for name in SPECIES_ORDER:
        out[name] = (o, shapes[name])
        o += int(np.prod(shapes[name]))
    return out, o


def iteration_offsets(L, names):
    """name -> (first word, shape) in the iteration sample vector for the named sections; the vector's length."""
    o = L.offsets
    n_sums = o["energy_recv_pool"] - o["esc_flux"]
    out = {name: ((n_sums if name == "scalars" else o[name] - o["esc_flux"]), L.shapes[name]) for name in names}
    return out, n_sums + (L.total - o["scalars"])
