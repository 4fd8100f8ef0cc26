"""What the tests of the source slot (the photon spectrum summed over species; include/mcs.h, "source sample") share: the small photon
layout, crafted spectra of three species, and the restatement of the deposit rule and of the update in Python floats."""
import numpy as np

from conftest import mcs

cons, ens = mcs.consumers, mcs.ensemble

# the small layout of test_gpu_ens_photons.py: 3 shells; 23 / 17 / 11 words at 0 / 9 / 20 of 31
LAYOUT = cons.PhotonLayout(3, {"synch": 23, "ic": 17, "pion": 11}, {"synch": 0, "ic": 9, "pion": 20}, 31)
N_WORDS = LAYOUT.offsets()["_total"]
# the processes of the three crafted species: every process is lit in one species, in two, or (a word on the floor in all) in none
SPECIES_PROCESSES = (("pion",), ("synch", "ic"), ("pion", "synch"))
FLOOR = 1.0e-99
# a layout of two shells and a handful of energy words, for tests of the bookkeeping; its two species; what mcs_photon_observe takes
# for it: the emission words per process (one more than the spectrum has) and the shell ends
SMALL_LAYOUT = cons.PhotonLayout(2, {"synch": 7, "ic": 5, "pion": 3}, {"synch": 0, "ic": 2, "pion": 6}, 9)
SMALL_PROCESSES = (("synch", "pion"), ("ic",))
SMALL_N_PHOTON = {p: n + 1 for p, n in SMALL_LAYOUT.n.items()}
SMALL_ENDS = [1, 9, 30]


def crafted_species(it, seed=0, layout=LAYOUT, species_processes=SPECIES_PROCESSES):
    """The ObservedSpectra of the species of iteration `it`.  Per process word, by a pattern that is the same in every species and
    iteration: one in five on the floor (lit in no species), one in five a value of a few 1e-99 (above the floor, and 1e-99 + x != x),
    the others over forty decades; on top of that every species has words of its own on the floor."""
    out = []
    for s, processes in enumerate(species_processes):
        rng = np.random.default_rng(1000 * seed + 10 * it + s)
        per = {}
        for p in processes:
            shape = (layout.rows, layout.n[p])
            kind = np.random.default_rng(77 + len(p)).integers(0, 5, shape)
            a = rng.uniform(1, 10, shape) * 10.0 ** rng.integers(-30, 10, shape)
            a[kind == 1] = rng.integers(2, 10, shape)[kind == 1] * 1.0e-99
            a[kind == 0] = FLOOR
            a[rng.random(shape) < 0.15] = FLOOR
            per[p] = a
        out.append(cons.ObservedSpectra(tuple(per), per, {}, cons.photon_total(per, layout), None, layout, 0.1))
    return out


def deposit_restated(samples):
    """The pending vector after the deposits of `samples` (sample vectors, in deposit order): the rule of include/mcs.h word by word in
    Python floats."""
    out = np.empty(len(samples[0]))
    for w in range(out.size):
        pending = None
        for k, x in enumerate(samples):
            v = float(x[w])
            lit = v if v > 1.0e-99 else 0.0
            pending = 1.0e-99 + lit if k == 0 else pending + lit
        out[w] = pending
    return out


def welford_restated(samples):
    """(mean, M2) of the sample vectors in order, the update of every slot word by word in Python floats."""
    mean, m2 = [0.0] * len(samples[0]), [0.0] * len(samples[0])
    for n, x in enumerate(samples, 1):
        for w in range(len(mean)):
            v = float(x[w])
            d = v - mean[w]
            mean[w] = mean[w] + d / float(n)
            m2[w] = m2[w] + d * (v - mean[w])
    return np.array(mean), np.array(m2)


def chan_restated(a, na, b, nb):
    """(mean, M2) of the merge of a = (mean, M2) with na samples and b with nb."""
    n = float(na + nb)
    d = b[0] - a[0]
    return a[0] + d * (float(nb) / n), (a[1] + b[1]) + (d * d) * (float(na) * float(nb) / n)


def slot_words(e, slot, n=N_WORDS):
    return e._read(slot, 0, 0, n), e._read(slot, 1, 0, n)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
