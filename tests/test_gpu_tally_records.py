"""The step where a particle event becomes numbers in the tally buffer, record by record, on a real MI355X.

mcs_eval_tally (include/mcs.h) runs caller-given records through the transport kernel's own flux_tally, particle_finish, tcut_track,
record stack (push_record / drain_events and the same-bin wave sum; form 2: push_record_k / drain_events_k), tally replicas and block
flush, in the translation unit they ship in; the results are read back with read_tallies, through fold_replicas.  The reference is the
oracle's serial walk of the same records with its deposit log (orc_eval_tally): tests/tally_common.py builds the records -- momenta
and angles within an ulp of every bin edge, the branch edges, the crossings, the exits, the stack shapes -- and turns the log into the
per-cell rule (no term: the bits stay; one term: bit for bit; k terms: the a-priori bound of a sum in any order), applied to the WHOLE
of the fp64 and int64 buffers after every launch.  tests/test_tally_records_host.py checks the records and the oracle on the CPU.

Regression cases found with these tests keep their records in REGRESSIONS below (none so far)."""
import ctypes as ct
import functools

import numpy as np
import pytest

from conftest import oracle_backend
import tally_common as tc

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 2)
COUNTS = {}
RESULTS = {}
REGRESSIONS = {}             # name -> (problem, rows [n][8] as hex floats, words): records that once differed, run by test_regressions


@functools.lru_cache(maxsize=None)
def material(name):
    """The launches of one problem with the oracle's logs, built once and never changed: (case, fp64 launches, fp32-unit launches)."""
    case = tc.make_case(name)
    R, _ = tc.build_records(case)
    ob = oracle_backend(case.prob)
    case.begin(ob)
    case.start = ob.read_tallies()        # a fresh context after begin_iteration / begin_species: where every run of a form starts
    launches = tc.split(case, R, ob) + tc.stack_shapes(case)
    tc.attach_logs(case, launches, ob)
    f32 = tc.attach_logs(case, [tc.to_f32_units(case, la) for la in launches], ob, f32=True)
    ob.destroy()
    for la in launches + f32:
        la.rec.setflags(write=False); la.word.setflags(write=False)
    return case, launches, f32


@pytest.fixture(scope="module")
def contexts():
    """One context per (problem, replicas), shared by the tests of the module."""
    from mcs_amd import hip_backend as hbm
    made = {}

    def get(name, rep):
        if (name, rep) not in made:
            be = hbm.HipBackend(0, options={"tally_replicas": rep})
            be.create(material(name)[0].prob)
            assert be.options()["tally_replicas"] == rep
            made[(name, rep)] = be
        return made[(name, rep)]
    yield get
    for be in made.values():
        be.destroy()
    print("\ntally records run (problem, form, replicas): launches, records, histogram deposits bit-exact / bounded:")
    for key, v in COUNTS.items():
        print("   ", key, v)


def run_form(hb, case, launches, form, what):
    """Every launch from the same state: that of a fresh context after begin_species, written back before each (begin_species leaves
    the running sums alone).  -> per launch the device's values of the cells its log names, and the counts."""
    L = hb.layout
    case.begin(hb)
    T0, I0 = case.start
    kept, n_rec, n_exact, n_bound = [], 0, 0, 0
    for n, la in enumerate(launches):
        hb.write_tallies(T0, I0)
        if n == 0:
            Tr, Ir = hb.read_tallies()
            assert np.array_equal(Tr.view(np.uint64), T0.view(np.uint64)) and np.array_equal(Ir, I0)
        hb.eval_tally(form, la.rec, la.word)
        T1, I1 = hb.read_tallies()
        e, b = tc.check_launch(L, la, T0, I0, T1, I1, f"{what}, launch '{la.name}' ({la.word.shape[0]} passes x {la.word.shape[1]} threads)")
        offs = np.unique(la.log[2][la.log[1] == 0])
        kept.append(T1[offs].copy())
        n_rec += int(np.count_nonzero((la.word >> np.uint64(40)) & np.uint64(3)))
        n_exact += e; n_bound += b
    return kept, (len(launches), n_rec, n_exact, n_bound)


@pytest.mark.parametrize("rep", (1, 0))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("problem", tc.PROBLEMS)
def test_records_against_the_log(contexts, problem, form, rep):
    case, launches, f32 = material(problem)
    hb = contexts(problem, rep)
    kept, counts = run_form(hb, case, f32 if form == 2 else launches, form, f"{problem}, form {form}, replicas {rep}")
    RESULTS[(problem, form, rep)] = kept
    COUNTS[(problem, form, rep)] = counts
    assert counts[1] > 4000 and counts[2] > 0


@pytest.mark.parametrize("rep", (1, 0))
@pytest.mark.parametrize("problem", tc.PROBLEMS)
def test_direct_and_stacked_forms_agree(contexts, problem, rep):
    """Form 0 and form 1 tally the same records, and each obeys the per-cell rule against the same reference
    (test_records_against_the_log).  Against each other: bit for bit where a cell has one term; where it has more, both lie within the
    bound of the exact sum, so they are within twice the bound of each other and no nearer is promised -- on the MI355X
    therm_pf[60, 37, 50] of "protons" (three terms) came out 2 ulp apart with the bound at 1.57 ulp."""
    case, launches, _ = material(problem)
    hb = contexts(problem, rep)
    got = []
    for form in (0, 1):
        if (problem, form, rep) not in RESULTS:
            RESULTS[(problem, form, rep)] = run_form(hb, case, launches, form, f"{problem}, form {form}, replicas {rep}")[0]
        got.append(RESULTS[(problem, form, rep)])
    L = hb.layout
    T0, I0 = case.start
    for la, a, b in zip(launches, got[0], got[1]):
        offs, serial, k, K, S, _, _ = tc.expected(L, T0, I0, la.log)
        bound = tc.bound(K, S)
        with np.errstate(invalid="ignore"):
            bad = np.where((k <= 1) | ~np.isfinite(serial), a.view(np.uint64) != b.view(np.uint64), ~(np.abs(a - b) <= 2 * bound))
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            o = int(offs[i])
            raise AssertionError(f"{problem}, replicas {rep}, launch '{la.name}': {int(bad.sum())} cells differ between the forms, first "
                                 f"{tc.cell_name(L, o)}: direct {float(a[i]).hex()} stacked {float(b[i]).hex()}, {int(k[i])} terms, bound "
                                 f"{'bit-exact' if k[i] <= 1 else float(2 * bound[i]).hex()}; fed by\n{tc.feeders(la, o)}")


def test_refusals(contexts):
    """Everything mcs_eval_tally refuses, with its message, and the context afterwards computes what it computed before."""
    case, launches, f32 = material("protons")
    hb = contexts("protons", 1)
    P = case.prob.params
    ng, ntc = P.n_grid, len(case.prob.tcuts)
    good = launches[-1]

    row = np.array([[[1e-15, 1e-15, 2e-15, 1.5, 0.1, 1.0, 2.0, 1.0]]])

    def refused(form, rec, word, msg):
        with pytest.raises(RuntimeError, match=msg):
            hb.eval_tally(form, rec, np.array(word, dtype=np.uint64).reshape(np.asarray(rec).shape[:2]))
    refused(3, row, [tc.pack(1, 0, 1, 0, 0, 1)], "unknown form")
    refused(-1, row, [tc.pack(1, 0, 1, 0, 0, 1)], "unknown form")
    refused(0, row, [int(tc.pack(1, 0, 1, 0, 0, 1)) | 4 << 40], "unknown kind")
    refused(0, row, [int(tc.pack(1, 0, 1, 0, 0, 1)) | 1 << 50], "stray bits")
    for word in (tc.pack(ng + 2, 0, 1, 0, 0, 1), tc.pack(1, ng + 2, 1, 0, 0, 1), tc.pack(1, 0, ng + 2, 0, 0, 1), tc.pack(0, 0, 255, 0, 1, 2)):
        refused(0, row, [word], "zone index outside")
    refused(0, row, [tc.pack(ng + 1, ng, 1, 0, 0, 1)], "outside zones 1 .. n_grid")        # downstream-going into zone n_grid + 1
    up = row.copy(); up[0, 0, 6], up[0, 0, 7] = 1.0, 2.0
    refused(1, up, [tc.pack(ng, ng + 1, 1, 0, 0, 1)], "outside zones 1 .. n_grid")         # upstream-going out of zone n_grid + 1
    for aux in (0, 5, 7):
        refused(1, row, [tc.pack(0, 0, 1, 0, aux, 2)], "i_reason outside")
    for aux in (0, ntc + 1, 255):
        refused(0, row, [tc.pack(0, 0, 0, 0, aux, 3)], "time cut outside")
    for j, v in ((2, np.nan), (5, np.inf), (6, -np.inf)):
        r = row.copy(); r[0, 0, j] = v
        refused(0, r, [tc.pack(1, 0, 1, 0, 0, 1)], "not finite")
    r = row.copy(); r[0, 0, 0] = 1.0 + 2.0 ** -30
    refused(2, r, [tc.pack(1, 0, 1, 0, 0, 1)], "no float")
    dp, up64 = ct.POINTER(ct.c_double), ct.POINTER(ct.c_uint64)
    w1 = np.array([tc.pack(1, 0, 1, 0, 0, 1)], dtype=np.uint64)
    assert hb.lib.mcs_eval_tally(hb.h, 0, 1, 1, None, w1.ctypes.data_as(up64)) != 0 and b"null argument" in hb.lib.mcs_last_error()
    assert hb.lib.mcs_eval_tally(hb.h, 0, 1, 1, row.ctypes.data_as(dp), None) != 0 and b"null argument" in hb.lib.mcs_last_error()
    assert hb.lib.mcs_eval_tally(hb.h, 0, -1, 1, row.ctypes.data_as(dp), w1.ctypes.data_as(up64)) != 0 and b"negative" in hb.lib.mcs_last_error()
    assert hb.lib.mcs_eval_tally(hb.h, 0, 1, -1, row.ctypes.data_as(dp), w1.ctypes.data_as(up64)) != 0 and b"negative" in hb.lib.mcs_last_error()
    assert hb.lib.mcs_eval_tally(None, 0, 1, 1, row.ctypes.data_as(dp), w1.ctypes.data_as(up64)) != 0 and b"null context" in hb.lib.mcs_last_error()
    assert hb.lib.mcs_eval_tally(hb.h, 0, 0, 0, None, None) == 0              # nothing to do is no error
    # a context that holds a population is refused: the launch constants are those of an empty one
    from conftest import hip_backend, start_species
    full = hip_backend(case.prob)
    start_species(full, case.prob)
    with pytest.raises(RuntimeError, match="holds a population"):
        full.eval_tally(0, good.rec, good.word)
    full.destroy()
    # ... and after all the refused calls the context tallies as before
    for form in FORMS:
        run_form(hb, case, [f32[-1] if form == 2 else good], form, f"after the refused calls, form {form}")


def test_regressions(contexts):
    for name, (problem, rows, words) in REGRESSIONS.items():
        case = material(problem)[0]
        hb = contexts(problem, 1)
        rec = np.array([[float.fromhex(v) for v in r] for r in rows]).reshape(1, -1, 8)
        word = np.array(words, dtype=np.uint64).reshape(1, -1)
        ob = oracle_backend(case.prob)
        la = tc.attach_logs(case, [tc.Launch(name, rec, word, np.arange(word.size).reshape(1, -1))], ob)[0]
        ob.destroy()
        for form in (0, 1):
            run_form(hb, case, [la], form, f"regression '{name}', form {form}")
