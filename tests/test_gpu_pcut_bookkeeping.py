"""The pcut bookkeeping kernels (K2 of csrc/mcs_population.hip) on crafted status bytes, on a real MI355X.

Only a transport launch can write l_save, so mcs_k_count_saved / mcs_k_scan_blocks / mcs_k_compact_index, their _dev twins,
mcs_k_pcut_decide, mcs_k_late_decide, mcs_k_split, mcs_k_split_dev and mcs_k_saved_export otherwise see only the patterns physics
produces.  mcs_eval_pcut_split (include/mcs.h) loads caller-given status bytes and saved states and runs the launchers of
mcs_run_pcut / mcs_new_pcut / mcs_saved_export (form 0), of one pcut of mcs_run_pcuts_fused (form 1) and of the late group of
mcs_run_pcuts_pipelined (form 2) with their own launch geometry.  The reference is the serial restatement of the reference code's
new_pcut / pcut_finalize in tests/pcut_common.py (tests/test_pcut_common_host.py ties its vectorised form to the serial loop and
to the oracle).  Every comparison is bit equality -- integers, the packed uint32 word, fp64 through .view(uint64) --, and every
word of the target outside the children's range must still hold the fill pattern.

The last test does the same for the binary search of mcs_k_init_pop over crafted bin tables."""
import ctypes as ct
import dataclasses
import functools

import numpy as np
import pytest

from conftest import mcs, make_problem, hip_backend, start_species, assert_pop_equal
import pcut_common as pc

pytestmark = pytest.mark.gpu

GUARD = 96
STALE = 70                   # status bytes and saved states beyond n in the host-sized and late forms, every byte the matched one
MAX_CHILDREN = 300_000       # of a small case: the multiplier of a case is the largest of I_MULTS, from its turn down, that keeps to it


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def hb():
    be = hip_backend(make_problem(64))
    yield be
    be.destroy()
    print("\npcut bookkeeping cases run:", CASES)          # (shown with -s: the figures a commit message can quote)


@functools.lru_cache(maxsize=4)
def saved(n):
    """n crafted saved states and their (f64, meta) form; computed once per size and never changed"""
    pop = pc.make_saved(n, seed=n % 1000 + 1)
    f64, meta = pc.state_of(pop)
    f64.setflags(write=False); meta.setflags(write=False)
    return pop, f64, meta


def with_stale(ls, match, extra=STALE):
    """the status bytes followed by `extra` stale ones, all equal to the matched byte"""
    return np.concatenate([ls, np.full(extra, match, dtype=np.uint8)])


def pick_mult(turn, n_saved):
    for im in pc.I_MULTS[turn % len(pc.I_MULTS)::-1]:
        if n_saved * im <= MAX_CHILDREN:
            return im
    return 1


def check_src(res, src, fill, what):
    got = res["src"]
    ns = len(src)
    assert res["scan_total"] == ns, f"{what}: scan total {res['scan_total']}, {ns} saved"
    bad = np.flatnonzero(got[:ns] != src)
    assert len(bad) == 0, f"{what}: src[] differs at {len(bad)} ranks, first {bad[:4]}: device {got[bad[:4]]}, reference {src[bad[:4]]}"
    assert (got[ns:] == fill).all(), f"{what}: src[] was written beyond the {ns} saved particles"


def check_target(res, off, ref_f, ref_m, what):
    """the children at [GUARD + off, GUARD + off + n_new) of the target, the fill pattern in every other word"""
    of, om = res["out_f64"], res["out_meta"]
    lo, hi = GUARD + off, GUARD + off + ref_f.shape[1]
    assert hi <= of.shape[1] - GUARD
    for f in range(8):
        bad = np.flatnonzero(u64(of[f, lo:hi]) != u64(ref_f[f]))
        assert len(bad) == 0, f"{what}: {pc.F64_FIELDS[f]} differs in {len(bad)} children, first {bad[:4]}: " \
                              f"device {[float(x).hex() for x in of[f, lo:hi][bad[:4]]]}, reference {[float(x).hex() for x in ref_f[f][bad[:4]]]}"
        assert (u64(of[f, :lo]) == pc.FILL_U64).all(), f"{what}: {pc.F64_FIELDS[f]} written below the children"
        assert (u64(of[f, hi:]) == pc.FILL_U64).all(), f"{what}: {pc.F64_FIELDS[f]} written beyond the children"
    bad = np.flatnonzero(om[lo:hi] != ref_m)
    assert len(bad) == 0, f"{what}: meta differs in {len(bad)} children, first {bad[:4]}"
    assert (om[:lo] == pc.FILL_U32).all() and (om[hi:] == pc.FILL_U32).all(), f"{what}: meta written outside the children"


def same_bytes(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8) if isinstance(a[k], np.ndarray) else a[k],
                              np.asarray(b[k]).view(np.uint8) if isinstance(b[k], np.ndarray) else b[k]) for k in a) and a.keys() == b.keys()


CASES = {"host": 0, "dev": 0, "late": 0, "export": 0, "max_nb": 0, "max_n_new": 0}


def count(form, nb, n_new):
    CASES[form] += 1
    CASES["max_nb"] = max(CASES["max_nb"], nb)
    CASES["max_n_new"] = max(CASES["max_n_new"], n_new)


# ---- form 0: mcs_k_count_saved, mcs_k_scan_blocks, mcs_k_compact_index, mcs_k_split --------------------------------------
def run_host(hb, ls, n, match, im, what, twice=False):
    cap_n = len(ls)
    pop, f64, meta = saved(cap_n)
    src, ref_f, ref_m = pc.split_vec(ls, n, match, im, f64, meta)
    fill = cap_n - 1 if cap_n else 0
    kw = dict(match=match, i_mult=im, src_fill=fill, guard=GUARD, out_cap=ref_f.shape[1] + 37)
    res = hb.eval_pcut_split(0, ls, pop, n, **kw)
    check_src(res, src, fill, what)
    check_target(res, 0, ref_f, ref_m, what)
    assert res["pd"] == [pc.PD_FILL] * 4 and res["pd_next"] == [pc.PD_FILL] * 4 and res["mismatch"] == 0, what
    if twice:
        assert same_bytes(res, hb.eval_pcut_split(0, ls, pop, n, **kw)), f"{what}: a second run gave other bytes"
    count("host", (n + 1023) // 1024, ref_f.shape[1])
    return res


@pytest.mark.parametrize("n", (0,) + pc.SMALL_SIZES)
def test_host_form_every_pattern(hb, n):
    """Every pattern at size n, the matched byte alternating between 1 and 5 (the other one is part of the background), the
    multiplier taking its turn; behind the n status bytes lie STALE stale ones that all match, and src[] starts out stale."""
    for k, pat in enumerate(pc.PATTERNS):
        turn = k + pc.SMALL_SIZES.index(n) + 1 if n else k
        rng = np.random.default_rng(1000 * n + k)
        match = (1, 5)[turn % 2]
        mask = pc.pattern_mask(pat, n, rng)
        ls = with_stale(pc.status_bytes(mask, match, rng), match)
        im = pick_mult(turn, int(mask.sum()))
        run_host(hb, ls, n, match, im, f"host form, n={n}, {pat}, match={match}, i_mult={im}", twice=pat == "bernoulli0.5")


def test_host_form_every_multiplier_and_both_bytes(hb):
    """1 and 5 in ONE array: a count of one must ignore the other; every multiplier, on weights whose quotients round either way."""
    n = 1025
    rng = np.random.default_rng(7)
    draw = rng.random(n)
    ls = pc.status_bytes(np.zeros(n, dtype=bool), 1, rng)
    ls[ls == 5] = 0
    ls[draw < 0.3] = 1
    ls[draw > 0.75] = 5
    assert (ls == 1).sum() > 200 and (ls == 5).sum() > 200
    for match in (1, 5):
        for im in pc.I_MULTS:
            run_host(hb, with_stale(ls, match), n, match, im, f"host form, 1 and 5 mixed, match={match}, i_mult={im}")


@pytest.mark.parametrize("nb", pc.CHUNK_BLOCKS)
def test_chunk_carry_of_the_block_scan(hb, nb):
    """nb blocks of status bytes around the 1024 blocks one pass of mcs_k_scan_blocks takes: sparse saves, full blocks across the
    boundary, in all three forms; then nobody saved, and only the last particle."""
    rng = np.random.default_rng(nb)
    mask = pc.chunk_mask(nb, rng)
    n = len(mask)
    assert (n + 1023) // 1024 == nb
    pop, f64, meta = saved(n)
    ls = pc.status_bytes(mask, 1, rng)
    run_host(hb, ls, n, 1, 2, f"host form, {nb} blocks")
    # device-sized: the same bytes, the population size on the device
    ns = int(mask.sum())
    src, ref_f, ref_m = pc.split_vec(ls, n, 1, 3, f64, meta)
    res = hb.eval_pcut_split(1, ls, pop, n, n_target=3 * ns + 2, ctr_saved=ns, ctr_work=n, src_fill=n - 1, guard=GUARD, out_cap=3 * ns + 5)
    check_src(res, src, n - 1, f"device form, {nb} blocks")
    check_target(res, 0, ref_f, ref_m, f"device form, {nb} blocks")
    assert res["pd"] == [n, ns, 3, 3 * ns] and res["pd_next"] == [3 * ns] + [pc.PD_FILL] * 3 and res["mismatch"] == 0
    count("dev", nb, 3 * ns)
    # late: status 5
    ls5 = pc.status_bytes(mask, 5, rng)
    src, ref_f, ref_m = pc.split_vec(ls5, n, 5, 2, f64, meta)
    res = hb.eval_pcut_split(2, ls5, pop, n, i_mult=2, n_main_next=257, src_fill=n - 1, guard=GUARD, out_cap=257 + 2 * ns + 5)
    check_src(res, src, n - 1, f"late form, {nb} blocks")
    check_target(res, pc.late_offset(257), ref_f, ref_m, f"late form, {nb} blocks")
    assert res["pd"] == [257 + 2 * ns, ns, 2, 2 * ns]
    count("late", nb, 2 * ns)
    for pat in ("none", "last"):
        ls = pc.status_bytes(pc.pattern_mask(pat, n, rng), 1, rng)
        run_host(hb, ls, n, 1, 7, f"host form, {nb} blocks, {pat}")


# ---- form 1: the _dev twins, mcs_k_pcut_decide, mcs_k_split_dev -----------------------------------------------------------
def run_dev(hb, ls, n_use, n_target, ctr_saved, what, twice=False):
    cap_n = len(ls)
    pop, f64, meta = saved(cap_n)
    ns = int((ls[:n_use] == 1).sum())
    im, n_new = pc.decide(n_target, ns)
    src, ref_f, ref_m = pc.split_vec(ls, n_use, 1, im, f64, meta)
    assert ref_f.shape[1] == n_new and len(src) == ns
    fill = cap_n - 1
    kw = dict(n_target=n_target, ctr_work=0x1234567, ctr_saved=ctr_saved, src_fill=fill, guard=GUARD, out_cap=n_new + 41)
    res = hb.eval_pcut_split(1, ls, pop, n_use, **kw)
    check_src(res, src, fill, what)
    check_target(res, 0, ref_f, ref_m, what)
    assert res["pd"] == [n_use, ns, im, n_new], f"{what}: pd {res['pd']}"
    assert res["pd_next"] == [n_new] + [pc.PD_FILL] * 3, f"{what}: pd_next {res['pd_next']}"
    assert res["ctr_work"] == 0 and res["ctr_saved"] == 0, f"{what}: the next launch's counters were not cleared"
    assert res["mismatch"] == (0 if ctr_saved == ns else 1), f"{what}: mismatch word {res['mismatch']} for counter {ctr_saved}, {ns} saved"
    if twice:
        assert same_bytes(res, hb.eval_pcut_split(1, ls, pop, n_use, **kw)), f"{what}: a second run gave other bytes"
    count("dev", (cap_n + 1023) // 1024, n_new)


@pytest.mark.parametrize("n_use", (1, 1000, 1024, 1025, 5000))
def test_device_form_sizes_targets_and_counter(hb, n_use):
    """n_use under every capacity that holds it; everything beyond n_use is stale: status bytes of 1 (a few 5s) and src[] words.
    Targets at 3 n_saved, one below it, n_saved - 1 and 1; the kernel's counter word right, one above, one below."""
    turn = 0
    for cap_n in sorted({n_use, max(4096, n_use), 70000}):          # (a capacity holds its population)
        for pat in pc.PATTERNS:
            rng = np.random.default_rng(n_use * 31 + cap_n + turn)
            mask = pc.pattern_mask(pat, n_use, rng)
            ns = int(mask.sum())
            stale = np.where(rng.random(cap_n - n_use) < 0.9, 1, 5).astype(np.uint8)
            ls = np.concatenate([pc.status_bytes(mask, 1, rng), stale])
            targets = sorted({max(3 * ns, 1), max(3 * ns - 1, 1), max(ns - 1, 1), 1})
            for n_target in targets:
                ctr = (ns, ns + 1, max(ns - 1, 0) if ns else 1)[turn % 3]
                run_dev(hb, ls, n_use, n_target, ctr, f"device form, n_use={n_use}, cap_n={cap_n}, {pat}, n_target={n_target}, counter={ctr}",
                        twice=turn % 11 == 0)
                turn += 1


def test_device_form_stride_loop(hb):
    """n_new above n_cu * 16 * 256 from five parents: mcs_k_split_dev takes a second trip through its grid-stride loop, which must
    stop at n_new.  The capacity is the target, as in mcs_run_pcuts_fused."""
    n_cu = hb.num_cus()
    n_target = n_cu * 16 * 256 + 4097
    n_use, cap_n = 5000, n_target
    ls = np.full(cap_n, 1, dtype=np.uint8)
    ls[:n_use] = 0
    ls[[0, 63, 1023, 1024, n_use - 1]] = 1
    im, n_new = pc.decide(n_target, 5)
    assert n_new > n_cu * 16 * 256 and im * 5 == n_new
    run_dev(hb, ls, n_use, n_target, 5, f"device form, stride loop, n_new={n_new}")


# ---- form 2: mcs_launch_late_split (match 5, mcs_k_late_decide, mcs_k_split_dev behind the main group) ---------------------
def run_late(hb, ls, n, im, n_main_next, what, twice=False):
    cap_n = len(ls)
    pop, f64, meta = saved(cap_n)
    src, ref_f, ref_m = pc.split_vec(ls, n, 5, im, f64, meta)
    ns, n_new = len(src), ref_f.shape[1]
    fill = cap_n - 1
    kw = dict(i_mult=im, n_main_next=n_main_next, src_fill=fill, guard=GUARD, out_cap=n_main_next + n_new + 29)
    res = hb.eval_pcut_split(2, ls, pop, n, **kw)
    check_src(res, src, fill, what)
    check_target(res, pc.late_offset(n_main_next), ref_f, ref_m, what)
    assert res["pd"] == [n_main_next + n_new, ns, im, n_new], f"{what}: pd {res['pd']}"
    assert res["pd_next"] == [pc.PD_FILL] * 4 and res["mismatch"] == 0 and res["ctr_work"] == 0 and res["ctr_saved"] == 0, what
    if twice:
        assert same_bytes(res, hb.eval_pcut_split(2, ls, pop, n, **kw)), f"{what}: a second run gave other bytes"
    count("late", (n + 1023) // 1024, n_new)


@pytest.mark.parametrize("n_main_next", (0, 1, 257, 5000))
def test_late_form(hb, n_main_next):
    """Status 5 among 1s (1 is part of the background here), the children behind n_main_next others: the words below them and
    beyond their end keep the fill pattern, and the next population's size is n_main_next + n_saved * i_mult."""
    turn = 0
    for n in (1, 64, 257, 1025, 4097):
        for pat in pc.PATTERNS:
            rng = np.random.default_rng(n * 17 + n_main_next + turn)
            mask = pc.pattern_mask(pat, n, rng)
            ls = with_stale(pc.status_bytes(mask, 5, rng), 5)
            im = pick_mult(turn, int(mask.sum()))
            run_late(hb, ls, n, im, n_main_next, f"late form, n={n}, {pat}, i_mult={im}, n_main_next={n_main_next}", twice=turn % 7 == 0)
            turn += 1


def test_late_form_stride_loop(hb):
    """n_new above n_cu * 4 * 256 from three parents: the late group's split takes a second trip through its grid-stride loop."""
    n_cu = hb.num_cus()
    im = (n_cu * 4 * 256) // 3 + 1000
    n = 4097
    ls = with_stale(np.full(n, 1, dtype=np.uint8), 5)
    ls[[64, 2048, n - 1]] = 5
    assert 3 * im > n_cu * 4 * 256
    run_late(hb, ls, n, im, 257, f"late form, stride loop, n_new={3 * im}")


# ---- mcs_k_saved_export --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 257, 1025, 4097))
def test_saved_export(hb, n):
    """gidx = first + src * stride and the index-list form, with the states and without; entries [n_saved, cap) untouched."""
    pop, f64, meta = saved(n + STALE)
    for k, pat in enumerate(("bernoulli0.5", "all", "none", "last", "lane63")):
        rng = np.random.default_rng(n + k)
        mask = pc.pattern_mask(pat, n, rng)
        ls = with_stale(pc.status_bytes(mask, 1, rng), 1)
        src = pc.saved_indices(ls, n, 1)
        ns = len(src)
        gin = rng.permutation(n).astype(np.int64) * 5 + 11
        for mode in (1, 2):
            for how in (dict(exp_first=5, exp_stride=3), dict(exp_first=0, exp_stride=1), dict(exp_gin=gin)):
                what = f"export, n={n}, {pat}, mode {mode}, {sorted(how)}"
                cap = ns + 13
                res = hb.eval_pcut_split(0, ls, pop, n, match=1, i_mult=1, src_fill=0, guard=GUARD, out_cap=ns, export_mode=mode,
                                         exp_cap=cap, **how)
                check_src(res, src, 0, what)
                ref = pc.export_gidx(src, how.get("exp_first", 0), how.get("exp_stride", 1), how.get("exp_gin"))
                assert np.array_equal(res["exp_gidx"][:ns], ref) and (res["exp_gidx"][ns:] == pc.FILL_I64).all(), what
                ef, em = res["exp_f64"], res["exp_meta"]
                assert ef.shape == (8, cap)
                if mode == 2:
                    assert np.array_equal(u64(ef[:, :ns]), u64(f64[:, src])) and np.array_equal(em[:ns], meta[src]), what
                    assert (u64(ef[:, ns:]) == pc.FILL_U64).all() and (em[ns:] == pc.FILL_U32).all(), what
                else:
                    assert (u64(ef) == pc.FILL_U64).all() and (em == pc.FILL_U32).all(), f"{what}: the states-off call wrote states"
                count("export", (n + 1023) // 1024, ns)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(hb):
    n = 300
    pop, f64, meta = saved(n)
    rng = np.random.default_rng(3)
    ls = pc.status_bytes(pc.pattern_mask("bernoulli0.5", n, rng), 1, rng)
    ns = int((ls == 1).sum())
    cur = mcs.capi.Population(5)
    for f in pc.F64_FIELDS:
        getattr(cur, f)[:] = np.arange(1, 6)
    cur.tcut[:] = 1
    hb.set_population(cur)
    good = dict(match=1, i_mult=2, src_fill=3, guard=GUARD, out_cap=2 * ns + 3)
    res0 = hb.eval_pcut_split(0, ls, pop, n, **good)
    bad_grid = pc.make_saved(n); bad_grid.grid[17] = 70000
    p32 = make_problem(64); p32.params.state_fp32 = 1
    h32 = hip_backend(p32)
    refusals = [
        (hb, 3, ls, pop, n, dict(good)), (hb, -1, ls, pop, n, dict(good)),                        # unknown form
        (hb, 0, ls, pop, n + 1, dict(good)), (hb, 0, ls, pop, -1, dict(good)),                    # n > cap_n, n < 0
        (hb, 0, ls, pop, n, dict(good, i_mult=0)), (hb, 2, ls, pop, n, dict(good, i_mult=-3)),    # i_mult < 1
        (hb, 1, ls, pop, n, dict(good, n_target=0)),
        (hb, 0, ls, pop, n, dict(good, match=2)),
        (hb, 0, ls, pop, n, dict(good, src_fill=n)), (hb, 0, ls, pop, n, dict(good, src_fill=-1)),
        (hb, 0, ls, pop, n, dict(good, out_cap=2 * ns - 1)),                                      # the children do not fit
        (hb, 2, ls, pop, n, dict(good, n_main_next=-1)),
        (hb, 0, ls, pop, n, dict(good, guard=-1)),
        (hb, 0, ls, pop, n, dict(good, export_mode=3, exp_cap=n)), (hb, 0, ls, pop, n, dict(good, export_mode=2, exp_cap=ns - 1)),
        (hb, 1, ls, pop, n, dict(good, n_target=5, export_mode=1, exp_cap=n)),
        (hb, 0, ls, bad_grid, n, dict(good)),
        (h32, 2, ls, pop, n, dict(good)),                                                         # the late form, fp32 state
    ]
    for be, form, l, p, nn, kw in refusals:
        with pytest.raises(RuntimeError, match="mcs_eval_pcut_split"):
            be.eval_pcut_split(form, l, p, nn, **kw)
    # null buffers and a null struct, through the library itself; the caller's output words stay as they were
    s = pop.soa()
    io = mcs.capi.McsPcutEval()
    io.form, io.match, io.n, io.cap_n, io.i_mult, io.guard, io.out_cap = 0, 1, n, n, 1, 4, n
    io.scan_total, io.mismatch = 0xDEAD, 0xBEEF
    io.saved = ct.pointer(s)
    assert hb.lib.mcs_eval_pcut_split(hb.h, ct.byref(io)) != 0 and b"null buffer" in hb.lib.mcs_last_error()
    assert hb.lib.mcs_eval_pcut_split(hb.h, None) != 0 and b"null argument" in hb.lib.mcs_last_error()
    assert hb.lib.mcs_eval_pcut_split(None, ct.byref(io)) != 0 and b"null context" in hb.lib.mcs_last_error()
    assert io.scan_total == 0xDEAD and io.mismatch == 0xBEEF and list(io.pd) == [0] * 4
    # the fp32-state context takes the forms that apply to it, and both contexts are as they were
    res32 = h32.eval_pcut_split(0, ls, pop, n, **good)
    assert same_bytes(res0, res32)
    h32.destroy()
    assert_pop_equal(cur, hb.get_population(), "the population after the refused calls")
    assert same_bytes(res0, hb.eval_pcut_split(0, ls, pop, n, **good)), "the same call after the refused ones gave other bytes"


# ---- the binned look-up of mcs_k_init_pop ---------------------------------------------------------------------------------
def bin_tables():
    """name -> bin_count: one bin; 4096 bins with runs of empty ones at the start, in the middle and at the end, mostly of one
    particle; a handful of wide bins between empty ones"""
    rng = np.random.default_rng(11)
    many = np.ones(4096, dtype=np.int64)
    many[:37] = 0; many[1000:1100] = 0; many[2047:2050] = 0; many[-50:] = 0
    many[rng.integers(40, 4000, 60)] = rng.integers(2, 9, 60)
    many[1000:1100] = 0; many[2047:2050] = 0
    few = np.array([0, 0, 5, 0, 1, 1, 0, 0, 0, 300, 1, 0, 64, 0], dtype=np.int64)
    return {"one bin": np.array([778], dtype=np.int64), "4096 bins": many, "wide bins between empty ones": few}


@pytest.mark.parametrize("name", list(bin_tables()))
def test_init_pop_binned_look_up(name):
    cnt = bin_tables()[name]
    prob = make_problem(64)
    be = hip_backend(prob)
    start_species(be, prob)
    base = mcs.inputs.init_pop_host(prob, 1)
    nbins = len(cnt)
    n_total = int(cnt.sum())
    b = np.arange(nbins, dtype=np.float64)
    bp = base.bin_ptot[0] * (1.0 + (b + 1.0) * 2.0 ** -20)
    bw = 1.0 + b
    bp[cnt == 0] = np.nan; bw[cnt == 0] = np.nan          # an empty bin is never anybody's: its entries must not be read
    inj = dataclasses.replace(base, n_pts_use=n_total, bin_ptot=bp, bin_weight=bw, bin_count=cnt)
    bs = inj.bin_start
    j_all = np.arange(n_total)
    own = pc.bin_of(bs, j_all)
    assert ((bs[own] <= j_all) & (j_all < bs[own + 1])).all() and (cnt[own] > 0).all()
    be.init_pop(inj, 0, n_total, n_total)
    full = be.get_population()
    assert np.array_equal(u64(full.ptot_pf), u64(bp[own])) and np.array_equal(u64(full.weight), u64(bw[own])), name
    be.init_pop_arrays(inj, 0, n_total, n_total)
    assert_pop_equal(full, be.get_population(), f"{name}: binned against per-particle arrays")
    # strided shards whose first and last particle sit on bin boundaries (the first or the last particle of a bin)
    first_of, last_of = set(bs[:-1][cnt > 0].tolist()), set((bs[1:][cnt > 0] - 1).tolist())
    n_shards = 0
    starts = sorted(first_of)[:3] + sorted(last_of - first_of)[:2]
    for stride in (3, 7):
        for j0 in starts:
            n_loc = (n_total - 1 - j0) // stride + 1
            while n_loc > 1 and (j0 + (n_loc - 1) * stride) not in (first_of | last_of):
                n_loc -= 1
            j = j0 + np.arange(n_loc) * stride
            assert j[-1] < n_total and int(j[0]) in (first_of | last_of) and int(j[-1]) in (first_of | last_of)
            be.init_pop(inj, int(j0), n_loc, n_total, j_stride=stride)
            assert_pop_equal(full.take(j), be.get_population(), f"{name}: shard {j0}+k*{stride}, {n_loc} particles")
            n_shards += 1
    assert n_shards == 2 * len(starts) and (nbins == 1 or len(starts) == 5)
    be.destroy()
