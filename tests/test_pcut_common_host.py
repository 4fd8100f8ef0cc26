"""The reference of tests/test_gpu_pcut_bookkeeping.py, checked without a GPU: the vectorised restatement of new_pcut
(tests/pcut_common.py) equals the serial loop bit for bit on every small case, the decide arithmetic equals Python integers and
exact rationals, and the oracle's new_pcut -- orc_new_pcut takes any flags and any saved population -- equals both."""
import ctypes as ct
from fractions import Fraction

import numpy as np
import pytest

from conftest import mcs, orc
import pcut_common as pc


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def small_cases():
    """(n, pattern, match, i_mult): every pattern at every small size, the multiplier and the matched byte cycling"""
    k = 0
    for n in (0,) + pc.SMALL_SIZES:
        for pat in pc.PATTERNS:
            # (the serial loop is Python: 64 copies up to 1025 particles, up to 3 above; 1000 copies only in the vectorised form)
            yield n, pat, (1, 5)[k % 2], pc.I_MULTS[k % 5] if n <= 1025 else pc.I_MULTS[k % 3]
            k += 1


def case_inputs(n, pat, match, seed):
    """n status bytes and three stale ones behind them that match (a walk that takes one index too many finds them), n + 3 states"""
    rng = np.random.default_rng(seed)
    ls = np.concatenate([pc.status_bytes(pc.pattern_mask(pat, n, rng), match, rng), np.full(3, match, dtype=np.uint8)])
    return ls, pc.make_saved(n + 3, seed)


def test_vectorised_split_equals_the_serial_loop():
    n_cases = 0
    for k, (n, pat, match, im) in enumerate(small_cases()):
        ls, pop = case_inputs(n, pat, match, k)
        f64, meta = pc.state_of(pop)
        s_src, s_f, s_m = pc.split_serial(ls, n, match, im, f64, meta)
        v_src, v_f, v_m = pc.split_vec(ls, n, match, im, f64, meta)
        what = f"n={n} {pat} match={match} i_mult={im}"
        assert np.array_equal(s_src, v_src) and v_src.dtype == np.int64, what
        assert s_f.shape == v_f.shape and np.array_equal(u64(s_f), u64(v_f)), what
        assert np.array_equal(s_m, v_m) and v_m.dtype == np.uint32, what
        n_cases += 1
    assert n_cases == 13 * len(pc.PATTERNS)


def test_patterns_are_what_their_names_say():
    rng = np.random.default_rng(0)
    n = 4097
    i = np.arange(n)
    assert pc.pattern_mask("lane63", n, rng).sum() == n // 64 and pc.pattern_mask("lane63", n, rng)[63]
    assert np.array_equal(np.flatnonzero(pc.pattern_mask("round2", n, rng))[:2], [512, 513])
    assert np.array_equal(np.flatnonzero(pc.pattern_mask("wave3", n, rng))[:2], [192, 193])
    assert np.flatnonzero(pc.pattern_mask("last", n, rng)).tolist() == [n - 1]
    for match in (1, 5):
        m = pc.pattern_mask("bernoulli0.5", n, rng)
        b = pc.status_bytes(m, match, rng)
        assert np.array_equal(b == match, m)
        assert set(np.unique(b[~m]).tolist()) == set(pc.BACKGROUND) | {6 - match}
    for nb in pc.CHUNK_BLOCKS:
        m = pc.chunk_mask(nb, rng)
        assert (len(m) + 1023) // 1024 == nb and len(m) % 1024 != 0
        if nb > 1024:
            assert m[1020 * 1024:1028 * 1024].all() and m[1024 * 1024:].sum() >= min(4096, len(m) - 1024 * 1024)
    assert i[pc.pattern_mask("alternating", n, rng)][0] == 1


def test_saved_states_are_distinct_in_every_field():
    pop = pc.make_saved(70000)
    f64, meta = pc.state_of(pop)
    for f in range(8):
        assert len(np.unique(u64(f64[f]))) == pop.n, pc.F64_FIELDS[f]
    assert np.array_equal(meta, np.arange(pop.n, dtype=np.uint32))
    w = pop.weight
    assert (np.abs(w[w != 0]) < 2.0 ** -1022).any() and (np.abs(w) > 1e299).any() and np.isfinite(w).all()
    # quotients by 3 and 7 that round up and that round down, against exact rationals
    for d in (3, 7):
        q = w[3:6000:6] / d
        exact = [Fraction(float(x)) / d for x in w[3:6000:6]]
        up = sum(Fraction(float(a)) > e for a, e in zip(q, exact))
        down = sum(Fraction(float(a)) < e for a, e in zip(q, exact))
        assert up > 100 and down > 100
        # ... and w * (1 / d) is NOT that quotient for some of them: the division cannot be replaced by a reciprocal
        assert (u64(w[3:6000:6] * (1.0 / d)) != u64(q)).any()


def test_decide_arithmetic():
    for ns in (0, 1, 2, 3, 7, 999, 1000, 4097, 10 ** 6):
        for k in (1, 2, 3, 64):
            for nt in {max(k * ns, 1), max(k * ns - 1, 1), max(ns - 1, 1), 1, k * ns + 1}:
                im, n_new = pc.decide(nt, ns)
                if ns == 0:
                    assert (im, n_new) == (1, 0)
                    continue
                assert im == max(int(Fraction(nt, ns).__floor__()), 1) and n_new == ns * im
                assert im >= 1 and (im == 1 or (im * ns <= nt < (im + 1) * ns))
                assert n_new <= max(nt, ns)          # every population of a species fits the largest of its targets
    assert pc.decide(3 * 1000 - 1, 1000) == (2, 2000) and pc.decide(999, 1000) == (1, 1000)


def test_oracle_new_pcut_equals_the_restatement():
    """orc_new_pcut walks l_save != 0: the flags given to it are the booleans `status == match`."""
    lib = orc.load("det", mcs.capi)
    n_cases = 0
    for k, (n, pat, match, im) in enumerate(small_cases()):
        if n == 0:
            continue
        ls, pop = case_inputs(n, pat, match, k)
        flags = np.ascontiguousarray(ls == match, dtype=np.uint8)
        f64, meta = pc.state_of(pop)
        src, r_f, r_m = pc.split_vec(ls, n, match, im, f64, meta)
        out = mcs.capi.Population(len(src) * im)
        ss, so = pop.soa(), out.soa()
        n_new = lib.orc_new_pcut(n, im, flags.ctypes.data_as(ct.POINTER(ct.c_uint8)), ct.byref(ss), ct.byref(so))
        assert n_new == out.n == r_f.shape[1]
        o_f, o_m = pc.state_of(out)
        assert np.array_equal(u64(o_f), u64(r_f)) and np.array_equal(o_m, r_m), f"n={n} {pat} i_mult={im}"
        n_cases += 1
    assert n_cases == 12 * len(pc.PATTERNS)


def test_bin_look_up_restatement():
    bs = np.array([0, 0, 0, 3, 4, 4, 9, 9], dtype=np.int64)
    j = np.arange(9)
    b = pc.bin_of(bs, j)
    assert b.tolist() == [2, 2, 2, 3, 5, 5, 5, 5, 5]
    assert all(bs[x] <= y < bs[x + 1] for x, y in zip(b, j))
