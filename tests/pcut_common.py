"""A plain restatement of the reference's pcut bookkeeping (pcut_finalize / new_pcut, src/cuts.jl:34-124) and the crafted cases
of tests/test_gpu_pcut_bookkeeping.py and tests/test_pcut_common_host.py.

The reference walks the saved flags in index order and writes i_mult copies of every saved particle, each with weight
w / i_mult, where i_mult = max(n_target ÷ n_saved, 1).  `split_serial` is that loop, one particle at a time, in Python integers
and floats; `split_vec` is the numpy form (flatnonzero, repeat) the large cases use.  tests/test_pcut_common_host.py proves the
two equal bit for bit on every small case and checks them against the oracle's new_pcut.

A particle state here is the pair (f64 [8][n], meta [n]): the eight fp64 fields in the order of capi.F64_FIELDS and the packed
word grid | tcut << 16 | downstream << 24 | inj << 25 the device keeps (mcs_pack_meta)."""
import numpy as np

from conftest import mcs

F64_FIELDS = mcs.capi.F64_FIELDS
BLOCK, ROUND, WAVE = 1024, 256, 64          # status bytes per block, per round of a block, per wave of a round (K2a / K2c)
CHUNK = 1024                                # blocks per pass of the block scan (K2b)
FILL_BYTE = 0xA5                            # every byte of the target and the export buffers before a call
FILL_U32, FILL_U64 = np.uint32(0xA5A5A5A5), np.uint64(0xA5A5A5A5A5A5A5A5)
FILL_I64 = np.array([FILL_U64]).view(np.int64)[0]
PD_FILL = -7                                # every PcutDev word before a call
BACKGROUND = (0, 2, 3, 4, 255)              # status bytes that never count, beside the non-matching one of {1, 5}

SMALL_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097)
I_MULTS = (1, 2, 3, 7, 64, 1000)
PATTERNS = ("none", "all", "first", "last", "lane63", "lane0", "alternating", "round0", "round1", "round2", "round3",
            "wave0", "wave1", "wave2", "wave3", "bernoulli0.001", "bernoulli0.5", "bernoulli0.999")
CHUNK_BLOCKS = (1023, 1024, 1025, 2049)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def decide(n_target, n_saved):
    """(i_mult, n_new) of pcut_finalize in Python integers: i_mult = max(n_target ÷ n_saved, 1) (src/cuts.jl:42); nobody saved: 1."""
    n_target, n_saved = int(n_target), int(n_saved)
    i_mult = max(n_target // n_saved, 1) if n_saved > 0 else 1
    return i_mult, n_saved * i_mult


def saved_indices_serial(l_save, n, match):
    src = []
    for j in range(int(n)):
        if int(l_save[j]) == int(match):
            src.append(j)
    return np.array(src, dtype=np.int64)


def saved_indices(l_save, n, match):
    """src[]: the indices below n whose status byte equals `match`, in index order."""
    return np.flatnonzero(np.asarray(l_save[:int(n)]) == match).astype(np.int64)


def split_serial(l_save, n, match, i_mult, f64, meta):
    """new_pcut one particle at a time -> (src, child f64 [8][n_new], child meta [n_new])."""
    src = saved_indices_serial(l_save, n, match)
    n_new = len(src) * int(i_mult)
    out_f, out_m = np.zeros((8, n_new)), np.zeros(n_new, dtype=np.uint32)
    o = 0
    for j in src:
        for _ in range(int(i_mult)):
            out_f[0, o] = float(f64[0, j]) / float(i_mult)          # (Python's float division is IEEE's: correctly rounded)
            for f in range(1, 8):
                out_f[f, o] = f64[f, j]
            out_m[o] = meta[j]
            o += 1
    return src, out_f, out_m


def split_vec(l_save, n, match, i_mult, f64, meta):
    src = saved_indices(l_save, n, match)
    parent = np.repeat(src, int(i_mult))
    out_f = np.ascontiguousarray(f64[:, parent])
    out_f[0] = out_f[0] / np.float64(i_mult)
    return src, out_f, np.ascontiguousarray(meta[parent])


def late_offset(n_main_next):
    """where the late group's first child goes: behind the main group's n_main_next children"""
    return int(n_main_next)


def export_gidx(src, first, stride, gin=None):
    src = np.asarray(src, dtype=np.int64)
    return np.asarray(gin, dtype=np.int64)[src] if gin is not None else np.int64(first) + src * np.int64(stride)


def bin_of(bin_start, j):
    """the bin b with bin_start[b] <= j < bin_start[b + 1] (the look-up of mcs_k_init_pop)"""
    return np.searchsorted(np.asarray(bin_start, dtype=np.int64), np.asarray(j, dtype=np.int64), "right") - 1


# ---- the crafted cases ----------------------------------------------------------------------------------------------------
def pack_meta(pop):
    return (pop.grid.astype(np.uint32) & np.uint32(0xffff)) | ((pop.tcut.astype(np.uint32) & np.uint32(0xff)) << np.uint32(16)) | \
           ((pop.downstream.astype(np.uint32) & np.uint32(1)) << np.uint32(24)) | ((pop.inj.astype(np.uint32) & np.uint32(1)) << np.uint32(25))


def state_of(pop):
    return np.ascontiguousarray(np.stack([getattr(pop, f) for f in F64_FIELDS])), pack_meta(pop)


def make_saved(n, seed=1):
    """n saved states, distinct per index in every field (n <= 2^26: the packed word is the index), so a wrong parent shows in
    all nine arrays.  Weights by index mod 6: subnormals, around 1e-300, around 1e300, a full random mantissa (whose quotients by
    3, 7 and 1000 round either way), and both signs of it."""
    assert n <= 1 << 26
    rng = np.random.default_rng(seed)
    k = np.arange(n, dtype=np.int64)
    kf = k.astype(np.float64)
    pop = mcs.capi.Population(n)
    wide = (1.0 + rng.random(n)) * (1.0 + kf * 2.0 ** -27)
    cls = k % 6
    w = np.where(cls == 0, (kf + 1.0) * 5e-324, wide)
    w = np.where(cls == 1, 1e-300 * (1.0 + kf * 2.0 ** -27), w)
    w = np.where(cls == 2, 1e300 * (1.0 + kf * 2.0 ** -27), w)
    w = np.where(cls == 4, -wide, w)
    w = np.where(cls == 5, wide * 2.0 ** -1030, w)          # quotients that end subnormal
    pop.weight[:] = w
    pop.ptot_pf[:] = 1e-17 * (1.0 + kf * 2.0 ** -27)
    pop.pb_pf[:] = -2e-17 * (1.0 + kf * 2.0 ** -27)
    pop.x_PT_cm[:] = 3e10 + kf
    pop.xn_per[:] = 4.0 + kf
    pop.prp_x_cm[:] = -5e12 - kf * 8.0
    pop.acctime_sec[:] = 6.0 + kf * 0.5
    pop.phi_rad[:] = 7.0 * 2.0 ** -20 * (kf + 1.0)
    pop.grid[:] = k & 0xffff
    pop.tcut[:] = (k >> 16) & 0xff
    pop.downstream[:] = (k >> 24) & 1
    pop.inj[:] = (k >> 25) & 1
    return pop


def pattern_mask(name, n, rng):
    """which of n indices are saved"""
    i = np.arange(n, dtype=np.int64)
    rnd, wave, lane = (i % BLOCK) // ROUND, (i % ROUND) // WAVE, i % WAVE
    if name == "none": return np.zeros(n, dtype=bool)
    if name == "all": return np.ones(n, dtype=bool)
    if name == "first": return i == 0
    if name == "last": return i == n - 1
    if name == "lane63": return lane == 63
    if name == "lane0": return lane == 0
    if name == "alternating": return i % 2 == 1
    if name.startswith("round"): return rnd == int(name[5:])
    if name.startswith("wave"): return wave == int(name[4:])
    if name.startswith("bernoulli"): return rng.random(n) < float(name[9:])
    raise KeyError(name)


def status_bytes(mask, match, rng):
    """`match` where the mask is set; elsewhere a draw from BACKGROUND and the non-matching one of {1, 5}"""
    other = 5 if match == 1 else 1
    pool = np.array(BACKGROUND + (other,), dtype=np.uint8)
    b = pool[rng.integers(0, len(pool), len(mask))]
    b[np.asarray(mask, dtype=bool)] = match
    return np.ascontiguousarray(b, dtype=np.uint8)


def chunk_mask(nb, rng, p=0.0005):
    """nb blocks of status bytes (the last one partial): sparse saves and eight full blocks laid across the boundary of the
    scan's first chunk (those of blocks 1020..1027 that exist), so the carry into the second chunk is large and exact"""
    n = (nb - 1) * BLOCK + 517
    m = rng.random(n) < p
    for b in range(CHUNK - 4, CHUNK + 4):
        if b < nb:
            m[b * BLOCK:min((b + 1) * BLOCK, n)] = True
    m[n - 1] = True
    return m
