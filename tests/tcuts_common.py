"""The time-cut spectra (include/mcs.h, mcs_tcut_spectra) restated in plain Python floats from the header's text, the crafted rows
of tests/test_tcut_spectra_host.py and tests/test_gpu_tcut_spectra.py, and the helper that puts them on a context.  Nothing here
imports the package's consumers module or shares code with csrc/mcs_consumers.hip; the library's log10 is used where the header names
it, for log10(tcuts[k]) of the index, and nowhere else.

  g[l] = now[l] - base[l];  number = ((0.0 + g[0]) + g[1]) + ... + g[nmom]
  weight = weight_coupled, or 1e-99 below 1e-60
  live: number > 1e-99.  live: spectrum[l] = g[l] / number, or 1e-99 below 1e-60; dead: spectrum 1e-99, number 0.0, the rest NaN
  mean_log_p = (sum g[l] * (0.5 * (e[l] + e[l+1]))) / number
  quantile: T = q * number; C_0 = 0.0, C_{l+1} = C_l + g[l]; l* the first l with g[l] > 0 and C_{l+1} >= T;
            f = (T - C_{l*}) / g[l*]; e[l*] + f * (e[l*+1] - e[l*]); the last lit bin with f = 1.0 if none is found
  index[j]: the slope rule of the products sample over the live rows, x = log10(tcuts[k]), y = quantile[j][k]"""
import math

import numpy as np

from conftest import mcs

Q = (0.5, 0.9, 0.99)
NA_C, PM = 100, 201                      # MCS_NA_C, MCS_PSD_MAX + 1: the rows and the row stride of a species' block of spectra_coupled
FLOOR, T60 = 1.0e-99, 1.0e-60
NAN = float("nan")


def up(x):
    return float(np.nextafter(x, math.inf))


def down(x):
    return float(np.nextafter(x, -math.inf))


class Reference:
    """The outputs of the call as numpy arrays, and the result as one vector in mcs_tcut_layout."""

    def __init__(self, spectrum, weight, number, mean_log_p, quantile, index, diag):
        self.spectrum, self.weight, self.number, self.mean_log_p = (np.array(a, dtype=np.float64) for a in (spectrum, weight, number, mean_log_p))
        self.quantile, self.index = np.array(quantile, dtype=np.float64), np.array(index, dtype=np.float64)
        self.diag = np.array(diag, dtype=np.int64)

    def words(self):
        return np.concatenate([a.ravel() for a in (self.spectrum, self.weight, self.number, self.mean_log_p, self.quantile, self.index)])


def quantile_of(g, e, nm, T):
    C, last = 0.0, -1
    for l in range(nm + 1):
        Cn = C + g[l]
        if g[l] > 0:
            if Cn >= T:
                f = (T - C) / g[l]
                return e[l] + f * (e[l + 1] - e[l]), False
            last = l
        C = Cn
    if last < 0:
        return NAN, True
    return e[last] + 1.0 * (e[last + 1] - e[last]), True


def slope_rule(x, y, valid):
    """include/mcs.h, "Slope of frame m", on Python floats."""
    idx = [k for k in range(len(x)) if valid[k]]
    if len(idx) < 3:
        return NAN
    n = float(len(idx))
    sx = sy = 0.0
    for k in idx:
        sx = sx + x[k]
        sy = sy + y[k]
    xbar, ybar = sx / n, sy / n
    sxx = sxy = 0.0
    for k in idx:
        dx = x[k] - xbar
        sxx = sxx + dx * dx
        sxy = sxy + dx * (y[k] - ybar)
    return sxy / sxx if sxx != 0.0 else (NAN if sxy == 0.0 else math.copysign(math.inf, sxy))


def reference(now, base, weight, mom_log, tcuts, nm, log10):
    """now, base: [nt][>= nm+1]; weight [nt]; mom_log [nm+2]; log10: the library's, arrays -> arrays."""
    nt, NM = len(tcuts), nm + 2
    e = [float(v) for v in mom_log[:NM]]
    spectrum, w_out, number, mean, quant = [], [], [], [], [[], [], []]
    n_neg = n_live = 0
    short = []
    for k in range(nt):
        g = []
        for l in range(nm + 1):
            n_, b_ = float(now[k][l]), float(base[k][l])
            n_neg += n_ < b_
            g.append(n_ - b_)
        num = 0.0
        for l in range(nm + 1):
            num = num + g[l]
        w = float(weight[k])
        w_out.append(FLOOR if w < T60 else w)
        if not num > FLOOR:
            spectrum.append([FLOOR] * NM); number.append(0.0); mean.append(NAN)
            for j in range(3):
                quant[j].append(NAN)
            continue
        n_live += 1
        row = []
        for l in range(nm + 1):
            s = g[l] / num
            row.append(FLOOR if s < T60 else s)
        spectrum.append(row + [FLOOR])
        number.append(num)
        s = 0.0
        for l in range(nm + 1):
            c = 0.5 * (e[l] + e[l + 1])
            s = s + g[l] * c
        mean.append(s / num)
        for j, q in enumerate(Q):
            v, was_short = quantile_of(g, e, nm, q * num)
            quant[j].append(v)
            short.append(was_short)
    x = [float(v) for v in log10(np.ascontiguousarray(tcuts, dtype=np.float64))]
    live = [n > FLOOR for n in number]
    index = [slope_rule(x, quant[j], live) for j in range(3)]
    ref = Reference(spectrum, w_out, number, mean, quant, index, [n_live, n_neg])
    ref.f_is_one = any(short)
    return ref


# ---- crafted rows: (base [nm+1], now [nm+1], weight) ------------------------------------------------------------------------------
def _row(nm, lit, base=0.0, weight=1.0):
    """A row whose bins `lit` (l -> deposit) grew by their deposit over a flat base."""
    b = np.full(nm + 1, float(base))
    n = b.copy()
    for l, w in lit.items():
        n[l] = n[l] + w
    return b, n, float(weight)


def tie_rows(nm, l0, l1):
    """For each q two lit bins l0 < l1 with g[l0] == q * number exactly: the >= of the quantile rule decides."""
    rows = []
    for q in Q:
        g0 = q * 1.0
        g1 = 1.0 - g0
        assert g0 + g1 == 1.0 and q * (g0 + g1) == g0
        rows.append(_row(nm, {l0: g0, l1: g1}))
    return rows


def crafted_rows(nm, seed=0):
    """name -> row.  Every single-row case; the multi-row ones (live and dead rows) are SCENARIOS."""
    rng = np.random.default_rng(seed)
    mid = nm // 2
    rows = {
        "one_bin_first": _row(nm, {0: 0.75}),
        "one_bin_last": _row(nm, {nm: 3.0e-7}, weight=up(T60)),
        "one_bin_middle": _row(nm, {mid: 2.5e11}, weight=T60),
        "now_equals_base": _row(nm, {}, base=0.375, weight=down(T60)),
        "empty_on_the_floor": _row(nm, {}, base=FLOOR, weight=FLOOR),
        "one_ulp_of_base": (np.full(nm + 1, 1.0), np.where(np.arange(nm + 1) == mid + 1, up(1.0), 1.0), 0.5),
        "floor_base_real_deposits": _row(nm, {l: float(rng.uniform(0.1, 2.0)) * 10.0 ** int(rng.integers(-12, 3)) for l in range(3, nm, 2)}, base=FLOOR),
        "around_1e-60": _row(nm, {1: 1.0, 4: T60, 5: down(T60), 6: up(T60), nm - 1: 1.0e-61}, weight=1.0e-3),
        "number_at_1e-99": _row(nm, {mid: FLOOR}),
        "number_above_1e-99": _row(nm, {mid: up(FLOOR)}),
        "number_below_1e-99": _row(nm, {mid: down(FLOOR)}),
        "two_bins_adjacent": _row(nm, {mid: 0.3, mid + 1: 0.7}),
    }
    for j, r in enumerate(tie_rows(nm, 2, nm - 2)):
        rows[f"tie_q{j}"] = r
    for s in range(3):
        d = rng.uniform(0.5, 1.5, nm + 1) * 10.0 ** (-0.02 * (s + 1) * np.arange(nm + 1) * rng.uniform(0.5, 1.5, nm + 1))
        b = rng.uniform(0.0, 5.0, nm + 1) if s else np.zeros(nm + 1)
        n = b + d
        n[::5] = b[::5]                    # (every fifth bin took nothing)
        rows[f"dense_{s}"] = (b, n, float(rng.uniform(0.1, 1.0)))
    return rows


DEAD = "now_equals_base"


def scenarios(nm):
    """name -> the rows of a call, one per time cut: n_tcuts = 1, 3 and 99."""
    R = crafted_rows(nm)
    names = list(R)
    out = {f"one_cut_{n}": [R[n]] for n in ("one_bin_middle", "now_equals_base", "dense_1")}
    out["three_cuts_two_live"] = [R["dense_0"], R[DEAD], R["two_bins_adjacent"]]                    # index NaN
    out["three_cuts_three_live"] = [R["one_bin_first"], R["dense_2"], R["one_bin_last"]]            # index finite
    out["three_cuts_ties"] = [R["tie_q0"], R["tie_q1"], R["tie_q2"]]
    out["99_cuts_every_row"] = [R[names[k % len(names)]] for k in range(99)]
    out["99_cuts_three_live_apart"] = [R["dense_1"] if k == 0 else R["one_bin_middle"] if k == 50 else R["dense_2"] if k == 98 else R[DEAD] for k in range(99)]
    out["99_cuts_two_live_apart"] = [R["dense_1"] if k == 0 else R["dense_2"] if k == 91 else R["empty_on_the_floor"] for k in range(99)]
    return out


def tcuts_for(prob, nt):
    """nt increasing times whose last lies above 10 age_max, as the inputs demand."""
    top = 20.0 * prob.params.age_max
    return np.array([top]) if nt == 1 else np.logspace(2.0, math.log10(top), nt)


def load_rows(be, prob, i_ion, rows, i_iter=1):
    """Puts the rows of a scenario on a context: the base rows into the species' block of spectra_coupled, begin_species (which takes
    the base), then the "now" rows and the weights -- this is how a test sets a base other than zero.  NaN goes into the rows k >= nt,
    the words l > nmom, the other ions' blocks and the other ions' weights: none of it may leave a trace.  Sets the context's cuts to
    len(rows) time cuts.  -> (now [nt][nm+1], base [nt][nm+1], weight [nt], the block [100][201] as begin_species found it)."""
    nt, nm = len(rows), prob.params.num_psd_mom_bins
    prob.tcuts = tcuts_for(prob, nt)
    be.set_cuts(prob)
    L = be.layout
    sp = prob.cfg.species[i_ion - 1]
    base = np.array([r[0] for r in rows]); now = np.array([r[1] for r in rows]); weight = np.array([r[2] for r in rows])
    sc = np.full(L.shapes["spectra_coupled"], np.nan)
    sc[i_ion - 1, :nt, :nm + 1] = base
    be.write_tally("spectra_coupled", sc)
    be.begin_species(i_iter, i_ion, sp.aa, abs(sp.zz), prob.pmax, sp.density, 1.0)
    block = sc[i_ion - 1].copy()
    sc[i_ion - 1, :nt, :nm + 1] = now
    be.write_tally("spectra_coupled", sc)
    wc = np.full(L.shapes["weight_coupled"], np.nan)
    wc[i_ion - 1, :nt] = weight
    be.write_tally("weight_coupled", wc)
    return now, base, weight, block


def two_ion_problem(make_problem, **kw):
    """Two species, so that the second one's block starts at a row offset of its own."""
    S = mcs.inputs.Species
    return make_problem(64, species=[S(1.0, 1.0, 1e6, 1.0), S(4.0, 2.0, 1e6, 0.1)], **kw)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_words(a, b):
    """Bit-equal, where a NaN equals a NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def assert_same(got, ref, what):
    """Every output word of a TcutSpectra against the Reference; the NaNs of dead rows are quiet NaNs on both sides."""
    for name in ("spectrum", "weight", "number", "mean_log_p", "quantile", "index"):
        a, b = getattr(got, name), getattr(ref, name)
        assert same_words(a, b), f"{what}: {name} differs in {int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())} words"
    assert np.array_equal(got.diag, ref.diag), f"{what}: diag {got.diag.tolist()} != {ref.diag.tolist()}"
