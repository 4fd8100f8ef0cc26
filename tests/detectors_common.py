"""The detector spectra (include/mcs.h, mcs_detector_spectra) restated in plain Python floats from the header's text, the crafted
rows of tests/test_detector_spectra_host.py, tests/test_gpu_detector_spectra.py and tests/test_gpu_ens_detectors.py, and the helper
that puts them on a context.  Nothing here imports the package's consumers module or shares code with csrc/mcs_consumers.hip; the
library's log10 is used where the header names it -- log10(dndp) of the slope, log10(g) of the gradient -- and nowhere else.

  frames f = 0 (spectra_sf), 1 (spectra_pf); detectors d = 0..nd-1; row r = f * nd + d
  g[l] = now[l] - base[l];  number = ((0.0 + g[0]) + g[1]) + ... + g[nmom]
  live: number > 1e-99.  dead: spectrum, dndp 1e-99, number 0.0, mean, quantiles, slope NaN
  live: spectrum[l] = g[l] / number, or 1e-99 below 1e-60; dndp[l] = g[l] / (E[l+1] - E[l]), or 1e-99 where g[l] == 0.0; entry nmom+1 1e-99
  mean_log_p = (sum g[l] * (0.5 * (e[l] + e[l+1]))) / number
  quantile: T = q * number; C_0 = 0.0, C_{l+1} = C_l + g[l]; l* the first l with g[l] > 0 and C_{l+1} >= T;
            f = (T - C_{l*}) / g[l*]; e[l*] + f * (e[l*+1] - e[l*]); the last lit bin with f = 1.0 if none is found
  slope: the slope rule over l_lo <= l < l_hi, valid g[l] > 0, x = 0.5 * (e[l] + e[l+1]), y = log10(dndp[l])
  gradient[l], frame 0: the slope rule over d, valid x_spec[d] < 0.0 and g[0][d][l] > 0, x = x_spec[d] / x_unit, y = log10(g[0][d][l]);
            gradient[nmom+1] NaN"""
import math

import numpy as np

from conftest import mcs

Q = (0.5, 0.9, 0.99)
PM = 201                                 # MCS_PSD_MAX + 1: the row stride of spectra_sf and spectra_pf
FLOOR, T60 = 1.0e-99, 1.0e-60
NAN = float("nan")
X_UNIT = 3.0e9                           # what the crafted positions are multiples of (any finite positive length)


def up(x):
    return float(np.nextafter(x, math.inf))


def down(x):
    return float(np.nextafter(x, -math.inf))


class Reference:
    """The outputs of the call as numpy arrays, and the result as one vector in mcs_detector_layout."""
    NAMES = ("spectrum", "dndp", "number", "mean_log_p", "quantile", "slope", "gradient")

    def __init__(self, diag, **parts):
        for name in self.NAMES:
            setattr(self, name, np.array(parts[name], dtype=np.float64))
        self.diag = np.array(diag, dtype=np.int64)

    def words(self):
        return np.concatenate([getattr(self, name).ravel() for name in self.NAMES])


def quantile_of(g, e, nm, T):
    C, last = 0.0, -1
    for l in range(nm + 1):
        Cn = C + g[l]
        if g[l] > 0:
            if Cn >= T:
                f = (T - C) / g[l]
                return e[l] + f * (e[l + 1] - e[l])
            last = l
        C = Cn
    if last < 0:
        return NAN
    return e[last] + 1.0 * (e[last + 1] - e[last])


def slope_rule(idx, x, y):
    """include/mcs.h, "Slope of frame m", on Python floats over the valid entries idx (ascending); x, y: index -> float."""
    if len(idx) < 3:
        return NAN
    n = float(len(idx))
    sx = sy = 0.0
    for k in idx:
        sx = sx + x(k)
        sy = sy + y(k)
    xbar, ybar = sx / n, sy / n
    sxx = sxy = 0.0
    for k in idx:
        dx = x(k) - xbar
        sxx = sxx + dx * dx
        sxy = sxy + dx * (y(k) - ybar)
    return sxy / sxx if sxx != 0.0 else (NAN if sxy == 0.0 or sxy != sxy else math.copysign(math.inf, sxy))


def reference(now, base, mom_log, mom_edge, x_spec, nm, window, x_unit, log10):
    """now, base: [2][nd][>= nm+1]; mom_log, mom_edge [nm+2]; log10: the library's, arrays -> arrays."""
    nd, NM = len(x_spec), nm + 2
    l_lo, l_hi = window
    e = [float(v) for v in mom_log[:NM]]
    E = [float(v) for v in mom_edge[:NM]]

    def logs(rows):
        """log10 of every positive word of rows (lists of floats) in one call of the library's -> the same lists, None elsewhere."""
        flat = [v for r in rows for v in r if v > 0]
        it = iter(float(v) for v in log10(np.array(flat, dtype=np.float64))) if flat else iter(())
        return [[next(it) if v > 0 else None for v in r] for r in rows]

    spectrum, dndp, number, mean, windows = [], [], [], [], []
    quant = [[], [], []]
    n_neg = n_live = 0
    G = []
    for f in range(2):
        for d in range(nd):
            g = []
            for l in range(nm + 1):
                n_, b_ = float(now[f][d][l]), float(base[f][d][l])
                n_neg += n_ < b_
                g.append(n_ - b_)
            G.append(g)
            num = 0.0
            for l in range(nm + 1):
                num = num + g[l]
            if not num > FLOOR:
                spectrum.append([FLOOR] * NM); dndp.append([FLOOR] * NM); number.append(0.0); mean.append(NAN); windows.append(None)
                for j in range(3):
                    quant[j].append(NAN)
                continue
            n_live += 1
            srow, drow = [], []
            for l in range(nm + 1):
                s = g[l] / num
                srow.append(FLOOR if s < T60 else s)
                drow.append(FLOOR if g[l] == 0.0 else g[l] / (E[l + 1] - E[l]))
            spectrum.append(srow + [FLOOR]); dndp.append(drow + [FLOOR]); number.append(num)
            s = 0.0
            for l in range(nm + 1):
                c = 0.5 * (e[l] + e[l + 1])
                s = s + g[l] * c
            mean.append(s / num)
            for j, q in enumerate(Q):
                quant[j].append(quantile_of(g, e, nm, q * num))
            windows.append([l for l in range(l_lo, l_hi) if g[l] > 0])
    log_dndp = logs([[v if g_ > 0 else 0.0 for v, g_ in zip(dndp[r][:nm + 1], G[r])] for r in range(2 * nd)])
    slope = [NAN if idx is None else slope_rule(idx, lambda l: 0.5 * (e[l] + e[l + 1]), lambda l: log_dndp[r][l]) for r, idx in enumerate(windows)]
    xs = [float(v) for v in x_spec]
    log_g = logs(G[:nd])
    gradient = []
    for l in range(nm + 1):
        idx = [d for d in range(nd) if xs[d] < 0.0 and G[d][l] > 0]
        gradient.append(slope_rule(idx, lambda d: xs[d] / x_unit, lambda d: log_g[d][l]))
    gradient.append(NAN)
    n_fin = sum(1 for v in gradient if math.isfinite(v))
    shape = lambda a, last=None: np.array(a, dtype=np.float64).reshape((2, nd) if last is None else (2, nd, last))
    return Reference([n_live, n_neg, n_fin], spectrum=shape(spectrum, NM), dndp=shape(dndp, NM), number=shape(number), mean_log_p=shape(mean),
                     quantile=np.array(quant, dtype=np.float64).reshape(3, 2, nd), slope=shape(slope), gradient=gradient)


# ---- crafted rows: (base [nm+1], now [nm+1]) ------------------------------------------------------------------------------------------
def _row(nm, lit, base=0.0):
    """A row whose bins `lit` (l -> deposit) grew by their deposit over a flat base."""
    b = np.full(nm + 1, float(base))
    n = b.copy()
    for l, w in lit.items():
        n[l] = n[l] + w
    return b, n


def crafted_rows(nm, seed=0):
    """name -> row."""
    rng = np.random.default_rng(seed)
    mid = nm // 2
    rows = {
        "one_bin_first": _row(nm, {0: 0.75}),
        "one_bin_last": _row(nm, {nm: 3.0e-7}),
        "dead": _row(nm, {}, base=0.375),
        "sum_at_1e-99": _row(nm, {mid: FLOOR}),
        "sum_below_1e-99": _row(nm, {mid - 1: 4.0e-100, mid + 1: 5.0e-100}),
        "sum_above_1e-99": _row(nm, {mid: up(FLOOR)}),
        # a base of 1e6 with growth of a few ulps (an ulp of 1e6 is 2^-33)
        "few_ulps_of_1e6": (np.full(nm + 1, 1.0e6), np.where(np.arange(nm + 1) % 7 == 3, 1.0e6 + 2.0 ** -33 * (1 + np.arange(nm + 1) % 4), 1.0e6)),
        "two_lit": _row(nm, {mid: 0.3, mid + 1: 0.7}),                       # a window over them has two valid bins: slope NaN
        "three_lit": _row(nm, {mid: 0.3, mid + 1: 0.5, mid + 3: 0.2}),        # ... three: finite
    }
    for j, q in enumerate(Q):              # the quantile target falls exactly on a cumulative edge
        g0 = q * 1.0
        g1 = 1.0 - g0
        assert g0 + g1 == 1.0 and q * (g0 + g1) == g0
        rows[f"tie_q{j}"] = _row(nm, {2: g0, nm - 2: g1})
    for s in range(6):
        d = rng.uniform(0.5, 1.5, nm + 1) * 10.0 ** (-0.02 * (s % 3 + 1) * np.arange(nm + 1) * rng.uniform(0.5, 1.5, nm + 1))
        b = rng.uniform(0.0, 5.0, nm + 1) if s % 2 else np.zeros(nm + 1)
        n = b + d
        n[(s % 5)::5] = b[(s % 5)::5]        # (every fifth bin took nothing)
        rows[f"dense_{s}"] = (b, n)
    for s in range(3):                     # every bin lit
        d = rng.uniform(0.5, 1.5, nm + 1) * 10.0 ** (-0.01 * (s + 1) * np.arange(nm + 1))
        b = rng.uniform(0.0, 5.0, nm + 1) if s else np.zeros(nm + 1)
        rows[f"full_{s}"] = (b, b + d)
    return rows


class Scenario:
    """The rows of a call: frames[f][d] = (base, now), the detectors' positions in units of X_UNIT, the slope window."""

    def __init__(self, sf, pf, x, window=None):
        assert len(sf) == len(pf) == len(x)
        self.frames, self.x, self.window = (sf, pf), [float(v) for v in x], window


def scenarios(nm, n_grid):
    """name -> Scenario: nd = 1, 3, 5 and n_grid."""
    R = crafted_rows(nm)
    names = list(R)
    mid = nm // 2
    full = (0, nm + 1)
    dense = [R[f"dense_{s}"] for s in range(6)]
    # a bin (mid) lit in only two of three upstream detectors: that gradient word is NaN while mid - 1 and mid + 1 stay finite
    b, n = R["full_1"]
    n_out = n.copy(); n_out[mid] = b[mid]
    keep = [mid - 1, mid + 1]
    out = {
        "one_detector_dense": Scenario([dense[0]], [dense[1]], [-0.5], full),
        "one_detector_dead": Scenario([R["dead"]], [R["one_bin_first"]], [-0.5], full),
        "three_upstream_dense": Scenario(dense[0:3], dense[3:6], [-0.5, -0.3, -0.1], full),                      # gradient finite
        "three_upstream_one_bin_in_two": Scenario([R["full_0"], (b, n_out), R["full_2"]], dense[0:3], [-0.5, -0.3, -0.1], (2, nm - 3)),
        "three_two_upstream": Scenario(dense[0:3], dense[3:6], [-0.5, -0.3, 0.05], full),                       # gradient all NaN
        "three_one_at_zero": Scenario(dense[0:3], dense[3:6], [-0.5, 0.0, -0.1], full),                         # 0.0 is not upstream: all NaN
        "three_edges_and_ties": Scenario([R["one_bin_first"], R["one_bin_last"], R["tie_q0"]], [R["tie_q1"], R["tie_q2"], R["few_ulps_of_1e6"]],
                                         [-2.0, -1.0, 1.0], full),
        "three_small_sums": Scenario([R["sum_at_1e-99"], R["sum_below_1e-99"], R["sum_above_1e-99"]], [R["dead"], R["few_ulps_of_1e6"], R["dead"]],
                                     [-0.5, -0.3, -0.1], full),
        "three_window_two_valid": Scenario([R["two_lit"]] * 3, [R["three_lit"]] * 3, [-0.5, -0.3, -0.1], (mid - 1, mid + 4)),
        "three_window_three_valid": Scenario([R["three_lit"]] * 3, [R["two_lit"]] * 3, [-0.5, -0.3, -0.1], (mid, mid + 4)),
        "five_unsorted": Scenario(dense[0:5], dense[1:6], [-0.1, 2.0, -0.5, 0.05, -0.3], (1, nm)),
        "five_every_kind": Scenario([R[k] for k in ("dense_0", "dead", "one_bin_first", "few_ulps_of_1e6", "dense_2")],
                                    [R[k] for k in ("tie_q0", "dense_5", "sum_below_1e-99", "one_bin_last", "three_lit")],
                                    [-0.5, -0.3, -0.1, 0.05, 2.0], full),
        "n_grid_detectors": Scenario([R[names[k % len(names)]] for k in range(n_grid)], [R[names[(k + 5) % len(names)]] for k in range(n_grid)],
                                     [-3.0 + 0.07 * k for k in range(n_grid)], (3, nm + 1)),
    }
    out["three_upstream_one_bin_in_two"].probe = (mid, keep)
    return out


def load_rows(be, prob, i_ion, sc, i_iter=1):
    """Puts a scenario on a context: the detectors' positions as the context's x_spec, the base rows into spectra_sf and spectra_pf,
    begin_species (which takes the base), then the "now" rows -- this is how a test sets a base other than zero.  NaN goes into the rows
    d >= nd and the words l > nmom: none of it may leave a trace.
    -> (now [2][nd][nm+1], base [2][nd][nm+1], the base rows [2][nd][201] as begin_species found them)."""
    nd, nm = len(sc.x), prob.params.num_psd_mom_bins
    prob.x_spec = np.array(sc.x, dtype=np.float64) * X_UNIT
    be.set_cuts(prob)
    L = be.layout
    sp = prob.cfg.species[i_ion - 1]
    base = np.array([[r[0] for r in fr] for fr in sc.frames]); now = np.array([[r[1] for r in fr] for fr in sc.frames])
    names = ("spectra_sf", "spectra_pf")
    T = [np.full(L.shapes[name], np.nan) for name in names]
    for f in range(2):
        T[f][:nd, :nm + 1] = base[f]
        be.write_tally(names[f], T[f])
    be.begin_species(i_iter, i_ion, sp.aa, abs(sp.zz), prob.pmax, sp.density, 1.0)
    block = np.stack([T[0][:nd], T[1][:nd]]).copy()
    for f in range(2):
        T[f][:nd, :nm + 1] = now[f]
        be.write_tally(names[f], T[f])
    return now, base, block


XSPEC_RG = (-0.5, -0.3, -0.1, 0.05, 2.0)


def xspec_problem(make_problem, n, **kw):
    """A problem with a row of detectors at XSPEC_RG times rg0."""
    rg0 = make_problem(64).rg0
    return make_problem(n, XSPEC=tuple(x * rg0 for x in XSPEC_RG), **kw)


def two_ion_problem(make_problem, **kw):
    """Two species; the call is made for the second."""
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
    """Every output word of a DetectorSpectra against the Reference."""
    for name in Reference.NAMES:
        a, b = getattr(got, name), getattr(ref, name)
        assert a.shape == b.shape, f"{what}: {name} has shape {a.shape}, not {b.shape}"
        assert same_words(a, b), f"{what}: {name} differs in {int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())} words"
    assert np.array_equal(got.diag, ref.diag), f"{what}: diag {got.diag.tolist()} != {ref.diag.tolist()}"


def check_claims(name, sc, ref, nm):
    """The properties the scenarios exist for, read off the restatement (so that a change of a builder cannot empty a case)."""
    nd = len(sc.x)
    fin = np.isfinite(ref.gradient)
    assert not fin[nm + 1]
    if name in ("three_two_upstream", "three_one_at_zero", "one_detector_dense", "one_detector_dead"):
        assert not fin.any() and ref.diag[2] == 0
    if name in ("three_upstream_dense", "five_unsorted", "n_grid_detectors"):
        assert fin.sum() >= nm // 3 and ref.diag[2] == fin.sum()
    if name == "three_upstream_one_bin_in_two":
        mid, keep = sc.probe
        assert not fin[mid] and all(fin[l] for l in keep) and fin.sum() == nm
    if name == "three_window_two_valid":
        assert np.all(np.isnan(ref.slope[0])) and np.all(np.isfinite(ref.slope[1])) and np.all(ref.number > 0)
    if name == "three_window_three_valid":
        assert np.all(np.isfinite(ref.slope[0])) and np.all(np.isnan(ref.slope[1])) and np.all(ref.number > 0)
    if name == "three_small_sums":
        assert ref.number[0].tolist() == [0.0, 0.0, up(FLOOR)] and ref.number[1, 0] == 0.0 and ref.number[1, 1] > 0 and ref.diag[0] == 2
        assert ref.number[1, 1] < 1.0e-6 and np.all(ref.dndp[0, 0] == FLOOR) and np.isnan(ref.slope[0, 1])
    if name == "three_edges_and_ties":
        assert ref.spectrum[0, 0, 0] == 1.0 and ref.spectrum[0, 1, nm] == 1.0 and (ref.spectrum[0, 0] > FLOOR).sum() == 1
        assert ref.dndp[0, 1, nm] > FLOOR and ref.dndp[0, 1, nm + 1] == FLOOR
    if name == "one_detector_dead":
        assert ref.number[0, 0] == 0.0 and np.isnan(ref.mean_log_p[0, 0]) and np.all(np.isnan(ref.quantile[:, 0, 0])) and ref.diag[0] == 1
    assert ref.spectrum.shape == (2, nd, nm + 2) and ref.diag[1] == 0
