"""Helpers of the escape-spectra tests (test_escape_spectra_host.py, test_gpu_escape_spectra.py, test_gpu_ens_escape.py): crafted
escape slabs and a restatement of mcs_dndp_esc (include/mcs.h) that shares no code with csrc/mcs_consumers.hip.

The restatement is built only from what consumers_common.py proves bit for bit against the kernel's arithmetic: `zone_parts_f64`,
called on ONE angle row of a door's slab at a time, so that the row of every part is known; `shock_frame_row`; the library's log10.
The parts are then summed with plain Python floats in the order the header fixes:

  frames 1, 2: R_j[l] = the parts of row j in bin l added to 0.0 with the cell index ascending;
               dN[l] = ((0.0 + R_0[l]) + R_1[l]) + ... + R_nt[l]
  frame 0:     dN[l] = the cells > 0 of column l added to 0.0, rows 0..nt+1 ascending
  number       = ((0.0 + dN[0]) + dN[1]) + ... + dN[nm]
  dNdp[l]      = 1e-99 if dN[l] < 1e-66 else dN[l] / (p_edge[l+1] - p_edge[l]);  dNdp[nm+1] = 1e-99

which yields the expected fp64 word of every output."""
import numpy as np

import consumers_common as cc
from conftest import mcs

PM = 201                      # MCS_PSD_MAX + 1: the fixed stride of an escape slab
FLOOR = 1.0e-99               # what mcs_begin_species fills the slabs with
U = cc.U


def empty_slabs(fill=FLOOR):
    """[door][jtheta][ip], as esc_psd_up | esc_psd_down lie in the tally buffer."""
    return np.full((2, PM, PM), fill)


def write_slabs(hb, slabs):
    """The two slabs into the context's tally buffer, in one write (they are neighbours in the layout)."""
    L = hb.layout
    assert L.offsets["esc_psd_down"] == L.offsets["esc_psd_up"] + PM * PM and slabs.shape == (2, PM, PM)
    hb.write_tally("esc_psd_up", slabs[0])
    hb.write_tally("esc_psd_down", slabs[1])


class Reference:
    """mcs_dndp_esc restated: dN [2][3][nm+2] (before the division; entry nm+1 is frame 0's column sum, 0 in the other frames), dndp,
    number [2][3], diag [2][2], and per (door, frame) the number of adds the longest chain to `number` went through."""

    def __init__(self, dN, dndp, number, diag, n_adds):
        self.dN, self.dndp, self.number, self.diag, self.n_adds = dN, dndp, number, diag, n_adds


_TABLES = {}


def _tables(gam, t):
    key = (float(gam), float(t.rest_energy), t.mom_edge_cgs.tobytes(), t.cos_edge.tobytes())
    if key not in _TABLES:
        if len(_TABLES) > 64:
            _TABLES.clear()
        _TABLES[key] = cc.corner_tables_f64(float(gam), t.rest_energy, t.mom_edge_cgs, t.cos_edge)
    return _TABLES[key]


def row_parts(row, j, gam, t, nm, tables):
    """The parts of angle row j (cells 0..nm of `row`) in the frame `gam` -> ({bin: [part, ...]} with the cell index ascending,
    corner errors, clamps): zone_parts_f64 on a one-row zone whose corner table holds the edges j and j + 1."""
    lpt, ctt = tables
    return cc.zone_parts_f64(np.asarray(row)[None, :], float(gam), t.rest_energy, t.mom_edge_cgs, t.cos_edge[j:j + 2], t.mom_log_cgs, nm, 0,
                             (lpt[j:j + 2], ctt[j:j + 2]))


def reference(slabs, t, gam_pf, nm, nt):
    """slabs [2][201][201], t the consumer tables (mom_log_cgs, mom_edge_cgs, cos_edge, rest_energy, gam0 are read), gam_pf [2]."""
    NM, NT = nm + 2, nt + 2
    pe = [float(v) for v in t.mom_edge_cgs]
    dN = np.zeros((2, 3, NM)); dndp = np.full((2, 3, NM), 1.0e-99); number = np.zeros((2, 3))
    diag = np.zeros((2, 2), dtype=np.int64); n_adds = np.zeros((2, 3), dtype=np.int64)
    for door in range(2):
        slab = slabs[door]
        for m in range(3):
            if m == 0:
                acc = [float(v) for v in cc.shock_frame_row(slab[:NT, :NM])]
                n_adds[door, m] = NT + nm + 1
            else:
                gam = float(gam_pf[door]) if m == 1 else float(t.gam0)
                tables = _tables(gam, t)
                acc = [0.0] * NM
                longest = 0
                for j in range(nt + 1):
                    if not np.any(slab[j, :nm + 1] >= cc.T66):
                        parts, e, c = {}, 0, 0
                    else:
                        parts, e, c = row_parts(slab[j, :NM], j, gam, t, nm, tables)
                    diag[door] += (e, c)
                    longest = max([longest] + [len(v) for v in parts.values()])
                    for l in range(NM):
                        r = 0.0
                        for v in parts.get(l, ()):
                            r = r + v
                        acc[l] = acc[l] + r
                n_adds[door, m] = longest + (nt + 1) + (nm + 1)
            n = 0.0
            for l in range(nm + 1):
                n = n + acc[l]
            number[door, m] = n
            dN[door, m] = acc
            for l in range(nm + 1):
                dndp[door, m, l] = 1.0e-99 if acc[l] < cc.T66 else acc[l] / (pe[l + 1] - pe[l])
    return Reference(dN, dndp, number, diag, n_adds)


def impulse_launches(nm, nt, n_gammas=None):
    """The impulse sweep: every cell (j, i) of the (nt+2) x (nm+2) written part of a slab meets every gamma of cc.GAMMAS (or, with
    n_gammas, so many of them, rotating with the cell) in EACH door; one lit cell per door per launch, the two doors on different
    cells.  Weights cycle through cc.WEIGHTS with cell + gamma index.  The ISM frame's gamma cycles through cc.GAMMAS too.
    -> [(cells [(j, i, value)] per door, gam_pf [2], gam0)]"""
    NM, NT = nm + 2, nt + 2
    G, W = cc.GAMMAS, cc.WEIGHTS
    ncls = len(G) if n_gammas is None else n_gammas
    pairs = [(c, (c + s) % len(G)) for c in range(NM * NT) for s in range(ncls)]
    shift = (NM * NT // 2 + 3) * ncls
    out = []
    for n, (c0, g0) in enumerate(pairs):
        c1, g1 = pairs[(n + shift) % len(pairs)]
        assert c0 != c1
        cells = []
        for c, g in ((c0, g0), (c1, g1)):
            j, i = divmod(c, NM)
            cells.append((j, i, W[(c + g) % len(W)]))
        out.append((cells, (G[g0], G[g1]), G[(n + 2) % len(G)]))
    return out


def impulse_slabs(cells):
    s = empty_slabs()
    for door, (j, i, v) in enumerate(cells):
        s[door, j, i] = v
    return s


def dense_slabs(nm, nt, seed, fill=1.0, decades=80.0, outside=FLOOR):
    """Random slabs over `decades` decades in the style of cc.dense_tallies: a power law in momentum (falling in door 0, rising in
    door 1) times a random angular pattern, a tenth of the cells 0, a tenth 1e-99, of the rest all but the share `fill` 0; rows
    nt+1 and column nm+1 filled too.  outside: what the never-written rows >= nt+2 and columns >= nm+2 hold."""
    NM, NT = nm + 2, nt + 2
    rng = np.random.default_rng(seed)
    s = empty_slabs(outside)
    for door in range(2):
        slope = decades / NM * rng.uniform(0.8, 1.0)
        k = np.arange(NM)
        law = 10.0 ** (10.0 - slope * (k if door == 0 else NM - 1 - k))
        v = law[None, :] * 10.0 ** rng.uniform(-2, 2, (NT, NM))
        u = rng.random((NT, NM))
        v[u < 0.1] = 0.0
        v[(u >= 0.1) & (u < 0.2)] = 1.0e-99
        v[u > 0.2 + 0.8 * fill] = 0.0
        s[door, :NT, :NM] = v
    return s


def escape_tables(prob, i_ion):
    return mcs.consumers.consumer_tables(prob, i_ion)


def bits_equal(a, b):
    return cc.bits_equal(a, b)
