"""The tally records of tests/tally_common.py and the oracle's walk of them (orc_eval_tally), checked without a GPU.

What the GPU test (tests/test_gpu_tally_records.py) takes for granted is asserted here: that the oracle's walk agrees with the
independent Python restatement (tests/twin/mcs_twin.py) and, for the bins, with exact arithmetic (mpmath at 60 digits); that every
ladder of records really lands in both bins beside its edge, for every edge of bin_momentum and bin_angle; that every branch the
records are meant to reach is reached (read from the log and the counters); and that at least 90 % of the histogram deposits of the
whole suite fall into the bit-exact class of the per-cell rule."""
import functools
import math

import numpy as np
import pytest

from conftest import mcs, oracle_backend
import tally_common as tc
from twin.mcs_twin import Twin

FAR = 2.0 ** -40


@functools.lru_cache(maxsize=None)
def material(name):
    case = tc.make_case(name)
    R, info = tc.build_records(case)
    ob = oracle_backend(case.prob)
    rows, words = R.arrays()
    case.begin(ob)
    T_init, I_init = ob.read_tallies()
    log = ob.eval_tally(rows, words)
    T_all, I_all = ob.read_tallies()
    pool = tc.split(case, R, ob)
    shapes = tc.stack_shapes(case)
    tc.attach_logs(case, pool + shapes, ob)
    return dict(case=case, R=R, info=info, ob=ob, rows=rows, words=words, log=log, T_init=T_init, I_init=I_init, T_all=T_all, I_all=I_all,
                pool=pool, shapes=shapes, probe=tc.Probe(case))


def deposits(mat, rec, name):
    """The deposits of record `rec` into array `name` of the fp64 tallies: [(index tuple, value)]."""
    L = mat["ob"].layout
    lr, lb, lo, lv = mat["log"]
    if "by_rec" not in mat:
        order = np.argsort(lr, kind="stable")
        mat["by_rec"] = (order, np.searchsorted(lr[order], np.arange(len(mat["R"]) + 1)))
    order, start = mat["by_rec"]
    o, n = L.offsets[name], int(np.prod(L.shapes[name]))
    out = []
    for i in order[start[rec]:start[rec + 1]]:
        if lb[i] == 0 and o <= lo[i] < o + n:
            out.append((tuple(int(v) for v in np.unravel_index(lo[i] - o, L.shapes[name])), float(lv[i])))
    return out


def kind_of(mat, rec):
    w = int(mat["words"][rec])
    return (w >> 40) & 0xff, (w >> 24) & 1, (w >> 32) & 0xff, (w >> 16) & 0xff          # kind, inj, aux, ig3


# ---- the oracle's walk against the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", tc.PROBLEMS)
def test_oracle_walk_agrees_with_the_twin(problem):
    """The records that are not placed within an ulp of an edge (the crossings, the exits, the clamp, p_cos = +-1, the far momenta)
    through the twin's flux_tally, particle_finish and tcut_track: every cell within 1e-11 of the oracle's, integers equal."""
    mat = material(problem)
    case, info, R = mat["case"], mat["info"], mat["R"]
    prob, P = case.prob, case.prob.params
    ids = []
    for key in ("crossings", "feb", "finish", "momentum clamp", "p_cos == +-1", "x == x_spec upstream-going: deposit", "x_old == x_spec: no deposit"):
        ids += info["branches"].get(key, [])
    for rec, v, _ in info["direct"]:
        e = P.psd_mom_min * 10.0 ** (round(math.log10(v / P.psd_mom_min) * P.psd_bins_per_dec_mom) / P.psd_bins_per_dec_mom)
        if abs(v / e - 1) > 1e-6:
            ids.append(rec)
    ids = sorted(set(ids))
    assert len(ids) > 100
    ob = oracle_backend(prob)
    case.begin(ob)
    T0, I0 = ob.read_tallies()
    ob.eval_tally(mat["rows"][ids], mat["words"][ids], log=False)
    T1, I1 = ob.read_tallies()
    sp = prob.cfg.species[case.i_ion - 1]
    tw = Twin(prob, 1, case.i_ion, sp.aa, abs(sp.zz), 0.0, sp.density, 1.0)
    for r in ids:
        pb, pp, pt, g, ph, w, x, xo = (float(v) for v in mat["rows"][r])
        wd = int(mat["words"][r])
        kind, inj, aux, z = kind_of(mat, r)
        zone = (tw.ux_g[z], tw.gsf_g[z], math.cos(tw.th_g[z]), math.sin(tw.th_g[z]))
        if kind == tc.KIND_CROSS:
            tw.flux_tally(pb, pp, pt, g, ph, w, wd & 0xff, (wd >> 8) & 0xff, *zone, x, xo, bool(inj))
        elif kind == tc.KIND_FINISH:
            tw.particle_finish(aux, pb, pp, g, ph, *zone, w)
        else:
            tw.tcut_track(aux, w, pt)
    L = ob.layout
    ng = P.n_grid
    assert np.array_equal(tw.num_crossings, I1[:ng] - I0[:ng])
    assert tw.cnt["MOMBIN_CLAMP"] == int(I1[ng + tc.IC_MOMBIN_CLAMP] - I0[ng + tc.IC_MOMBIN_CLAMP]) > 0
    for name in L.offsets:
        a, b = tw.T[name], L.view(T1, name) - L.view(T0, name)
        scale = np.maximum(np.abs(a), np.abs(b))
        bad = np.abs(a - b) > 1e-11 * scale + 1e-90
        assert not bad.any(), f"{problem}: {name}{np.argwhere(bad)[0]}: twin {a[bad][0]!r} oracle {b[bad][0]!r}"
    ob.destroy()


# ---- the bins against exact arithmetic ----------------------------------------------------------------------------------------------
def mp_bin_momentum(mp, P, p):
    """(bin, far) of the double p in exact arithmetic; far: p is further than 2^-40 (relatively) from every edge."""
    if p < P.psd_mom_min:
        return 0, abs(p / P.psd_mom_min - 1) > FAR
    q = mp.log10(mp.mpf(p) / mp.mpf(P.psd_mom_min)) * P.psd_bins_per_dec_mom
    k = int(mp.floor(q))
    far = all(abs(mp.mpf(p) / (mp.mpf(P.psd_mom_min) * mp.power(10, mp.mpf(e) / P.psd_bins_per_dec_mom)) - 1) > FAR for e in (k, k + 1))
    return min(k + 1, P.num_psd_mom_bins), far


def mp_bin_angle(mp, P, px, p):
    """The same for bin_angle on the double p_cos = fl(-px / p), the number the code itself compares with its edges."""
    if p == 0:
        return 0, True
    c = -px / p
    far = abs(c / P.psd_cos_fine - 1) > FAR
    if c < P.psd_cos_fine:
        y = (mp.mpf(c) + 1) / mp.mpf(P.psd_dcos)
        k = int(mp.floor(y))
        far = far and all(abs((mp.mpf(c) + 1) / (e * mp.mpf(P.psd_dcos)) - 1) > FAR for e in (k, k + 1) if e > 0)
        return min(P.num_psd_tht_bins - k, P.num_psd_tht_bins), far
    th = mp.acos(mp.mpf(c)) if c < 1 else mp.mpf(0)
    if th < P.psd_tht_min:
        return 0, far and (th == 0 or abs(th / mp.mpf(P.psd_tht_min) - 1) > FAR)
    q = mp.log10(th / mp.mpf(P.psd_tht_min)) * P.psd_bins_per_dec_tht
    k = int(mp.floor(q))
    far = far and all(abs(th / (mp.mpf(P.psd_tht_min) * mp.power(10, mp.mpf(e) / P.psd_bins_per_dec_tht)) - 1) > FAR for e in (k, k + 1))
    return min(k + 1, P.num_psd_tht_bins), far


@pytest.mark.parametrize("problem", tc.PROBLEMS)
def test_logged_bins_against_exact_arithmetic(problem):
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 60
    mat = material(problem)
    P, pr = mat["case"].prob.params, mat["probe"]
    n_far = n_near = 0
    for rec, v, name in mat["info"]["direct"]:                       # the momentum the record carries is the binned one
        dep = deposits(mat, rec, name)
        assert len(dep) == 1, (rec, name, dep)
        want, far = mp_bin_momentum(mp, P, v)
        got = dep[0][0][-1]
        if far:
            assert got == want, f"{problem}: {tc.describe(mat['rows'][rec], mat['words'][rec], mat['R'].tags[rec])}: bin {got}, exact {want}"
        else:
            assert abs(got - want) <= 1
        n_far += far; n_near += not far
    for rec in range(len(mat["R"])):                                  # every exit: both bins of the shock-frame momentum
        kind, inj, aux, z = kind_of(mat, rec)
        if kind != tc.KIND_FINISH or aux > 2:
            continue
        pb, pp, pt, g, ph = (float(v) for v in mat["rows"][rec][:5])
        ptot_sk, px = pr.sk(z, pb, pp, g, ph)[:2]
        dep = deposits(mat, rec, "esc_psd_down" if aux == 1 else "esc_psd_up")
        assert len(dep) == 1
        (jth, ip) = dep[0][0]
        (wm, fm), (wa, fa) = mp_bin_momentum(mp, P, ptot_sk), mp_bin_angle(mp, P, px, ptot_sk)
        what = f"{problem}: {tc.describe(mat['rows'][rec], mat['words'][rec], mat['R'].tags[rec])}"
        if fm:
            assert ip == wm, f"{what}: momentum bin {ip}, exact {wm}"
        if fa:
            assert jth == wa, f"{what}: angle bin {jth}, exact {wa}"
        n_far += fm + fa; n_near += (not fm) + (not fa)
    print(f"\n{problem}: {n_far} bins checked against exact arithmetic, {n_near} values within 2^-40 of an edge left to the ladders")
    assert n_far > 1000 and n_near > 1000


# ---- the ladders ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", tc.PROBLEMS)
def test_every_ladder_straddles_its_edge(problem):
    """Every edge of bin_angle and of bin_momentum in the shock frame has a ladder, and the records of each ladder land in BOTH bins
    beside the edge -- in the injected crossing's psd cell, the thermal crossing's, the downstream exit's and the upstream exit's."""
    mat = material(problem)
    P = mat["case"].prob.params
    want = {"angle": {(j, j + 1) for j in range(P.num_psd_tht_bins)}, "momentum": {(k, k + 1) for k in range(P.num_psd_mom_bins)}}
    have = {"angle": set(), "momentum": set()}
    users = [("psd", 1, 1, 0), ("therm_sf", 1, 0, 0), ("esc_psd_down", 2, 0, 1), ("esc_psd_up", 2, 0, 2)]
    if not P.track_thermal:
        users.pop(1)
    for what, key, ids in mat["info"]["ladders"]:
        for name, kind, inj, aux in users:
            bins = set()
            for rec in ids:
                k_, inj_, aux_, _ = kind_of(mat, rec)
                if (k_, inj_, aux_) != (kind, inj, aux):
                    continue
                dep = deposits(mat, rec, name)
                assert len(dep) == 1, (what, key, name, rec, dep)
                idx = dep[0][0]
                bins.add(idx[-2] if what == "angle" else idx[-1])
            assert bins == set(key), f"{problem}: the {what} ladder of edge {key} lands in bins {sorted(bins)} of {name}"
        have[what].add(key)
    for what in want:
        assert have[what] == want[what], f"{problem}: {what} edges without a ladder: {sorted(want[what] - have[what])[:8]}"
    # the named edges are among them: psd_tht_min is the edge (0, 1), psd_cos_fine the one between the last log-theta bin and the first linear one
    pr = mat["probe"]
    n_log = pr.bin_ang(-math.nextafter(P.psd_cos_fine, 2.0), 1.0)
    assert pr.bin_ang(-math.nextafter(P.psd_cos_fine, 0.0), 1.0) == n_log + 1 and (n_log, n_log + 1) in have["angle"] and (0, 1) in have["angle"]


# ---- the branches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", tc.PROBLEMS)
def test_every_branch_is_reached(problem):
    mat = material(problem)
    case, info, pr = mat["case"], mat["info"], mat["probe"]
    P, prob = case.prob.params, case.prob
    L, br = mat["ob"].layout, info["branches"]
    ng, nm = P.n_grid, P.num_psd_mom_bins
    lr, lb, lo, lv = mat["log"]

    def sk(rec):
        pb, pp, pt, g, ph = (float(v) for v in mat["rows"][rec][:5])
        return pr.sk(kind_of(mat, rec)[3], pb, pp, g, ph)
    # the clamp bin and its counter
    clamp_recs = set(lr[(lb == 1) & (lo == ng + tc.IC_MOMBIN_CLAMP)].tolist())
    binned = [r for r in br["momentum clamp"] if P.track_thermal or kind_of(mat, r)[:2] != (tc.KIND_CROSS, 0)]      # (an untracked thermal crossing bins nothing)
    assert len(binned) >= 6 and set(binned) <= clamp_recs
    for rec in br["momentum clamp"]:
        kind, inj, aux, _ = kind_of(mat, rec)
        if kind == tc.KIND_FINISH and aux <= 2:
            assert deposits(mat, rec, "esc_psd_down" if aux == 1 else "esc_psd_up")[0][0][-1] == nm
    assert any(v > P.psd_mom_min * 10.0 ** (nm / P.psd_bins_per_dec_mom) for _, v, _ in info["direct"])
    assert any(v < P.psd_mom_min for _, v, _ in info["direct"]) and any(v == math.nextafter(P.psd_mom_min, 0) for _, v, _ in info["direct"])
    # nothing moves in the shock frame: bin (0, 0), and the weight factor of a vanishing p_x
    for rec in br["ptot_sk == 0"]:
        assert sk(rec)[0] == 0.0
        kind, inj, aux, _ = kind_of(mat, rec)
        name = ("psd" if inj else "therm_sf") if kind == tc.KIND_CROSS else ("esc_psd_down" if aux == 1 else "esc_psd_up")
        if name == "therm_sf" and not P.track_thermal:
            continue
        dep = deposits(mat, rec, name)
        assert len(dep) == 1 and dep[0][0][-2:] == (0, 0) and dep[0][1] == math.inf
    # both sides of the spike-away switch and of the E_rel_pt switch (whose two spellings, > in flux_tally and >= in particle_finish,
    # cannot be told apart: gam_sk - 1 is a multiple of 2^-52 and the double 0.005 is none, so equality never occurs)
    sides = {sk(rec)[0] > abs(sk(rec)[1] * tc.SPIKE_AWAY) for rec in br["spike"]}
    assert sides == {True, False}
    gm1 = [sk(rec)[4] - 1 for rec in br["e_rel"]]
    assert any(g > tc.E_REL_PT for g in gm1) and any(g < tc.E_REL_PT for g in gm1) and not any(g == tc.E_REL_PT for g in gm1)
    assert math.fmod(tc.E_REL_PT, 2.0 ** -52) != 0.0
    # the plasma-frame clamp |px_Xf| > pt_Xf: with a correctly rounded square root pt_tot_sk >= |px| and so pt_Xf >= |px_Xf|: the branch
    # cannot be taken, and p_y = p_z = 0 sits on its edge, pt_Xf == |px_Xf| (p_cos = -+1 in that frame: the first and the last angle bin)
    if "p_cos == +-1" in br:
        for rec in br["p_cos == +-1"]:
            s = sk(rec)
            assert s[2] == 0.0 and s[3] == 0.0 and s[0] == abs(s[1])
            kind, inj, aux, _ = kind_of(mat, rec)
            if kind == tc.KIND_CROSS and not inj and P.track_thermal:
                assert deposits(mat, rec, "therm_pf")[0][0][-2] in (0, P.num_psd_tht_bins)
                assert deposits(mat, rec, "therm_sf")[0][0][-2] in (0, P.num_psd_tht_bins)
    for rec in range(len(mat["R"])):
        kind, inj, aux, _ = kind_of(mat, rec)
        if kind == tc.KIND_CROSS and not inj and rec % 7 == 0:
            s = sk(rec)
            assert s[0] >= abs(s[1])
    # crossings: an injected particle moving upstream leaves no trace in the zones up to i_grid_feb; a thermal one does
    feb = P.i_grid_feb
    seen_skip = seen_noskip = 0
    for rec in br["crossings"]:
        kind, inj, aux, _ = kind_of(mat, rec)
        wd = int(mat["words"][rec])
        i_new, i_old = wd & 0xff, (wd >> 8) & 0xff
        zones = sorted(idx[0] + 1 for idx, _ in deposits(mat, rec, "psd" if inj else "therm_sf")) if (inj or P.track_thermal) else None
        if zones is None:
            continue
        if i_new > i_old:
            assert zones == list(range(i_old + 1, i_new + 1))
        elif inj:
            assert zones == [i for i in range(i_new + 1, i_old + 1) if i > feb]
            seen_skip += i_new + 1 <= feb < i_old
        else:
            assert zones == list(range(i_new + 1, i_old + 1))
            seen_noskip += i_new + 1 <= feb < i_old
    assert seen_skip >= 2 and (seen_noskip >= 2 or not P.track_thermal)
    # the escape scalars: exactly the injected records that pass feb_upstream going upstream (x < feb <= x_old)
    sc = L.offsets["scalars"]
    hit = set(lr[(lb == 0) & ((lo == sc + 2) | (lo == sc + 3))].tolist())
    want = {rec for rec in br["feb"] if kind_of(mat, rec)[1] and mat["rows"][rec][6] < P.feb_upstream <= mat["rows"][rec][7]}
    assert hit & set(br["feb"]) == want and len(want) == 2 and len(br["feb"]) - len(want) >= 4
    # exits: 3 and 4 leave nothing, 1 one deposit, 2 six (esc_flux, esc_psd_up, px_esc_feb, energy_esc_feb, esc_energy_eff, esc_num_eff)
    for rec in br["finish"]:
        n = int(np.count_nonzero((lr == rec) & (lb == 0)))
        assert n == {1: 1, 2: 6, 3: 0, 4: 0}[kind_of(mat, rec)[2]]
    assert {kind_of(mat, rec)[3] for rec in br["finish"]} == set(tc.zone_classes(P))
    # detectors: x == x_spec counts as crossed in either direction, x_old == x_spec in neither
    if len(prob.x_spec):
        for rec in br["x_old == x_spec: no deposit"]:
            assert not deposits(mat, rec, "spectra_sf") and not deposits(mat, rec, "spectra_pf")
        for rec in br["x == x_spec upstream-going: deposit"]:
            assert len(deposits(mat, rec, "spectra_sf")) == 1 and len(deposits(mat, rec, "spectra_pf")) == 1
        assert sum(1 for rec, _, name in info["direct"] if name == "spectra_pf") > 300
    if case.i_ion > 1:
        assert min(lo[(lb == 0) & (lo >= L.offsets["spectra_coupled"]) & (lo < L.offsets["spectra_sf"])]) >= L.offsets["spectra_coupled"] + (tc.PSD_MAX + 1) * tc.NA_C


# ---- the launches -------------------------------------------------------------------------------------------------------------------
def test_bit_exact_share_and_launch_shapes():
    """No histogram cell of a pool launch receives two deposits; over all problems at least 90 % of the histogram deposits are in
    the bit-exact class; the stack shapes are what they claim to be."""
    n_exact = n_bound = 0
    for problem in tc.PROBLEMS:
        mat = material(problem)
        L = mat["ob"].layout
        assert len(mat["pool"]) <= 24 and sum(int(np.count_nonzero(la.ids >= 0)) for la in mat["pool"]) == len(mat["R"])
        for la in mat["pool"] + mat["shapes"]:
            offs, serial, k, K, S, _, _ = tc.expected(L, mat["T_init"], mat["I_init"], la.log)
            h = tc.is_hist(L, offs)
            if not la.exempt and la in mat["pool"]:
                assert not np.any(k[h] > 1), f"{problem}, {la.name}: {tc.cell_name(L, int(offs[h][np.argmax(k[h])]))} receives {int(k[h].max())} deposits"
            n_exact += int(k[h & (k <= 1)].sum()); n_bound += int(k[h & (k > 1)].sum())
    share = n_exact / (n_exact + n_bound)
    print(f"\nhistogram deposits: {n_exact} bit-exact, {n_bound} bounded: {100 * share:.1f} % bit-exact")
    assert share >= 0.9
    mat = material("protons")
    L = mat["ob"].layout
    by_name = {la.name: la for la in mat["shapes"]}
    assert {la.word.size for la in mat["shapes"] if la.name.endswith("one pass")} == {1, 63, 64, 65, 255, 257, 3001}
    assert all(la.word.shape[1] % 64 for la in mat["shapes"] if "n=" in la.name and la.word.shape[1] > 64 and "three" not in la.name)
    one = by_name["64 in one bin"]
    offs, _, k, *_ = tc.expected(L, mat["T_init"], mat["I_init"], one.log)
    assert sorted(k[tc.is_hist(L, offs)]) == [64]
    for odd in (0, 31, 63):
        la = by_name[f"63 in one bin, lane {odd} in another"]
        offs, _, k, *_ = tc.expected(L, mat["T_init"], mat["I_init"], la.log)
        assert sorted(k[tc.is_hist(L, offs)]) == [1, 63]
        lone = offs[tc.is_hist(L, offs)][np.argmin(k[tc.is_hist(L, offs)])]
        assert la.log[0][(la.log[1] == 0) & (la.log[2] == lone)].tolist() == [odd]
    la = by_name["reasons 1 and 2 with equal bins"]
    offs, _, k, *_ = tc.expected(L, mat["T_init"], mat["I_init"], la.log)
    ho = offs[tc.is_hist(L, offs)]
    assert sorted(k[tc.is_hist(L, offs)]) == [32, 32] and abs(int(ho[0]) - int(ho[1])) == abs(L.offsets["esc_psd_up"] - L.offsets["esc_psd_down"])
    la = by_name["ragged idle lanes, 300 threads x 4 passes"]
    kinds = (la.word >> np.uint64(40)) & np.uint64(3)
    assert la.word.shape == (4, 300) and 0 < np.count_nonzero(kinds == 0) < kinds.size and len({tuple(r) for r in (kinds[:, :64] != 0)}) > 1


def test_log_is_off_by_default_and_changes_nothing():
    mat = material("protons")
    case, ob = mat["case"], mat["ob"]
    la = mat["pool"][-1]
    ob.write_tallies(mat["T_init"], mat["I_init"])
    ob.eval_tally(la.rec, la.word, log=True)
    T1, I1 = ob.read_tallies()
    ob.write_tallies(mat["T_init"], mat["I_init"])
    assert ob.eval_tally(la.rec, la.word, log=False) is None and ob.lib.orc_tally_log(ob.h, 0, None, None, None, None) == 0
    T2, I2 = ob.read_tallies()
    assert np.array_equal(T1.view(np.uint64), T2.view(np.uint64)) and np.array_equal(I1, I2)
    # a whole transport run logs nothing either
    from conftest import make_problem, start_species
    prob = make_problem(64)
    ob2 = oracle_backend(prob)
    start_species(ob2, prob)
    ob2.run_pcut(1, 0)
    assert ob2.lib.orc_tally_log(ob2.h, 0, None, None, None, None) == 0
    ob2.destroy()
    # the log's serial sum is the oracle's buffer, bit for bit
    # the log accounts for the oracle's buffer: one-term cells bit for bit, the others within the bound of the exact sum
    offs, ref, k, K, S, ioffs, iexp = tc.expected(ob.layout, mat["T_init"], mat["I_init"], mat["log"])
    got = mat["T_all"][offs]
    one = k <= 1
    assert np.array_equal(got[one].view(np.uint64), ref[one].view(np.uint64)) and np.array_equal(mat["I_all"][ioffs], iexp)
    fin = np.isfinite(ref) & ~one
    assert np.all(np.abs(got[fin] - ref[fin]) <= tc.bound(K, S)[fin]) and np.array_equal(got[~one & ~fin], ref[~one & ~fin])
    untouched = np.ones(mat["T_all"].size, dtype=bool); untouched[offs] = False
    assert np.array_equal(mat["T_all"][untouched].view(np.uint64), mat["T_init"][untouched].view(np.uint64))


def test_refusals_of_the_oracle_walk():
    mat = material("protons")
    ob, ng = mat["ob"], mat["case"].prob.params.n_grid
    row = np.array([[1e-15, 1e-15, 2e-15, 1.5, 0.1, 1.0, 2.0, 1.0]])
    for word, msg in ((tc.pack(ng + 2, 0, 1, 0, 0, 1), "zone index"), (tc.pack(ng + 1, ng, 1, 0, 0, 1), "outside zones"), (tc.pack(0, 0, 1, 0, 5, 2), "i_reason"),
                      (tc.pack(0, 0, 1, 0, 0, 3), "time cut"), (np.uint64(4 << 40), "unknown kind")):
        with pytest.raises(RuntimeError, match=msg):
            ob.eval_tally(row, np.array([word], dtype=np.uint64))
