"""The compute backend of the transport path: libmcs_hip.so (gfx950 kernels)
through the C ABI of include/mcs.h.

There is no other backend in this package and no fallback: if the library or a
GPU is missing, construction fails with an error.  (Tests drive the same host
driver with the CPU oracle by injecting a backend object defined under oracle/;
the product never does.)
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import capi
from .capi import McsSoa, Population, c_double_p, c_int64_p, c_uint8_p, c_int32_p


def _dp(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_double_p)


class HipBackend:
    name = "hip"

    def __init__(self, device: int = 0, stream: int = 0, torch_tallies: bool = False, debug_finals: bool = False,
                 options: dict | None = None, use_env: bool = True):
        """torch_tallies: keep the flat tally buffers in torch CUDA tensors, so that torch.distributed can
        all-reduce them in place (multi-GPU driver).  The context then works on torch's CURRENT stream
        (passed to mcs_create), so torch ops and library kernels are ordered by that stream; with
        stream=0 and torch_tallies=False the context creates its own blocking stream.
        debug_finals: record per-particle end states for finals() (tests; 24 B of stores per particle).
        options: run options of the context by name, e.g. {"k1_ws": 1} (capi.option_table() lists them, include/mcs.h documents
        them); use_env=False: the MCS_* environment variables, otherwise the default of every option not given, are not read."""
        self.lib = capi.load_library()          # raises MissingNativeLibrary
        if self.lib.mcs_abi_version() != capi.MCS_ABI_VERSION:
            raise RuntimeError("libmcs_hip.so ABI version mismatch")
        self.device = int(device)
        self.stream = int(stream)
        self.torch_tallies = torch_tallies
        self.debug_finals = debug_finals
        self._options = {capi.option_key(name): int(v) for name, v in (options or {}).items()}     # KeyError: no such option
        self.use_env = bool(use_env)
        self.h = ct.c_void_p(None)
        self._bound = None

    # -- lifecycle
    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError("libmcs_hip: " + self.lib.mcs_last_error().decode())

    def create(self, prob):
        self.prob = prob
        self.P = prob.params
        self.layout = capi.Layout(self.P)
        if self.torch_tallies:
            import torch
            torch.cuda.set_device(self.device)
            self.stream = int(torch.cuda.current_stream(self.device).cuda_stream)
        keys = (ct.c_int32 * len(self._options))(*self._options.keys())
        values = (ct.c_int64 * len(self._options))(*self._options.values())
        self._chk(self.lib.mcs_create_with_options(ct.byref(self.P), self.device, ct.c_void_p(self.stream or None), keys, values,
                                                   len(self._options), int(self.use_env), ct.byref(self.h)))
        if self.debug_finals:
            self._chk(self.lib.mcs_set_debug_finals(self.h, 1))
        if self.torch_tallies:
            dev = torch.device("cuda", self.device)
            t_f = torch.zeros(self.layout.total, dtype=torch.float64, device=dev)
            t_i = torch.zeros(self.layout.n_i64, dtype=torch.int64, device=dev)
            self.bind_torch_tallies(t_f, t_i)
        self.set_grid(prob)
        self.set_cuts(prob)

    def set_grid(self, prob):
        """The grid tables of src/main_loops.jl:255-260 (again after every profile update, iter_finalize.py)."""
        tabs = [np.ascontiguousarray(t, dtype=np.float64) for t in prob.grid_tables()]
        self._chk(self.lib.mcs_set_grid(self.h, len(tabs[0]), *[_dp(t) for t in tabs]))

    def set_cuts(self, prob):
        pc, tc, xs, inj, eps = (np.ascontiguousarray(a, dtype=np.float64) for a in
                                (prob.pcuts, prob.tcuts, prob.x_spec, prob.inj_fracs, prob.eps_target))
        self._chk(self.lib.mcs_set_cuts(self.h, len(pc), _dp(pc), len(tc), _dp(tc), len(xs), _dp(xs), _dp(inj), _dp(eps)))
        self.n_tcuts = len(tc)
        self.n_xspec = len(xs)

    def destroy(self):
        if self.h:
            self.lib.mcs_destroy(self.h)
            self.h = ct.c_void_p(None)

    def bind_torch_tallies(self, t_f64, t_i64):
        """Accumulate into caller-owned torch CUDA tensors (for in-place all-reduce)."""
        assert t_f64.is_cuda and t_f64.numel() >= self.layout.total
        self._bound = (t_f64, t_i64)
        self._chk(self.lib.mcs_bind_tallies(self.h, ct.c_void_p(t_f64.data_ptr()), t_f64.numel(),
                                            ct.c_void_p(t_i64.data_ptr()), t_i64.numel()))

    def tally_tensors(self):
        """Live device tensors (f64, i64) holding the tallies, or None when the context owns them."""
        return self._bound

    def num_cus(self) -> int:
        return int(self.lib.mcs_num_cus(self.h))

    def set_launch(self, blocks: int = 0, threads: int = 0):
        self._chk(self.lib.mcs_set_launch(self.h, blocks, threads))

    def set_tail_slicing(self, budget_trips: int):
        """Sliced tail of run_pcut* (mcs_set_tail_slicing): 0 = one launch per pcut."""
        self._chk(self.lib.mcs_set_tail_slicing(self.h, int(budget_trips)))

    def set_option(self, name: str, value: int):
        """Change a run option for the launches queued from now on (mcs_set_option); RuntimeError with the library's message where
        the option, the value or the moment is not allowed -- the context is then unchanged."""
        self._chk(self.lib.mcs_set_option(self.h, capi.option_key(name), int(value)))

    def get_option(self, name: str) -> int:
        """The value the next launch will use (mcs_get_option)."""
        v = ct.c_int64(0)
        self._chk(self.lib.mcs_get_option(self.h, capi.option_key(name), ct.byref(v)))
        return int(v.value)

    def options(self) -> dict:
        """Every run option's effective value, by name."""
        return {name: self.get_option(name) for name in capi.option_table()}

    def last_launches(self) -> int:
        return int(self.lib.mcs_last_launches(self.h))

    def last_kernel(self) -> int:
        """0 general, 1 plain, 2 lossy, 3 fp32, 4 fp32 plain loop, 5 fp32 lossy, 6 plain with energy transfer, 7 / 8 wave-specialised, 9 fp32 exact loop,
        10 general sliced, 11 / 12 / 13 the sliced forms of 1 / 2 / 6 (mcs_last_kernel; the K1Kernel enum of csrc/mcs_device.h)"""
        return int(self.lib.mcs_last_kernel(self.h))

    # -- per iteration / species
    def begin_iteration(self, i_iter):
        self._chk(self.lib.mcs_begin_iteration(self.h, i_iter))

    def begin_species(self, i_iter, i_ion, aa, zz, pmax_cutoff, density, ewf):
        self._chk(self.lib.mcs_begin_species(self.h, i_iter, i_ion, aa, zz, pmax_cutoff, density, ewf))

    def set_fluxes(self, pxx, pxz, en):
        a, b, c = (np.ascontiguousarray(v, dtype=np.float64) for v in (pxx, pxz, en))
        self._chk(self.lib.mcs_set_fluxes(self.h, _dp(a), _dp(b), _dp(c)))

    # -- population
    def init_pop(self, inj, j_offset, n_local, n_total, j_stride: int = 1):
        """K3 from the binned momentum discretisation: O(bins) host work and upload, whatever N.  Local particle k is
        global particle j_offset + k * j_stride."""
        bp = np.ascontiguousarray(inj.bin_ptot, dtype=np.float64)
        bw = np.ascontiguousarray(inj.bin_weight, dtype=np.float64)
        bs = np.ascontiguousarray(inj.bin_start, dtype=np.int64)
        self._chk(self.lib.mcs_init_pop_binned_strided(self.h, n_local, j_offset, j_stride, n_total, len(bp), _dp(bp), _dp(bw),
                                                       bs.ctypes.data_as(c_int64_p), inj.x_start_cm, inj.i_grid_start,
                                                       int(inj.relativistic), int(inj.fast_push)))

    def init_pop_arrays(self, inj, j_offset, n_local, n_total):
        """K3 from per-particle arrays (the reference's own form of the call)."""
        ptot = np.ascontiguousarray(inj.ptot_pf[j_offset:j_offset + n_local], dtype=np.float64)
        w = np.ascontiguousarray(inj.weight[j_offset:j_offset + n_local], dtype=np.float64)
        self._chk(self.lib.mcs_init_pop(self.h, n_local, j_offset, n_total, _dp(ptot), _dp(w), inj.x_start_cm,
                                        inj.i_grid_start, int(inj.relativistic), int(inj.fast_push)))

    def set_population(self, pop: Population):
        s = pop.soa()
        self._chk(self.lib.mcs_pop_upload(self.h, pop.n, ct.byref(s)))

    def get_population(self) -> Population:
        n = self.pop_size()
        pop = Population(n)
        s = pop.soa()
        self._chk(self.lib.mcs_pop_download(self.h, n, ct.byref(s)))
        return pop

    def pop_size(self) -> int:
        return int(self.lib.mcs_pop_size(self.h))

    def run_pcut(self, i_pcut, i_prt_offset, i_prt_stride: int = 1) -> int:
        """Local particle k has the global 0-based index i_prt_offset + k * i_prt_stride."""
        ns = ct.c_int64(0)
        self._chk(self.lib.mcs_run_pcut_strided(self.h, i_pcut, i_prt_offset, i_prt_stride, ct.byref(ns)))
        self._n_saved_last = int(ns.value)
        return int(ns.value)

    def run_pcut_indexed(self, i_pcut, gidx) -> int:
        """Local particle k has the global 0-based index gidx[k] (int64 CUDA tensor, kept alive here until the next run)."""
        import torch
        assert gidx.is_cuda and gidx.dtype == torch.int64 and gidx.is_contiguous() and gidx.numel() == self.pop_size()
        torch.cuda.current_stream(self.device).synchronize()
        self._gidx_keep = gidx
        ns = ct.c_int64(0)
        self._chk(self.lib.mcs_run_pcut_indexed(self.h, i_pcut, ct.c_void_p(gidx.data_ptr()), ct.byref(ns)))
        self._n_saved_last = int(ns.value)
        return int(ns.value)

    def saved_gidx(self):
        """Global indices of the particles the last run_pcut* saved, in local order (int64 CUDA tensor; mcs_saved_gidx)."""
        import torch
        n = self._n_saved_last
        g = torch.zeros(max(n, 1), dtype=torch.int64, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(self.device).synchronize()
        self._chk(self.lib.mcs_saved_gidx(self.h, max(n, 1), ct.c_void_p(g.data_ptr())))
        return g[:n]

    def set_retro_cap(self, cap: int):
        self._chk(self.lib.mcs_set_retro_cap(self.h, int(cap)))

    # -- multi-GPU new_pcut: saved particles out (to be all-gathered), global split slice in
    def export_saved(self, cap: int):
        """(gidx int64[cap], f64[8, cap], meta int32[cap]) torch CUDA tensors; the first n_saved columns are
        the saved particles of the last run_pcut in index order (mcs_saved_export)."""
        import torch
        dev = torch.device("cuda", self.device)
        gidx = torch.zeros(cap, dtype=torch.int64, device=dev)
        f64 = torch.zeros((8, cap), dtype=torch.float64, device=dev)
        meta = torch.zeros(cap, dtype=torch.int32, device=dev)      # the packed uint32 word, bit pattern kept
        torch.cuda.current_stream(self.device).synchronize()
        self._chk(self.lib.mcs_saved_export(self.h, cap, ct.c_void_p(gidx.data_ptr()), ct.c_void_p(f64.data_ptr()),
                                            ct.c_void_p(meta.data_ptr())))
        return gidx, f64, meta

    def import_split(self, f64, meta, n_parents: int, i_mult: int, first: int, stride: int, n_local: int):
        """New local population = elements first + k*stride of the global split of the parents (mcs_split_import)."""
        import torch
        assert f64.is_cuda and f64.is_contiguous() and meta.is_contiguous() and f64.shape[0] == 8
        torch.cuda.current_stream(self.device).synchronize()
        self._chk(self.lib.mcs_split_import(self.h, n_parents, f64.shape[1], ct.c_void_p(f64.data_ptr()),
                                            ct.c_void_p(meta.data_ptr()), i_mult, first, stride, n_local))

    def run_pcut_host(self, i_pcut, pop: Population, i_prt_offset=0):
        """The literal drop-in call (host buffers in, saved arrays out)."""
        saved = Population(pop.n)
        l_save = np.zeros(pop.n, dtype=np.uint8)
        ns = ct.c_int64(0)
        si, so = pop.soa(), saved.soa()
        self._chk(self.lib.mcs_run_pcut_host(self.h, i_pcut, pop.n, i_prt_offset, ct.byref(si), ct.byref(so),
                                             l_save.ctypes.data_as(c_uint8_p), ct.byref(ns)))
        return saved, l_save, int(ns.value)

    def get_saved(self):
        n = self.pop_size()
        saved = Population(n)
        l_save = np.zeros(n, dtype=np.uint8)
        s = saved.soa()
        self._chk(self.lib.mcs_saved_download(self.h, n, ct.byref(s), l_save.ctypes.data_as(c_uint8_p)))
        return saved, l_save

    def finals(self):
        if not self.debug_finals:
            raise RuntimeError("finals() needs HipBackend(..., debug_finals=True)")
        n = self.pop_size()
        reason = np.zeros(n, np.int32); helix = np.zeros(n, np.int32); retro = np.zeros(n, np.int32)
        ptot = np.zeros(n); x = np.zeros(n)
        self._chk(self.lib.mcs_final_download(self.h, n, reason.ctypes.data_as(c_int32_p), helix.ctypes.data_as(c_int32_p),
                                              retro.ctypes.data_as(c_int32_p), _dp(ptot), _dp(x)))
        return dict(reason=reason, helix=helix, retro=retro, ptot=ptot, x=x)

    def new_pcut(self, i_mult) -> int:
        nn = ct.c_int64(0)
        self._chk(self.lib.mcs_new_pcut(self.h, i_mult, ct.byref(nn)))
        return int(nn.value)

    # -- tallies
    def sync(self):
        """Everything launched so far is done and the bound tally tensors are complete (replicas folded in)."""
        self._chk(self.lib.mcs_sync(self.h))

    def read_tallies(self):
        f = np.zeros(self.layout.total)
        i = np.zeros(self.layout.n_i64, dtype=np.int64)
        self._chk(self.lib.mcs_read_tallies(self.h, _dp(f), i.ctypes.data_as(c_int64_p)))
        return f, i

    def read_tallies_light(self):
        """The same shapes as read_tallies, but only the part of the fp64 buffer behind the three big histograms is
        fetched (fluxes, escape spectra, coupled spectra, pools, scalars: what the host's iter_finalize reads); psd /
        therm_sf / therm_pf read as zeros -- their consumers (K4) run on the device."""
        f = np.zeros(self.layout.total)
        i = np.zeros(self.layout.n_i64, dtype=np.int64)
        first = int(self.layout.offsets["esc_psd_up"])
        tail = f[first:]
        self._chk(self.lib.mcs_read_tallies_part(self.h, first, tail.size, _dp(tail), i.ctypes.data_as(c_int64_p)))
        return f, i

    def run_pcuts_fused(self, i_pcut_first: int, i_pcut_last: int, n_target):
        """mcs_run_pcuts_fused: the pcuts first .. last of the current species queued back to back, n_saved / i_mult / the next
        population's size decided on the device -> (n_use, n_saved, i_mult, kernel_ms) per pcut.  driver.run(fused_pcuts=False): not used."""
        npc = i_pcut_last - i_pcut_first + 1
        tg = np.ascontiguousarray(n_target, dtype=np.int64)
        assert tg.shape == (npc,)
        nu, ns, im = (np.zeros(npc, dtype=np.int64) for _ in range(3))
        ms = np.zeros(npc)
        self._chk(self.lib.mcs_run_pcuts_fused(self.h, int(i_pcut_first), int(i_pcut_last), tg.ctypes.data_as(c_int64_p), nu.ctypes.data_as(c_int64_p),
                                               ns.ctypes.data_as(c_int64_p), im.ctypes.data_as(c_int64_p), _dp(ms)))
        return nu, ns, im, ms

    def run_pcuts_pipelined(self, i_pcut_first: int, i_pcut_last: int, n_target, long_draws: int, long_imult_max: int = 0):
        """mcs_run_pcuts_pipelined: the pcuts first .. last of the current species with every pcut's long histories (>= long_draws random
        draws) finishing beside the next pcut on a second stream -> (n_use, n_saved, i_mult, kernel_ms, strag[npc][2]) per pcut; strag:
        particles exported, and 1 where i_mult had to wait for them.  The next population is ordered non-long before long (include/mcs.h);
        long_imult_max > 0: only in pcuts whose predecessor split by at most that factor."""
        npc = i_pcut_last - i_pcut_first + 1
        tg = np.ascontiguousarray(n_target, dtype=np.int64)
        assert tg.shape == (npc,)
        nu, ns, im = (np.zeros(npc, dtype=np.int64) for _ in range(3))
        ms = np.zeros(npc)
        sg = np.zeros((npc, 2), dtype=np.int64)
        self._chk(self.lib.mcs_run_pcuts_pipelined(self.h, int(i_pcut_first), int(i_pcut_last), tg.ctypes.data_as(c_int64_p), int(long_draws), int(long_imult_max),
                                                   nu.ctypes.data_as(c_int64_p), ns.ctypes.data_as(c_int64_p), im.ctypes.data_as(c_int64_p), _dp(ms),
                                                   sg.ctypes.data_as(c_int64_p)))
        return nu, ns, im, ms, sg

    def read_counters(self):
        """The int64 tallies alone (num_crossings + event counters: ~1 KB), no fp64 word."""
        i = np.zeros(self.layout.n_i64, dtype=np.int64)
        self._chk(self.lib.mcs_read_tallies_part(self.h, 0, 0, None, i.ctypes.data_as(c_int64_p)))
        return i

    def write_tallies(self, f, i):
        f = np.ascontiguousarray(f, dtype=np.float64)
        i = np.ascontiguousarray(i, dtype=np.int64)
        self._chk(self.lib.mcs_write_tallies(self.h, _dp(f), i.ctypes.data_as(c_int64_p)))

    def write_tally(self, name: str, arr):
        """One named array of the layout back into the device buffer (mcs_write_tallies_part)."""
        a = np.ascontiguousarray(arr, dtype=np.float64).ravel()
        assert a.size == int(np.prod(self.layout.shapes[name]))
        self._chk(self.lib.mcs_write_tallies_part(self.h, int(self.layout.offsets[name]), a.size, _dp(a)))

    def accumulate_tallies_from(self, other: "HipBackend"):
        """mcs_accumulate_tallies(self, other): other's running sums added into this context's and cleared in other; the
        per-species sections of both stay (include/mcs.h).  Queued on the two streams, no host synchronisation."""
        self._chk(self.lib.mcs_accumulate_tallies(self.h, other.h))

    def k1_blocks_per_cu(self) -> int:
        """Workgroups of the current species' transport kernel a CU holds under an explicit launch geometry (mcs_k1_blocks_per_cu)."""
        n = int(self.lib.mcs_k1_blocks_per_cu(self.h))
        if n <= 0:
            raise RuntimeError("libmcs_hip: " + self.lib.mcs_last_error().decode())
        return n

    # -- consumers of the tallies (K4)
    def dndp_cr(self, tabs):
        """get_dNdp_cr + CR normalisation on the resident psd -> ([3][n_grid][nmom+2], diag[2])."""
        P = self.P
        out = np.zeros((3, P.n_grid, P.num_psd_mom_bins + 2))
        diag = np.zeros(2, dtype=np.int64)
        s = tabs.as_struct()
        self._chk(self.lib.mcs_dndp_cr(self.h, ct.byref(s), _dp(out), diag.ctypes.data_as(c_int64_p)))
        return out, diag

    def thermo_calcs(self, tabs):
        """thermo_calcs on the resident psd / therm_pf / num_crossings -> (P_par, P_perp, energy_density)."""
        n = self.P.n_grid
        a, b, c = np.zeros(n), np.zeros(n), np.zeros(n)
        s = tabs.as_struct()
        self._chk(self.lib.mcs_thermo_calcs(self.h, ct.byref(s), _dp(a), _dp(b), _dp(c)))
        return a, b, c

    def dndp_esc(self, tabs, gam_pf):
        """K10: dN/dp of the escaping particles from the resident escape slabs -> (dNdp [2][3][nmom+2], number [2][3], diag [2][2]);
        door (upstream, downstream) x frame (shock, the door's plasma frame of Lorentz factor gam_pf[door], ISM)."""
        out = np.zeros((2, 3, self.P.num_psd_mom_bins + 2))
        number = np.zeros((2, 3))
        diag = np.zeros((2, 2), dtype=np.int64)
        g = np.ascontiguousarray(gam_pf, dtype=np.float64)
        if g.shape != (2,):
            raise ValueError("dndp_esc: gam_pf holds one Lorentz factor per door")
        s = tabs.as_struct()
        self._chk(self.lib.mcs_dndp_esc(self.h, ct.byref(s), _dp(g), _dp(out), _dp(number), diag.ctypes.data_as(c_int64_p)))
        return out, number, diag

    def angle_dist(self, tabs, l_lo, l_hi):
        """K11: the pitch-angle distributions of every zone over the momentum windows l_lo[m] <= k < l_hi[m], from the resident
        tallies -> (dist [3][n_grid][n_win][ntht+2], number [3][n_grid][n_win], moments [3][n_grid][n_win][2]); frame (shock, the
        zone's plasma frame, ISM)."""
        lo = np.ascontiguousarray(l_lo, dtype=np.int32); hi = np.ascontiguousarray(l_hi, dtype=np.int32)
        if lo.ndim != 1 or lo.shape != hi.shape:
            raise ValueError("angle_dist: l_lo and l_hi hold one bin index per window")
        n_win, ng = len(lo), self.P.n_grid
        dist = np.zeros((3, ng, max(n_win, 1), self.P.num_psd_tht_bins + 2))
        number = np.zeros((3, ng, max(n_win, 1)))
        moments = np.zeros((3, ng, max(n_win, 1), 2))
        s = tabs.as_struct()
        self._chk(self.lib.mcs_angle_dist(self.h, ct.byref(s), n_win, lo.ctypes.data_as(c_int32_p), hi.ctypes.data_as(c_int32_p), _dp(dist),
                                          _dp(number), _dp(moments)))
        return dist, number, moments

    def tcut_spectra(self, tabs):
        """K12: the spectra of the time cuts of the context's current species from the resident weight_coupled and spectra_coupled and
        the base taken at begin_species -> (out, diag [2]); `out` in mcs_tcut_layout (capi.tcut_layout), diag = (live rows, words with
        now < base)."""
        if self.n_tcuts < 1:
            raise ValueError("tcut_spectra: the context has no time cuts")
        out = np.zeros(capi.tcut_layout(self.P, self.n_tcuts).total)
        diag = np.zeros(2, dtype=np.int64)
        s = tabs.as_struct()
        self._chk(self.lib.mcs_tcut_spectra(self.h, ct.byref(s), _dp(out), diag.ctypes.data_as(c_int64_p)))
        return out, diag

    def profile_update(self, pin, pressures=None):
        """K13: the shock-profile update from the resident fluxes and running scalars, the grid tables of set_grid and the pressures
        mcs_thermo_calcs left on the device -- or `pressures` = (P_par, P_perp, energy_density), host [n_grid] each, in their place
        -> (out, diag [3]); `out` in mcs_profile_layout (capi.profile_layout), diag = (non-finite output words, zones whose Newton ran
        out of steps, the largest Newton step count).  pin: a consumers.ProfileIn."""
        n = self.P.n_grid
        out = np.zeros(capi.profile_layout(self.P).total)
        diag = np.zeros(3, dtype=np.int64)
        s = pin.as_struct()
        pr = None
        if pressures is not None:
            pr = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).ravel()[:n] for a in pressures]))
            if pr.size != 3 * n:
                raise ValueError("profile_update: the pressures are three arrays of n_grid doubles")
        self._chk(self.lib.mcs_profile_update(self.h, ct.byref(s), _dp(pr) if pr is not None else None, _dp(out),
                                              diag.ctypes.data_as(c_int64_p)))
        return out, diag

    def detector_spectra(self, tabs, l_lo: int, l_hi: int, x_unit: float):
        """K14: the spectra at the detectors for the context's current species from the resident spectra_sf and spectra_pf and the base
        taken at begin_species -> (out, diag [3]); `out` in mcs_detector_layout (capi.detector_layout), diag = (live rows, words with
        now < base, finite gradient words)."""
        if self.n_xspec < 1:
            raise ValueError("detector_spectra: the context has no detector")
        out = np.zeros(capi.detector_layout(self.P, self.n_xspec).total)
        diag = np.zeros(3, dtype=np.int64)
        s = tabs.as_struct()
        self._chk(self.lib.mcs_detector_spectra(self.h, ct.byref(s), int(l_lo), int(l_hi), float(x_unit), _dp(out), diag.ctypes.data_as(c_int64_p)))
        return out, diag

    def photon_synch(self, dndp_pf, mom_edge_cgs, mc, n_photon, emin_mev, bins_per_dec):
        """K5: synchrotron emission dP/d(ln E) [erg/s] per zone from the plasma-frame electron dN/dp -> (E_erg[n_photon], emis[n_grid][n_photon])."""
        d = np.ascontiguousarray(dndp_pf, dtype=np.float64); pe = np.ascontiguousarray(mom_edge_cgs, dtype=np.float64)
        assert d.shape == (self.P.n_grid, self.P.num_psd_mom_bins + 2) and pe.shape == (self.P.num_psd_mom_bins + 2,)
        E = np.zeros(n_photon); out = np.zeros((self.P.n_grid, n_photon))
        self._chk(self.lib.mcs_photon_synch(self.h, _dp(d), _dp(pe), float(mc), int(n_photon), float(emin_mev), float(bins_per_dec), _dp(E), _dp(out)))
        return E, out

    def photon_pion(self, dndp_pf, mom_edge_cgs, mc, aa, target_density, scaling, n_photon, emin_mev, bins_per_dec, i_data=1):
        """K7: pion-decay emission dP/d(ln E) [erg/s] per zone from the plasma-frame dN/dp of a nucleus species -> (E_erg[n_photon],
        emis[n_grid][n_photon])."""
        d = np.ascontiguousarray(dndp_pf, dtype=np.float64); pe = np.ascontiguousarray(mom_edge_cgs, dtype=np.float64)
        td = np.ascontiguousarray(target_density, dtype=np.float64)
        assert d.shape == (self.P.n_grid, self.P.num_psd_mom_bins + 2) and pe.shape == (self.P.num_psd_mom_bins + 2,)
        assert td.shape == (self.P.n_grid,)
        E = np.zeros(n_photon); out = np.zeros((self.P.n_grid, n_photon))
        self._chk(self.lib.mcs_photon_pion(self.h, _dp(d), _dp(pe), float(mc), float(aa), _dp(td), float(scaling), int(i_data), int(n_photon),
                                           float(emin_mev), float(bins_per_dec), _dp(E), _dp(out)))
        return E, out

    def dndp_2d(self, tabs, gam_x, beta_x, download=True):
        """K6: get_dNdp_2D on the resident histograms -> d2N/dp dcos [n_grid][ntht+2][nmom+2] in the frame (gam_x, beta_x); the array
        stays on the device for photon_ic (download=False: nothing crosses PCIe)."""
        P = self.P
        out = np.zeros((P.n_grid, P.num_psd_tht_bins + 2, P.num_psd_mom_bins + 2)) if download else None
        s = tabs.as_struct()
        self._chk(self.lib.mcs_dndp_2d(self.h, ct.byref(s), float(gam_x), float(beta_x), _dp(out) if download else None))
        return out

    def photon_ic(self, mom_edge_cgs, mc_e, j_max, alpha_in, n_in, n_photon, emin_mev, bins_per_dec, beam_area):
        """K6: inverse-Compton energy flux per d(ln E) at Earth [erg/(s cm^2)] per zone from the d2N/dp dcos of the last dndp_2d."""
        pe = np.ascontiguousarray(mom_edge_cgs, dtype=np.float64)
        ai = np.ascontiguousarray(alpha_in, dtype=np.float64); ni = np.ascontiguousarray(n_in, dtype=np.float64)
        assert pe.shape == (self.P.num_psd_mom_bins + 2,) and ai.shape == ni.shape
        E = np.zeros(n_photon); out = np.zeros((self.P.n_grid, n_photon))
        self._chk(self.lib.mcs_photon_ic(self.h, _dp(pe), float(mc_e), int(j_max), int(len(ai)), _dp(ai), _dp(ni), int(n_photon), float(emin_mev),
                                         float(bins_per_dec), float(beam_area), _dp(E), _dp(out)))
        return E, out

    def photon_observe(self, process, energy_div, energy_grid, area, dlog, last_mid_ratio, cos_edge, gam_ef, beta_ef, gam3_ef, shell_ends,
                       emis=None, download=True):
        """K9: the observed shell spectra of one emission process ("synch", "ic" or "pion"; mcs_photon_observe in include/mcs.h) ->
        photons per bin [n_shells + 1][n_photon - 1], the last row all shells.  emis=None: from what the last fold of that process left
        on the context; else the caller's [n_grid][n_photon].  The result stays on the device for Ensemble.add_photons; download=False:
        nothing comes back (None is returned)."""
        ed, eg, ce, ga, be, g3 = (np.ascontiguousarray(a, dtype=np.float64) for a in (energy_div, energy_grid, cos_edge, gam_ef, beta_ef, gam3_ef))
        ends = np.ascontiguousarray(shell_ends, dtype=np.int64)
        n_photon, ng = len(ed), self.P.n_grid
        assert eg.shape == (n_photon,) and ce.shape == (181,) and ga.shape == be.shape == g3.shape == (ng,) and ends.ndim == 1 and len(ends) >= 2
        em = None
        if emis is not None:
            em = np.ascontiguousarray(emis, dtype=np.float64)
            assert em.shape == (ng, n_photon)
        out = np.zeros((len(ends), n_photon - 1)) if download else None
        self._chk(self.lib.mcs_photon_observe(self.h, capi.PHOTON_PROCESS[process], n_photon, None if em is None else _dp(em), _dp(ed), _dp(eg),
                                              float(area), float(dlog), float(last_mid_ratio), _dp(ce), _dp(ga), _dp(be), _dp(g3), len(ends) - 1,
                                              ends.ctypes.data_as(c_int64_p), None if out is None else _dp(out)))
        return out

    def last_kernel_ms(self) -> float:
        return float(self.lib.mcs_last_kernel_ms(self.h))

    def eval_fn(self, name: str, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = a if b is None else np.ascontiguousarray(b, dtype=np.float64)
        out = np.zeros_like(a)
        self._chk(self.lib.mcs_eval_fn(self.h, capi.FN[name], len(a), _dp(a), _dp(b), _dp(out)))
        return out

    def eval_scatter(self, form: int, states):
        """One scatter per state in the transport kernel's spelling `form` (0 common pass, 1 lossy kernel / tail ring, 2 tail
        loop: mcs_eval_scatter in include/mcs.h).  states [n][10]: key (as the BITS of the float64 slot: np.uint64 viewed as
        float64), draw index, aa, gyro_denom, ptot_pf, gam_pf, xn_per, pb_pf, p_perp, phi -> [n][5]: pb_pf, p_perp, phi,
        gyro_period, cos_max."""
        s = np.ascontiguousarray(states, dtype=np.float64)
        assert s.ndim == 2 and s.shape[1] == 10
        out = np.zeros((len(s), 5))
        self._chk(self.lib.mcs_eval_scatter(self.h, int(form), len(s), _dp(s), _dp(out)))
        return out

    def eval_tally(self, form: int, rec, word):
        """Caller-given tally records through the transport kernel's own tally code (mcs_eval_tally in include/mcs.h: form 0 direct,
        1 the record stack, 2 the fp32 kernels' stack).  rec [n_pass][n_thread][8]: pb_pf, p_perp, ptot_pf, gam_pf, phi, weight, x,
        x_old; word [n_pass][n_thread] uint64: i_grid | i_grid_old << 8 | ig3 << 16 | inj << 24 | aux << 32 | kind << 40.  The
        deposits land in the context's tallies: read them with read_tallies()."""
        r = np.ascontiguousarray(rec, dtype=np.float64)
        w = np.ascontiguousarray(word, dtype=np.uint64)
        assert w.ndim == 2 and r.shape == w.shape + (8,)
        self._chk(self.lib.mcs_eval_tally(self.h, int(form), w.shape[0], w.shape[1], _dp(r), w.ctypes.data_as(ct.POINTER(ct.c_uint64))))

    def eval_move(self, form: int, post: int, i_pcut: int = 1, x_thr=None):
        """One move of Code Block 2 per state of the context's population (set_population), and what follows it, through the
        transport kernel's own code (mcs_eval_move in include/mcs.h: form 0 move_and_detect, 1 the thresholds of the common pass,
        2 the tail loop's literals, 3 the lossy kernel's thresholds; post 0 nothing, 1 / 2 slow_post pushed / direct, 3 / 4
        plain_crossing pushed / direct).  x_thr: the position at which forms 1-3 compute their thresholds (default: the state's own).
        Returns out [n][18] and the packed word [n] of include/mcs.h; the deposits land in the context's tallies."""
        n = self.pop_size()
        thr = None if x_thr is None else np.ascontiguousarray(x_thr, dtype=np.float64)
        if thr is None and form != 0:
            thr = np.ascontiguousarray(self.get_population().x_PT_cm[:n], dtype=np.float64)
        assert thr is None or thr.shape == (n,)
        out = np.zeros((n, 18))
        word = np.zeros(n, dtype=np.uint64)
        self._chk(self.lib.mcs_eval_move(self.h, int(form), int(post), int(i_pcut), n, None if thr is None else _dp(thr), _dp(out),
                                         word.ctypes.data_as(ct.POINTER(ct.c_uint64))))
        return out, word

    def eval_pass(self, form: int, helix, i_pcut: int = 1):
        """One pass boundary per state of the context's population (set_population): the move of Code Block 2 with what it triggers,
        then the head of Code Block 3 through the transport kernel's own slow_pre (form 0) or the LOSSY kernel's in-line loss (form 1);
        helix: the count of the pass that moves, per state (mcs_eval_pass in include/mcs.h).  Returns out [n][28] and the packed word
        [n]; the deposits land in the context's tallies."""
        n = self.pop_size()
        hx = np.ascontiguousarray(helix, dtype=np.int32)
        assert hx.shape == (n,)
        out = np.zeros((n, 28))
        word = np.zeros(n, dtype=np.uint64)
        self._chk(self.lib.mcs_eval_pass(self.h, int(form), int(i_pcut), n, hx.ctypes.data_as(ct.POINTER(ct.c_int32)), _dp(out),
                                         word.ctypes.data_as(ct.POINTER(ct.c_uint64))))
        return out, word

    def eval_pcut_split(self, form: int, l_save, saved: Population, n=None, *, match=1, i_mult=1, n_target=1, ctr_work=0, ctr_saved=0,
                        n_main_next=0, src_fill=0, guard=64, out_cap=0, export_mode=0, exp_cap=0, exp_first=0, exp_stride=1, exp_gin=None):
        """The pcut bookkeeping kernels on the caller's status bytes and saved states (mcs_eval_pcut_split in include/mcs.h: form 0
        host-sized, 1 device-sized, 2 late).  len(l_save) = saved.n is cap_n; n (default: all of them) the population size the kernels
        are told.  Returns a dict: src [cap_n], scan_total, pd / pd_next (n_use, n_saved, i_mult, n_new), ctr_work, ctr_saved and
        mismatch after the call, out_f64 [8][guard + out_cap + guard] and out_meta (the whole target, guards included), and with
        export_mode 1 / 2 exp_gidx [exp_cap] (2: exp_f64 [8][exp_cap], exp_meta [exp_cap])."""
        ls = np.ascontiguousarray(l_save, dtype=np.uint8)
        cap_n = len(ls)
        assert saved.n == cap_n
        io = capi.McsPcutEval()
        io.form, io.match, io.export_mode = int(form), int(match), int(export_mode)
        io.n, io.cap_n, io.src_fill = cap_n if n is None else int(n), cap_n, int(src_fill)
        io.i_mult, io.n_target, io.n_main_next = int(i_mult), int(n_target), int(n_main_next)
        io.guard, io.out_cap, io.exp_cap, io.exp_first, io.exp_stride = int(guard), int(out_cap), int(exp_cap), int(exp_first), int(exp_stride)
        io.ctr_work, io.ctr_saved = int(ctr_work), int(ctr_saved)
        total = max(2 * int(guard) + int(out_cap), 0)
        s = saved.soa()
        src = np.zeros(cap_n, dtype=np.int64)
        out_f64, out_meta = np.zeros((8, total)), np.zeros(total, dtype=np.uint32)
        ne = max(int(exp_cap), 0) if export_mode else 0
        exp_gidx, exp_f64, exp_meta = np.zeros(ne, dtype=np.int64), np.zeros((8, ne)), np.zeros(ne, dtype=np.uint32)
        u32p = ct.POINTER(ct.c_uint32)
        io.l_save, io.saved, io.src = ls.ctypes.data_as(c_uint8_p), ct.pointer(s), src.ctypes.data_as(c_int64_p)
        io.out_f64, io.out_meta = _dp(out_f64), out_meta.ctypes.data_as(u32p)
        io.exp_gidx, io.exp_f64, io.exp_meta = exp_gidx.ctypes.data_as(c_int64_p), _dp(exp_f64), exp_meta.ctypes.data_as(u32p)
        if exp_gin is not None:
            gin = np.ascontiguousarray(exp_gin, dtype=np.int64)
            assert len(gin) >= io.n
            io.exp_gin = gin.ctypes.data_as(c_int64_p)
        self._chk(self.lib.mcs_eval_pcut_split(self.h, ct.byref(io)))
        return dict(src=src, scan_total=int(io.scan_total), pd=[int(v) for v in io.pd], pd_next=[int(v) for v in io.pd_next],
                    ctr_work=int(io.ctr_work_after), ctr_saved=int(io.ctr_saved_after), mismatch=int(io.mismatch),
                    out_f64=out_f64, out_meta=out_meta, exp_gidx=exp_gidx, exp_f64=exp_f64, exp_meta=exp_meta)
