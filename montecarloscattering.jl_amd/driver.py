"""Host driver: the iteration -> species -> pcut nest of the reference's
`main_loops` (src/main_loops.jl:52-391) around the batched transport kernel.

The reference calls `particle_loop` once per particle (main_loops.jl:228-292);
here one backend call runs a whole pcut.  The population stays resident on the
device between pcuts (K1 transport, K2 compaction+split, K3 initial fill);
the host sees one 8-byte count per pcut.

Multi-GPU (one process per GPU, torch.distributed; RCCL over xGMI when the backend is NCCL).  The RNG key of a
particle is (iteration, species, pcut, GLOBAL particle index) whatever GPU it runs on, so the histories -- and every
tally up to the order of the sums -- are those of a one-GPU run.  Baseline fills (1e-99 floors, analytic fast-push
fluxes) live on rank 0 only so that the sum over ranks is the single-GPU result.
  * The injection is dealt out like cards: rank r of W holds global particles r, r + W, r + 2W, ... -- every rank gets
    the same mix of the momentum-sorted injection (mcs_init_pop_binned_strided).  (Round 1's contiguous ranges put all
    the cold particles on rank 0.)
  * Per pcut ONE small collective, all-gather(n_saved, n_local), then `new_pcut` (src/cuts.jl:34-98 rebuilds the
    population from ALL saved particles) in one of two ways:
      "local"   the bulk of a run (n_saved > `gather_max` and max(count) <= `skew_max` x mean): every rank replicates
                ITS saved particles (K2 exactly as on one GPU); no particle leaves its GPU.  The ranks exchange the
                index column only -- all-gather of the saved particles' global indices, 8 B each -- from which each
                rank finds the position of its saved particles in the global order (one searchsorted per peer) and so
                the global indices of their children, position * i_mult + j: the numbering of src/cuts.jl:66-92.  The
                next pcut runs with that index list (mcs_run_pcut_indexed).
      "gather"  few saved particles (late pcuts: a handful, each replicated 10^5 times, which a local split would
                leave on one or two ranks) or counts that drifted apart: all-gather of the saved particles themselves
                (mcs_saved_export, 72 B each), sorted by global index; rank r builds elements r, r + W, ... of the
                global split (mcs_split_import) -- balanced to one particle whatever the counts were, and the shard
                is an arithmetic progression again (mcs_run_pcut_strided).
  * Per species ONE sum-all-reduce of the flat tally buffers (fp64 + int64), on the device under RCCL.
"""
from __future__ import annotations

import contextlib
import dataclasses
import os
import threading
import time
import types
from concurrent.futures import FIRST_COMPLETED, ThreadPoolExecutor, wait
from typing import Callable, List, Optional

import numpy as np

from . import consumers, inputs, iter_finalize as itf
from . import ensemble as ens
from .capi import IC, RUNNING_F64, running_i64
from .inputs import Problem


@dataclasses.dataclass
class PcutStat:
    i_iter: int
    i_ion: int
    i_pcut: int
    n_pts_use: int          # global
    n_saved: int            # global
    i_mult: int
    n_use_max: int          # largest local population of this pcut over the ranks (load balance: max/mean)
    split: str              # how the NEXT population was built: "local" | "gather" | "identity" (all saved, i_mult 1: nothing moves) | "-" (last pcut)
    kernel_ms: float        # local kernel time (HIP events), nan for CPU backends
    wall_ms: float


@dataclasses.dataclass
class RunResult:
    tallies_f64: np.ndarray       # global (all-reduced) flat tallies after the last species
    tallies_i64: np.ndarray
    per_species: list             # [(i_iter, i_ion, f64, i64)] global tallies at each species end
    stats: List[PcutStat]
    steps_helix: int
    steps_retro: int
    iter_finals: list = dataclasses.field(default_factory=list)   # [(i_iter, IterFinal, IonFinal)] when run(finalize=True)
    iter_state: object = None     # iter_finalize.IterState after the last iteration (run(finalize=True))
    local_steps: list = dataclasses.field(default_factory=list)   # [(i_iter, i_ion, helix + retro steps made by THIS rank's kernels)]
    empty_launches: list = dataclasses.field(default_factory=list)   # [(i_iter, i_ion, i_pcut, kernel_ms)]: transport launches of a fused species
                                                                  # loop on an EMPTY population (the pcuts after the one that saved nobody)
    species_spans: list = dataclasses.field(default_factory=list)    # [(i_iter, i_ion, context index, t_start, t_end)]: host times
                                                                  # (time.perf_counter) around each species' transport, run(species_backends=...)
    options: dict = dataclasses.field(default_factory=dict)          # what the run ran with: the primary backend's options() (a backend that
                                                                  # has them: the run options of the HIP context, by name) and the driver's own
                                                                  # fused_pcuts, fused_chunk, long_draws, long_imult_max as actually used
    ensemble: object = None       # the ensemble statistics the run fed (run(ensemble=...), run_overlapped(ensemble=True)); ensemble.py
    convergence: object = None    # a Convergence: what run / run_overlapped(triggers=...) checked and where it stopped; None without triggers
    photons: object = None        # [consumers.ObservedSpectra], one per species, of the last iteration (run(photons=...)); None without
    escape: object = None         # [(i_iter, i_ion, consumers.EscapeSpectra)] of every species end (run(escape=True)); None without
    tcuts: object = None          # [(i_iter, i_ion, consumers.TcutSpectra)] of every species end (run(tcuts=True)); None without
    profile: object = None        # [(i_iter, consumers.ProfileUpdate)] of every iteration's finalize step (run(profile=True)); None without
    detectors: object = None      # [(i_iter, i_ion, consumers.DetectorSpectra)] of every species end (run(detectors=True)); None without
    angles: object = None         # [(i_iter, i_ion, consumers.AngleDistributions)] of every species end (run(angles=[...])); None without


@dataclasses.dataclass
class TriggerCheck:
    trigger: object               # the ensemble.Trigger
    summary: object               # the ensemble.Summary of its range; None while its slot has fewer than two samples
    value: float                  # the trigger's statistic (nan where it has none)
    met: bool
    predicted_samples: Optional[int]      # ensemble.Trigger.predicted_samples


@dataclasses.dataclass
class Convergence:
    checks: list                  # [(i_iter, [TriggerCheck, in the order of run's triggers])], one per iteration end that was checked
                                  # (run_overlapped: per round end that was checked, i_iter the round's last iteration)
    stopped_at: int               # the last iteration the run did
    satisfied: bool               # every trigger was met at the last check (False: the run did all its n_itrs)


class Comm:
    """Thin torch.distributed wrapper (None/1 rank -> no-ops)."""

    def __init__(self, enabled: bool = False, device=None):
        self.enabled = enabled
        self.rank, self.world = 0, 1
        self.device = device
        if enabled:
            import torch.distributed as dist
            self.dist = dist
            self.rank, self.world = dist.get_rank(), dist.get_world_size()

    def all_gather_ints(self, vals) -> List[List[int]]:
        """A few int64 per rank -> [rank][j] (one collective, one device-to-host copy)."""
        vals = [int(v) for v in vals]
        if not self.enabled:
            return [vals]
        import torch
        # NCCL/RCCL needs device tensors; gloo gathers on the host
        dev = self.device if self.dist.get_backend() == "nccl" else None
        t = torch.tensor(vals, dtype=torch.int64, device=dev)
        out = torch.zeros(self.world * len(vals), dtype=torch.int64, device=dev)     # flat: gloo takes no other shape
        self.dist.all_gather_into_tensor(out, t)
        return out.view(self.world, len(vals)).tolist()

    def all_gather_int(self, v: int) -> List[int]:
        return [r[0] for r in self.all_gather_ints([v])]

    def all_gather_cols(self, t, counts):
        """t: [..., cap] on every rank, rank r's first counts[r] columns valid -> [..., sum(counts)], rank-major."""
        import torch
        if not self.enabled or self.world == 1:
            return t[..., :counts[0]].contiguous()
        flat = torch.zeros(self.world * t.numel(), dtype=t.dtype, device=t.device)
        self.dist.all_gather_into_tensor(flat, t.contiguous().view(-1))
        out = flat.view((self.world,) + tuple(t.shape))
        return torch.cat([out[r][..., :counts[r]] for r in range(self.world)], dim=-1).contiguous()

    def all_gather_rows(self, t):
        """t: [cap] on every rank -> [W, cap]."""
        import torch
        if not self.enabled or self.world == 1:
            return t.view(1, -1)
        flat = torch.empty(self.world * t.numel(), dtype=t.dtype, device=t.device)      # (filled completely by the collective)
        self.dist.all_gather_into_tensor(flat, t.contiguous().view(-1))
        return flat.view(self.world, t.numel())

    def all_reduce_sum_(self, tensor):
        if self.enabled:
            self.dist.all_reduce(tensor, op=self.dist.ReduceOp.SUM)
        return tensor


def shard_range(n: int, rank: int, world: int):
    """Contiguous, balanced index ranges; rank r gets [lo, hi)."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def accumulate_tallies_host(L, dst, src):
    """mcs_accumulate_tallies through the host, for backends without it (the CPU oracle): src's running sums (capi.RUNNING_F64 and
    the event counters) added into dst's, then set to zero in src; the per-species sections of both stay as they are."""
    df, di = dst.read_tallies()
    sf, si = src.read_tallies()
    for name in RUNNING_F64:
        L.view(df, name)[...] += L.view(sf, name)
        L.view(sf, name)[...] = 0.0
    r = running_i64(L)
    di[r] += si[r]
    si[r] = 0
    dst.write_tallies(df, di)
    src.write_tallies(sf, si)


def _launch_share(be, n_flight: int) -> int:
    """Workgroups of one transport launch while n_flight species share the chip: an equal share of the workgroup slots the
    species' kernel has (mcs_k1_blocks_per_cu per CU); 0, the automatic full-chip geometry, for a species alone."""
    if n_flight <= 1:
        return 0
    return max(be.num_cus() * be.k1_blocks_per_cu() // n_flight, 1)


# Optional backend methods and their fallbacks (capability is duck-typed on the instance and looked up at call time: tests wrap
# backends in proxies, tools patch methods).
def _read_light(be):
    """(f64, i64) without the three big histograms where the backend can leave them on the device; the whole buffers otherwise."""
    return be.read_tallies_light() if hasattr(be, "read_tallies_light") else be.read_tallies()


def _read_counters(be):
    """The int64 tallies alone."""
    return be.read_counters() if hasattr(be, "read_counters") else be.read_tallies()[1]


def _steps(i64, n_grid: int):
    """(helix, retro) step counters of an int64 tally buffer, host array or device tensor: never reset, a context's running totals."""
    return int(i64[n_grid + IC["STEPS_HELIX"]]), int(i64[n_grid + IC["STEPS_RETRO"]])


def _zero_running_sums(L, be):
    f, i = _read_light(be)
    if any(np.any(L.view(f, name)) for name in RUNNING_F64) or np.any(i[running_i64(L)]):
        f, i = be.read_tallies()
        for name in RUNNING_F64:
            L.view(f, name)[...] = 0.0
        i[running_i64(L)] = 0
        be.write_tallies(f, i)


class _ChipShare:
    """Launches of several contexts that share the chip (run_overlapped's iterations, run's side-by-side species): how many
    are in flight, and the launch geometry of each while it is not alone."""

    def __init__(self):
        self.n, self.lock = 0, threading.Lock()

    def enter(self):
        with self.lock:
            self.n += 1

    @contextlib.contextmanager
    def geometry(self, be, share: Callable, active=True):
        """For a context that has entered: yields its before_pcut hook, which gives every launch share(number in flight)
        workgroups (0: the automatic geometry); leaves on exit.  Not active, or no set_launch: the hook does nothing."""
        geo = active and hasattr(be, "set_launch")

        def hook(*_):
            # decided before EVERY launch: one left alone on the chip (the last iteration of an odd count, a species whose
            # neighbour has ended) gets the automatic full-chip geometry back
            if geo:
                blocks = int(share(self.n))
                be.set_launch(blocks, 256 if blocks else 0)
        try:
            yield hook
        finally:
            with self.lock:
                self.n -= 1
            if geo:
                be.set_launch(0, 0)          # back to the automatic geometry, also when the body raised


def _pcut_target(rs, i_pcut, p_pcut_hi):
    return rs.prob.cfg.N_PTS_PCUT if rs.prob.pcuts[i_pcut - 1] < p_pcut_hi else rs.prob.cfg.N_PTS_PCUT_HI


def _device_pcut_rows(rs, i_iter, i_ion, counts, wall, note, out_stats, out_empty=None):
    """PcutStat rows and verbose lines (ended by note(ip)) of a pcut loop decided on the device, from its (n_use, n_saved, i_mult, kernel_ms)
    per launch.  The rows end with the pcut that saved nobody; out_empty takes the launches after it (None: they are not recorded)."""
    n_use_a, n_saved_a, i_mult_a, ms_a = counts
    n_rows = next((ip for ip in range(1, len(n_saved_a) + 1) if int(n_saved_a[ip - 1]) == 0), len(n_saved_a))
    n_timed = n_rows if out_empty is None else len(n_saved_a)
    for ip in range(1, n_rows + 1):
        nu, nsv, im = int(n_use_a[ip - 1]), int(n_saved_a[ip - 1]), int(i_mult_a[ip - 1])
        out_stats.append(PcutStat(i_iter, i_ion, ip, nu, nsv, im if nsv > 0 else 0, nu, "-", float(ms_a[ip - 1]), wall / max(n_timed, 1)))
        if rs.verbose and rs.is_root:
            print(f"[iter {i_iter} ion {i_ion} pcut {ip:2d}] n_use={nu} n_saved={nsv} i_mult={im} kernel={ms_a[ip - 1]:.2f} ms {note(ip)}", flush=True)
    if out_empty is not None:
        out_empty.extend((i_iter, i_ion, jp, float(ms_a[jp - 1])) for jp in range(n_rows + 1, len(n_saved_a) + 1))


def _pcuts_pipelined(rs, be, i_iter, i_ion, targets, out_stats):
    """The species' pcuts in one backend call (mcs_run_pcuts_pipelined)."""
    t0 = time.perf_counter()
    *counts, strag_a = be.run_pcuts_pipelined(1, rs.n_pcuts, targets, int(rs.long_draws), int(rs.long_imult_max))
    wall = (time.perf_counter() - t0) * 1e3
    _device_pcut_rows(rs, i_iter, i_ion, counts, wall, lambda ip: f"(pipelined: {int(strag_a[ip - 1][0])} long histories exported"
                      f"{', waited' if strag_a[ip - 1][1] else ''})", out_stats)


def _pcuts_fused(rs, be, i_iter, i_ion, targets, out_stats, out_empty):
    """The species' pcuts in one backend call per chunk (mcs_run_pcuts_fused)."""
    t0 = time.perf_counter()
    # (in chunks: a species that ends early -- the thermal electrons in their first pcut -- would otherwise pay ~35 us of
    # empty launches for every remaining pcut; one read-back per chunk of 12 instead of one per pcut)
    chunk = rs.fused_chunk
    counts = ([], [], [], [])
    for c0 in range(1, rs.n_pcuts + 1, chunk):
        c1 = min(c0 + chunk - 1, rs.n_pcuts)
        got = be.run_pcuts_fused(c0, c1, targets[c0 - 1:c1])
        for all_, new in zip(counts, got):
            all_.extend(new)
        if min(got[1]) == 0:
            break
    wall = (time.perf_counter() - t0) * 1e3
    _device_pcut_rows(rs, i_iter, i_ion, counts, wall, lambda ip: "(fused loop)", out_stats, out_empty)


def _next_population(rs, be, row, counts, n_prev_global, local_ok, shard):
    """new_pcut (src/cuts.jl:34-98) after a pcut that saved row.n_saved particles in all, counts[r] of them on rank r: the next
    population in one of the four ways of the module docstring -> its shard (first, stride, gidx, n_local)."""
    import torch
    comm, i_mult = rs.comm, row.i_mult
    first, stride, gidx, n_local = shard
    n_use_global = row.n_saved * i_mult
    if rs.multi and row.n_saved == n_prev_global and i_mult == 1:
        # everybody was saved and nobody is replicated (the first pcuts of a species): the saved particles' positions
        # in the global order ARE their indices, so every rank's children keep the global indices their parents had
        # -- no index column to exchange, no particle to move; the shard description (first / stride / gidx) stands
        be.new_pcut(1)
        row.split = "identity"
    elif not rs.multi:
        be.new_pcut(i_mult)                     # one process: the shard stays 0, 1, 2, ...
        n_local = n_use_global
    elif local_ok:
        # every rank splits its own saved particles; the index column alone goes round
        g_loc = be.saved_gidx()                                  # ascending, counts[rank] entries
        cap = max(max(counts), 1)
        # (padded with the largest integer: every row of the gathered table stays sorted; for each of my saved particles a
        # searchsorted per peer row counts that rank's saved particles below it.  One row at a time, accumulated in place:
        # the working set is O(n) -- round 3 searched all rows at once through an expanded [W, n] key matrix and an int64
        # [W, n] result, 0.5 + 0.8 GB per rank and pcut at config[3]'s 1.25e7 particles per GPU)
        # (the column travels as int32 while every index fits: half the bytes on the wire and in the search -- 4 B per saved
        # particle per peer, 32 MB per rank and pcut at 10^6 particles per GPU on 8 GPUs)
        idt = torch.int32 if n_prev_global < 2 ** 31 - 1 else torch.int64
        g_key = g_loc.to(idt)
        pad = torch.full((cap,), torch.iinfo(idt).max, dtype=idt, device=g_loc.device)
        pad[:g_key.numel()] = g_key
        g_all = comm.all_gather_rows(pad)                             # [W, cap]
        pos = torch.zeros(g_key.numel(), dtype=torch.int64, device=g_loc.device)
        for w in range(g_all.shape[0]):
            pos += torch.searchsorted(g_all[w], g_key)
        gidx = (pos[:, None] * i_mult + torch.arange(i_mult, dtype=torch.int64, device=g_loc.device)[None, :]).reshape(-1).contiguous()
        be.new_pcut(i_mult)
        n_local = counts[comm.rank] * i_mult
    else:
        # all ranks see all parents (sorted by global index); rank r builds elements r, r+W, ... of the split
        g, f64, meta = be.export_saved(max(max(counts), 1))
        g = comm.all_gather_cols(g, counts)
        f64 = comm.all_gather_cols(f64, counts)
        meta = comm.all_gather_cols(meta, counts)
        order = torch.argsort(g, stable=True)
        f64 = f64.index_select(1, order).contiguous()
        meta = meta.index_select(0, order).contiguous()
        first, stride, gidx = comm.rank, comm.world, None
        n_local = (n_use_global - comm.rank + comm.world - 1) // comm.world if n_use_global > comm.rank else 0
        be.import_split(f64, meta, row.n_saved, i_mult, first, stride, n_local)
    return first, stride, gidx, n_local


def _pcuts_one_by_one(rs, be, i_iter, i_ion, hook, p_pcut_hi, n_use_global, shard, out_stats):
    """One backend call and one small collective per pcut; the host decides i_mult and builds the next population."""
    comm, long_draws = rs.comm, rs.long_draws
    i_mult_prev = 0                 # (the rule of mcs_run_pcuts_pipelined for the per-pcut loop: see long_imult_max)
    for i_pcut in range(1, rs.n_pcuts + 1):
        t0 = time.perf_counter()
        first, stride, gidx, n_local = shard
        if hook is not None:
            hook(i_iter, i_ion, i_pcut)
        if long_draws:
            be.set_long_draws(int(long_draws) if (i_pcut == 1 or rs.long_imult_max <= 0 or i_mult_prev <= rs.long_imult_max) else 0)
        n_saved_local = be.run_pcut_indexed(i_pcut, gidx) if gidx is not None else be.run_pcut(i_pcut, first, stride)
        gathered = comm.all_gather_ints([n_saved_local, n_local])
        counts = [g[0] for g in gathered]
        n_use_max = max(g[1] for g in gathered)
        n_saved = sum(counts)
        wall = (time.perf_counter() - t0) * 1e3
        # pcut_finalize (src/cuts.jl:100-124)
        i_mult = max(_pcut_target(rs, i_pcut, p_pcut_hi) // n_saved, 1) if n_saved > 0 else 0         # new_pcut, src/cuts.jl:42
        i_mult_prev = i_mult
        last = n_saved == 0 or i_pcut == rs.n_pcuts
        local_ok = not rs.multi or (n_saved > rs.gather_max and max(counts) * comm.world <= rs.skew_max * n_saved)
        row = PcutStat(i_iter, i_ion, i_pcut, n_use_global, n_saved, i_mult, n_use_max,
                       "-" if last else ("local" if local_ok else "gather"), be.last_kernel_ms(), wall)
        out_stats.append(row)
        if rs.verbose and rs.is_root:
            print(f"[iter {i_iter} ion {i_ion} pcut {i_pcut:2d}] n_use={n_use_global} (max local {n_use_max}) "
                  f"n_saved={n_saved} i_mult={i_mult} split={row.split} kernel={be.last_kernel_ms():.2f} ms "
                  f"wall={wall:.1f} ms", flush=True)
        if n_saved == 0:
            break
        # (every global index of the pcut just run is below n_use_global)
        shard = _next_population(rs, be, row, counts, n_use_global, local_ok, shard)
        n_use_global = n_saved * i_mult


def _species_transport(rs, be, i_iter, i_ion, hook, out_stats, out_empty):
    """begin_species .. the last pcut of species i_ion on context `be`; its pcuts go to out_stats / out_empty.  hook: the
    before_pcut of this species (None: the fused loop where it applies)."""
    prob, comm, L, cfg = rs.prob, rs.comm, rs.L, rs.prob.cfg
    sp = cfg.species[i_ion - 1]
    pmax_cutoff = inputs.get_pmax_cutoff(prob.Emax_keV, prob.Emax_per_aa_keV, prob.pmax, sp.aa)
    inj = inputs.init_pop_host(prob, i_ion)
    zz = abs(sp.zz) if cfg.abs_charge else sp.zz
    ewf = 1.0 / cfg.species[-1].density if cfg.species[-1].density != 0 else float("inf")
    be.begin_species(i_iter, i_ion, sp.aa, zz, pmax_cutoff, sp.density, ewf)
    if rs.do_tcuts and not hasattr(be, "tcut_spectra"):
        # (a backend without K12: the base its numpy statement needs, the species' coupled spectra as they stand now)
        rs.tcut_base[id(be)] = L.view(be.read_tallies()[0], "spectra_coupled")[i_ion - 1].copy()
    if rs.detector_window is not None and not hasattr(be, "detector_spectra"):
        # (a backend without K14: the base its numpy statement needs, the detectors' rows as they stand now)
        rs.detector_base[id(be)] = consumers.detector_base(be, len(rs.prob.x_spec))
    if rs.is_root:
        be.set_fluxes(inj.pxx_flux, inj.pxz_flux, inj.energy_flux)
    if rs.multi:
        # (on the bound device tensors in place, otherwise on the host's copy of the buffers)
        f, i = (rs.dev_t[0], None) if rs.dev_t is not None else be.read_tallies()
        if not rs.is_root:   # per-species fills are baselines too
            for name in ("psd", "esc_psd_up", "esc_psd_down"):
                L.view(f, name)[...] = 0.0
        if rs.G_pool is not None:   # ions' donated energy, merged at the previous species end
            L.view(f, "energy_recv_pool")[...] = rs.G_pool
        if rs.dev_t is None:
            be.write_tallies(f, i)

    n_total = inj.n_pts_use
    # the shard: global index of local particle k = first + k * stride, or gidx[k] after a local split
    first, stride = comm.rank, comm.world
    n_local = (n_total - comm.rank + comm.world - 1) // comm.world if n_total > comm.rank else 0
    if stride == 1:
        be.init_pop(inj, 0, n_local, n_total)
    else:
        be.init_pop(inj, first, n_local, n_total, stride)
    p_pcut_hi = inputs.pcut_hi(cfg.EN_PCUT_HI, sp.mass)
    # One rank, no per-pcut hook: the whole pcut loop of the species is queued on the device at once -- n_saved, i_mult and
    # the next population's size are decided there (mcs_run_pcuts_fused), one read-back per species instead of one per pcut.
    fused = rs.fused_pcuts and not rs.multi and hook is None and hasattr(be, "run_pcuts_fused") and rs.n_pcuts >= 1
    # Long histories told apart (long_draws > 0): the next population is ordered non-long before long, which lets a
    # pcut's long histories finish beside the next pcut (mcs_run_pcuts_pipelined; one rank).  A backend without that entry point
    # (the oracle) is told the order (set_long_draws) and runs the ordinary loop: same populations, same streams, same results.
    pipelined = False
    if rs.long_draws:
        if rs.multi:
            raise ValueError("long_draws: the pipelined pcut loop and its population order are single-rank (one process per replica)")
        if not hasattr(be, "run_pcuts_pipelined") and not hasattr(be, "set_long_draws"):
            raise ValueError("long_draws: the backend can neither pipeline the pcuts nor order the population by history length")
        pipelined = hook is None and hasattr(be, "run_pcuts_pipelined") and rs.n_pcuts >= 1 and not getattr(prob.params, "state_fp32", 0)
        if not pipelined:
            if not hasattr(be, "set_long_draws"):
                raise ValueError("long_draws: this configuration runs the per-pcut loop, and the backend cannot order the population there")
            be.set_long_draws(int(rs.long_draws))
    targets = [_pcut_target(rs, ip, p_pcut_hi) for ip in range(1, rs.n_pcuts + 1)]
    if pipelined:
        _pcuts_pipelined(rs, be, i_iter, i_ion, targets, out_stats)
    elif fused:
        _pcuts_fused(rs, be, i_iter, i_ion, targets, out_stats, out_empty)
    else:
        _pcuts_one_by_one(rs, be, i_iter, i_ion, hook, p_pcut_hi, n_total, (first, stride, None, n_local), out_stats)


def _merge_ranks_device(rs, light):
    """Species end over the ranks, in place on the bound tally tensors (RCCL, no host round trip) -> (G_f, G_i, this rank's own step total)."""
    L, comm = rs.L, rs.comm
    rs.backend.sync()          # the bound tensors are complete after mcs_sync (it folds the tally replicas in)
    tf, ti = rs.dev_t
    local = sum(_steps(ti, L.n_grid))
    if not rs.is_root:   # every rank carried a full copy of the received-energy pool
        L.view(tf, "energy_recv_pool").zero_()
    comm.all_reduce_sum_(tf); comm.all_reduce_sum_(ti)
    rs.G_pool = L.view(tf, "energy_transfer_pool").clone()
    if light:
        o_small = L.offsets["esc_psd_up"]
        G_f = np.zeros(L.total)
        G_f[o_small:] = tf[o_small:].cpu().numpy()
        G_i = ti.cpu().numpy()
    else:
        G_f, G_i = tf.cpu().numpy(), ti.cpu().numpy()
    if not rs.is_root:
        tf.zero_(); ti.zero_()
    return G_f, G_i, local


def _merge_ranks_host(rs):
    """The same steps through read_tallies / write_tallies (CPU test backends)."""
    import torch
    L, comm, backend = rs.L, rs.comm, rs.backend
    f, i = backend.read_tallies()
    local = sum(_steps(i, L.n_grid))
    if not rs.is_root:
        L.view(f, "energy_recv_pool")[...] = 0.0
    tf, ti = torch.from_numpy(f), torch.from_numpy(i)
    comm.all_reduce_sum_(tf); comm.all_reduce_sum_(ti)
    G_f, G_i = f.copy(), i.copy()
    rs.G_pool = L.view(G_f, "energy_transfer_pool").copy()
    if rs.is_root:
        backend.write_tallies(G_f, G_i)
    else:
        backend.write_tallies(np.zeros_like(G_f), np.zeros_like(G_i))
    return G_f, G_i, local


def _species_end(rs, k, i_iter, i_ion, before_hook=None):
    """Species i_ion has ended on context k (k > 0: a secondary, already merged into the primary): the tallies of all ranks merged (C1)
    and handed to the host -- rs.G_f / rs.G_i, per_species, local_steps, on_species_end.  before_hook: called once the context is read."""
    L, be = rs.L, rs.ctxs[k]
    last_read = rs.final_full_read and i_iter == rs.last_iter and i_ion == len(rs.prob.cfg.species)
    light = rs.species_tallies == "light" and not last_read
    if rs.multi:
        G_f, G_i, local = _merge_ranks_device(rs, light) if rs.dev_t is not None else _merge_ranks_host(rs)
        seen = sum(_steps(G_i, L.n_grid)) if rs.is_root else 0     # rank 0 carries the merged totals on
    else:
        G_f, G_i = _read_light(be) if light else be.read_tallies()
        if k > 0:
            # species k's own per-species sections (the secondary's) with the running sums of species 1..k (the primary's)
            pf, pi = _read_light(rs.backend)
            for name in RUNNING_F64:
                L.view(G_f, name)[...] = L.view(pf, name)
            G_i[running_i64(L)] = pi[running_i64(L)]
        local = seen = sum(_steps(G_i, L.n_grid))
    rs.local_steps.append((i_iter, i_ion, local - rs.steps_seen))
    rs.steps_seen = seen
    rs.G_f, rs.G_i = G_f, G_i
    rs.per_species.append((i_iter, i_ion, G_f, G_i))      # fresh host arrays: no copy needed
    if rs.ensemble is not None:
        # from the context that holds this species' per-species sections, before it is freed for its next species
        rs.ensemble.add_species(be, i_ion - 1)
    if before_hook is not None:
        before_hook()
    if rs.on_species_end is not None:
        rs.on_species_end(i_iter, i_ion, G_f, G_i)


class _SpeciesScheduler:
    """Which species of an iteration runs on which context, and when (run's species_backends): species 1, every receiver and the last
    species on the primary, each after every earlier species has been merged; any other on a secondary as soon as one is free."""

    def __init__(self, rs, pool, i_iter):
        cfg = rs.prob.cfg
        self.rs, self.pool, self.i_iter, self.n_sp = rs, pool, i_iter, len(cfg.species)
        etf = rs.prob.params.energy_transfer_frac > 0
        self.on_primary = {k: k == 1 or k == self.n_sp or (etf and cfg.species[k - 1].aa < 1) for k in range(1, self.n_sp + 1)}
        self.free = list(range(1, len(rs.ctxs)))      # idle secondaries (context indices)
        self.started = {}                             # i_ion -> (context index, future)
        self.flight = _ChipShare()                    # species in flight on the chip (their launches share it)
        self.next_merge = 1                           # every species before this one is merged into the primary
        self.start_ready(True)

    def _job(self, k, i_ion, overlapped):
        be = self.rs.ctxs[k]
        out_stats, out_empty = [], []
        t0 = time.perf_counter()
        with self.flight.geometry(be, lambda n: _launch_share(be, n), overlapped) as geometry:
            _species_transport(self.rs, be, self.i_iter, i_ion, geometry if overlapped else None, out_stats, out_empty)
            t1 = time.perf_counter()
        return out_stats, out_empty, t0, t1

    def start_ready(self, primary_too):
        started, on_primary = self.started, self.on_primary
        for i_ion in range(1, self.n_sp + 1):
            if i_ion in started:
                continue
            if on_primary[i_ion]:
                if not (primary_too and i_ion == self.next_merge):
                    continue
                k = 0
            elif self.free:
                k = self.free.pop(0)
            else:
                continue
            # the primary's species overlap whatever species of a secondary has not ended yet (or is still to start); one that
            # starts alone keeps the fused loop
            overlapped = k > 0 or any(not on_primary[j] and not (j in started and started[j][1].done()) for j in range(1, self.n_sp + 1))
            self.flight.enter()
            started[i_ion] = (k, self.pool.submit(self._job, k, i_ion, overlapped))

    def result(self, i_ion):
        """Waits for species i_ion -> (context index, stats, empty launches, t_start, t_end); re-raises what it or, meanwhile, another raised."""
        k, fu = self.started[i_ion]
        while not fu.done():
            wait([f for _, f in self.started.values() if not f.done()], return_when=FIRST_COMPLETED)
            for j in sorted(self.started):         # a species that raised: no more merges; the pool's exit waits for the others
                if self.started[j][1].done() and self.started[j][1].exception() is not None:
                    raise self.started[j][1].exception()
        return (k,) + fu.result()

    def merged(self, k):
        """Species next_merge is merged and its context read: a freed secondary takes its next species (the primary waits for the hook)."""
        if k > 0:
            self.free = sorted(self.free + [k])
        self.next_merge += 1
        self.start_ready(False)


def _check_trigger_args(have_ensemble, pass_what, min_iterations, check_every):
    """What run and run_overlapped refuse of a stop rule's arguments before anything runs (the triggers themselves: Ensemble.check_trigger)."""
    if not have_ensemble:
        raise ValueError(f"triggers: they read the error bars of an ensemble; pass {pass_what}")
    if min_iterations < 2:
        raise ValueError(f"triggers: min_iterations {min_iterations} < 2 (there is no standard error below two samples)")
    if check_every < 1:
        raise ValueError(f"triggers: check_every {check_every} < 1")


def _check_photon_triggers(triggers, photons):
    """run and run_overlapped refuse a trigger on a photons slot or on the source slot when no spectra are made."""
    if photons is not None:
        return
    if any(ens.Ensemble.is_photons(t.slot) for t in triggers):
        raise ValueError("triggers: a trigger on a photons slot needs photons= (a consumers.PhotonSetup; no sample would ever arrive)")
    if any(ens.Ensemble.is_photons_all(t.slot) for t in triggers):
        raise ValueError("triggers: a trigger on the source slot needs photons= (a consumers.PhotonSetup; no sample would ever arrive)")


def _add_products(ensemble, prob, backend, ion_fin):
    """The products sample of the iteration whose last species' ion_finalize has just run on `backend` (ensemble.py, "Products"):
    slot n_species - 1, from what the consumers left on the device (a HIP backend) or from ion_fin (the numpy ensemble).  An ensemble
    without a slope window first gets one over all bins."""
    if not ensemble.has_slope_window():
        ensemble.set_slope_window(0, prob.params.num_psd_mom_bins + 1, ens.bin_centres_log10(prob))
    ensemble.add_products(backend, len(prob.cfg.species) - 1, ion_fin)


def _check_triggers(ensemble, triggers, others=()):
    """One summary per slot that has triggers -> [TriggerCheck] in the order of `triggers`.  others: further ensembles, of the other
    contexts of an overlapped run; the summary is then that of `ensemble` merged with them in that order (Ensemble.summarize_merged)."""
    rows = [None] * len(triggers)
    others = list(others)
    for slot in sorted({t.slot for t in triggers}):
        mine = [k for k, t in enumerate(triggers) if t.slot == slot]
        reqs = [triggers[k].request for k in mine]
        # (a slot that has not had two samples yet meets nothing)
        if sum(e.count(slot) for e in [ensemble] + others) < 2:
            got = [None] * len(mine)
        else:
            got = ensemble.summarize_merged(others, slot, reqs) if others else ensemble.summarize(slot, reqs)
        for k, s in zip(mine, got):
            t = triggers[k]
            rows[k] = TriggerCheck(t, s, float("nan"), False, None) if s is None else TriggerCheck(t, s, t.value(s), t.met(s), t.predicted_samples(s))
    return rows


def _species_photons(rs, i_iter, i_ion):
    """The photon spectra at Earth of the species that has just ended on the primary context (run(photons=...)): one ion_finalize of
    ITS tallies (K4; the last species' is the one the iteration's finalize step needs, and is kept for it), its folds and the observed
    shell spectra (consumers.observed_spectra: K5-K7 and K9 on a HIP backend), and one photons sample of the ensemble, which also
    deposits it for the iteration's source sample."""
    ion_fin, obs = _photons_of_species(rs.prob, rs.backend, i_ion, rs.photons, rs.ensemble)
    if i_ion == len(rs.prob.cfg.species):
        rs.last_ion_fin = ion_fin
    rs.photon_spectra[i_ion - 1] = obs


def _photons_of_species(prob, be, i_ion, setup, ensemble):
    """ion_finalize and the observed spectra of species i_ion from the tallies on `be`; with an ensemble, its photons sample and the
    deposit into the pending source sample (ensemble.py, "The source") -> (IonFinal, ObservedSpectra)."""
    ion_fin = consumers.ion_finalize(prob, be, i_ion)
    obs = consumers.observed_spectra(prob, be, i_ion, setup, ion_fin)
    if ensemble is not None:
        ensemble.add_photons(be, i_ion - 1, obs, deposit=True)
    return ion_fin, obs


def _species_escape(rs, be, i_iter, i_ion):
    """The spectra of the particles that left the shock while species i_ion ran on `be` (run(escape=True); K10 on a HIP backend): from
    the escape slabs of ITS tallies, which are per-species sections -- before the context's next begin_species clears them.  With an
    ensemble, one escape sample into Ensemble.escape_slot(i_ion - 1)."""
    if not rs.is_root:
        return
    spec = consumers.escape_spectra(rs.prob, be, i_ion)
    rs.escape.append((i_iter, i_ion, spec))
    if rs.ensemble is not None:
        if not rs.ensemble.has_slope_window():
            rs.ensemble.set_slope_window(0, rs.prob.params.num_psd_mom_bins + 1, ens.bin_centres_log10(rs.prob))
        rs.ensemble.add_escape(be, i_ion - 1, spec)


def _species_angles(rs, be, i_iter, i_ion):
    """The pitch-angle distributions of species i_ion over the run's momentum windows (run(angles=[...]); K11 on a HIP backend), from
    the psd and thermal tallies of the context that transported it -- per-species sections, before the context's next begin_species
    clears them.  With an ensemble, one angles sample into Ensemble.angles_slot(i_ion - 1)."""
    if not rs.is_root:
        return
    dist = consumers.angle_distributions(rs.prob, be, i_ion, rs.angle_windows)
    rs.angles.append((i_iter, i_ion, dist))
    if rs.ensemble is not None:
        if not rs.ensemble.has_angle_windows():
            rs.ensemble.set_angle_windows([w[0] for w in rs.angle_windows], [w[1] for w in rs.angle_windows])
        rs.ensemble.add_angles(be, i_ion - 1, dist)


def _species_tcuts(rs, be, i_iter, i_ion):
    """The time-cut spectra of species i_ion (run(tcuts=True); K12 on a HIP backend): the growth of ITS block of spectra_coupled on
    the context that transported it since that context's begin_species, before the running sums travel to the primary.  With an
    ensemble, one tcuts sample into Ensemble.tcuts_slot(i_ion - 1)."""
    if not rs.is_root:
        return
    spec = consumers.tcut_spectra(rs.prob, be, i_ion, base=rs.tcut_base.get(id(be)))
    rs.tcuts.append((i_iter, i_ion, spec))
    if rs.ensemble is not None:
        rs.ensemble.add_tcuts(be, i_ion - 1, spec)


def _species_detectors(rs, be, i_iter, i_ion):
    """The detector spectra of species i_ion (run(detectors=...); K14 on a HIP backend): the growth of the detectors' rows of
    spectra_sf and spectra_pf on the one context since its begin_species.  With an ensemble, one detectors sample into
    Ensemble.detectors_slot(i_ion - 1)."""
    if not rs.is_root:
        return
    spec = consumers.detector_spectra(rs.prob, be, i_ion, window=rs.detector_window, base=rs.detector_base.get(id(be)))
    rs.detectors.append((i_iter, i_ion, spec))
    if rs.ensemble is not None:
        rs.ensemble.add_detectors(be, i_ion - 1, spec)


def _iteration_profile(rs, be, it_state, sm, i_iter, ion_fin):
    """The profile update of iteration i_iter (run(profile=True); K13 on a HIP backend) from the tallies and pressures of the last
    species on the primary context, before iter_finalize touches `prob`.  With smooth_shocks the q of up to three earlier iterations
    -- what iter_finalize averages with this iteration's -- go with it; with a fixed profile none.  With an ensemble, one profile
    sample."""
    history = None
    if sm.smooth_shocks:
        n_avg = min(i_iter, 4)
        history = list(zip(it_state.q_esc_cal_px[i_iter - n_avg:i_iter - 1], it_state.q_esc_cal_energy[i_iter - n_avg:i_iter - 1]))
    pressures = None if hasattr(be, "profile_update") else (ion_fin.P_psd_par, ion_fin.P_psd_perp, ion_fin.energy_density_psd)
    upd = consumers.profile_update(rs.prob, be, it_state, sm, i_iter, history=history, pressures=pressures)
    rs.profile.append((i_iter, upd))
    if rs.ensemble is not None:
        rs.ensemble.add_profile(be, upd)


def _iteration_species(rs, i_iter, before_pcut):
    """The species of iteration i_iter in order: its transport (here, or with secondaries on the pool's threads as the
    scheduler places it), its merge into the primary if it ran on a secondary, its species end."""
    n_sp = len(rs.prob.cfg.species)
    if len(rs.ctxs) == 1:
        for i_ion in range(1, n_sp + 1):
            _species_transport(rs, rs.backend, i_iter, i_ion, before_pcut, rs.stats, rs.empty_launches)
            _species_end(rs, 0, i_iter, i_ion)
            if rs.do_escape:
                _species_escape(rs, rs.backend, i_iter, i_ion)      # (after the ranks' merge: rank 0 holds the whole slabs)
            if rs.angle_windows is not None:
                _species_angles(rs, rs.backend, i_iter, i_ion)
            if rs.do_tcuts:
                _species_tcuts(rs, rs.backend, i_iter, i_ion)
            if rs.detector_window is not None:
                _species_detectors(rs, rs.backend, i_iter, i_ion)
            if rs.photons is not None:
                _species_photons(rs, i_iter, i_ion)
        return
    with ThreadPoolExecutor(max_workers=len(rs.ctxs)) as pool:   # (leaving the block waits for every thread, also on an exception)
        sched = _SpeciesScheduler(rs, pool, i_iter)
        for i_ion in range(1, n_sp + 1):
            k, out_stats, out_empty, t0, t1 = sched.result(i_ion)
            if rs.do_escape:
                _species_escape(rs, rs.ctxs[k], i_iter, i_ion)      # (the slabs do not travel with the running sums)
            if rs.angle_windows is not None:
                _species_angles(rs, rs.ctxs[k], i_iter, i_ion)      # (nor do the histograms)
            if rs.do_tcuts:
                _species_tcuts(rs, rs.ctxs[k], i_iter, i_ion)       # (the growth is that of the context's own running sums)
            if k > 0 and hasattr(rs.backend, "accumulate_tallies_from") and type(rs.ctxs[k]) is type(rs.backend):
                rs.backend.accumulate_tallies_from(rs.ctxs[k])      # its running sums added to the primary's and cleared
            elif k > 0:
                accumulate_tallies_host(rs.L, rs.backend, rs.ctxs[k])
            rs.stats.extend(out_stats)
            rs.empty_launches.extend(out_empty)
            rs.species_spans.append((i_iter, i_ion, k, t0, t1))
            _species_end(rs, k, i_iter, i_ion, lambda: sched.merged(k))
            sched.start_ready(True)


def run(prob: Problem, backend, comm: Optional[Comm] = None, n_itrs: Optional[int] = None,
        max_pcuts: Optional[int] = None, on_species_end: Optional[Callable] = None,
        verbose: bool = False, gather_max: int = 1 << 17, skew_max: float = 1.1,
        finalize: bool = False, smoothing=None, on_iteration_end: Optional[Callable] = None,
        first_iter: int = 1, iter_state=None, species_tallies: str = "full", final_full_read: bool = True,
        before_pcut: Optional[Callable] = None, tcut_print: bool = False, fused_pcuts: Optional[bool] = None, long_draws: Optional[int] = None,
        long_imult_max: Optional[int] = None, species_backends: Optional[list] = None, fused_chunk: Optional[int] = None,
        ensemble=None, triggers: Optional[list] = None, min_iterations: int = 2, check_every: int = 1, photons=None,
        escape: bool = False, angles=None, tcuts: bool = False, profile: bool = False, detectors=False) -> RunResult:
    """Run `n_itrs` iterations of all species through all pcuts.

    backend protocol: create/begin_iteration/begin_species/set_fluxes/init_pop/
    run_pcut/new_pcut/export_saved/import_split/pop_size/read_tallies/write_tallies/
    last_kernel_ms (HipBackend in hip_backend.py; tests inject the CPU oracle's).
    gather_max / skew_max: see the module docstring (multi-rank new_pcut).
    finalize: close every iteration as the reference does (src/main_loops.jl:324-391): `ion_finalize`'s dN/dp and
    thermo_calcs on the device-resident histograms (K4, consumers.py) and `iter_finalize` (iter_finalize.py).
    smoothing: an iter_finalize.SmoothingConfig; with smooth_shocks the profile tables of `prob` are replaced after
    every iteration (smooth_grid_par) and uploaded again (mcs_set_grid / mcs_set_cuts) -- BASELINE config[2]'s loop.
    Rank 0 computes the update from the merged tallies and broadcasts the tables, so that every rank transports its
    particles through bit-identical profiles.
    species_tallies: "full" -- every species end hands the whole tally buffer to the host (per_species, on_species_end);
    "light" -- only the part behind the three big histograms (fluxes, escape and coupled spectra, pools, scalars: what
    iter_finalize reads) and the int64 tallies; psd / therm_sf / therm_pf stay on the device, where their consumers run (K4),
    and are fetched once, after the last species of the last iteration (RunResult.tallies_f64 is then complete; with
    final_full_read = False not even then -- run_overlapped fetches every context's buffer once, at the very end).
    tcut_print: replicate the in-place rewrite the reference's `tcut_print` makes at the end of every iteration when time-cut
    tracking is on (src/io.jl:28-45, src/main_loops.jl:383-389): weight_coupled floored, every coupled spectrum normalised
    to a total of 1 and floored -- on the merged tallies, written back to the device (rank 0), so that the next iteration
    accumulates on top of it exactly as the reference does.  Off by default: the tallies then stay plain sums over the
    iterations, which is what the parity fixtures and the overlapped run compare.
    before_pcut(i_iter, i_ion, i_pcut): called before every transport launch (run_overlapped sets the launch geometry there).
    first_iter / iter_state: run iterations first_iter .. first_iter + n_itrs - 1 (the iteration number enters the
    RNG keys and indexes the per-iteration tallies), carrying the iter_finalize state of an earlier call
    (RunResult.iter_state) -- lets a caller step through the loop one iteration at a time.
    species_backends: further contexts of the same `prob` (created by the caller: each costs its own device memory) on which the
    species of an iteration that depend on nothing run beside the others.  A species depends on every earlier one when it is a
    receiver -- aa < 1 with energy_transfer_frac > 0: its begin_species copies what the earlier species deposited (include/mcs.h,
    mcs_begin_species) -- and on nothing otherwise.  `backend` is the primary context: begin_iteration runs there only, and it holds
    the iteration's running sums (the table beside mcs_tally_layout).  Species 1, every receiver and the last species run on the
    primary, each after every earlier species has been merged into it; any other species runs on a secondary as soon as one is
    free.  Species end in any order and are merged into the primary in species order (mcs_accumulate_tallies, or
    accumulate_tallies_host); a secondary takes its next species only after its merge.  Species that run side by side take the
    per-pcut loop, and before every launch each gets an equal share of the workgroup slots while others are in flight
    (_launch_share).  What the caller sees is what the one-context run gives: stats, per_species, local_steps and the
    on_species_end calls (calling thread, species order; for a species of a secondary after its merge, with the running sums of
    species 1..k and species k's own per-species sections) are in species order, and what the hook writes back through
    `backend.write_tallies` is what the later species start from.  RunResult.species_spans says what overlapped.  None or []:
    the one-context loop.  Single process without a communicator, no long_draws and no before_pcut.
    fused_pcuts, fused_chunk, long_draws, long_imult_max: how the driver walks a species' pcuts; these arguments are the supported way
    to set them.  fused_pcuts: one rank without a per-pcut hook queues the pcuts on the device in calls of fused_chunk pcuts
    (mcs_run_pcuts_fused), False: one mcs_run_pcut + mcs_new_pcut per pcut.  long_draws > 0: histories of at least that many random
    draws finish beside the next pcut (mcs_run_pcuts_pipelined), in pcuts whose predecessor split by at most long_imult_max (<= 0: in
    every pcut).  An argument left out (None) takes the default an environment variable gives, else the built-in one: MCS_FUSED_PCUTS
    (off iff "0"; True), MCS_FUSED_CHUNK (12), MCS_LONG_DRAWS (0; not read by a multi-rank run), MCS_LONG_IMULT_MAX (8).  The values used
    are in RunResult.options, beside the run options of the backend's context (HipBackend.options()).
    ensemble: an ensemble.Ensemble (Ensemble.for_backend(backend, number of species)) that takes one sample per species end -- slot
    i_ion - 1, from the context that holds the species' per-species sections, after a secondary context's merge -- and one per
    iteration end (the growth of the never-reset tallies since begin_iteration, the rest as it stands): per-cell mean and standard
    error over the iterations, which are independent realisations while the profile is fixed (ensemble.py; on a HIP backend the
    histograms stay on the device).  Not with tcut_print (the in-place rewrite makes the coupled spectra no longer sums), not with
    smooth_shocks (the iterations then depend on each other), not with an enabled communicator: the multi-rank case is left out.
    triggers: a list of ensemble.Trigger on parts of `ensemble`'s slots: the run ends once their error bars are small enough.  After
    the ensemble has taken the iteration sample of iteration i, when done = i - first_iter + 1 >= min_iterations and done -
    min_iterations is a multiple of check_every, every slot that has triggers is summarised once (Ensemble.summarize: on a HIP backend
    one reduction on the device, a few hundred bytes to the host) and the loop ends when every trigger is met.  n_itrs stays the cap
    (the per-iteration tallies px_esc_feb / energy_esc_feb are sized by the problem's).  A run that stops after iteration k has done
    exactly what the same call with n_itrs = k - first_iter + 1 does: same tallies, same per_species, same ensemble (with
    species_tallies = "light" the buffers of the last species end are fetched whole once the run has stopped, as they are at the last
    species end of a run that knew its length; on_species_end has seen that species end without the histograms).
    RunResult.convergence holds the checks, stopped_at and satisfied; predicted_samples in a check is a report, nothing acts on it.
    Refused: triggers without ensemble, min_iterations < 2 (no error bar below two samples), check_every < 1, a trigger whose slot or
    part the ensemble does not have, a trigger on a products slot without finalize.  None or []: no check, RunResult.convergence is None.
    With finalize and ensemble, the ensemble also takes one PRODUCTS sample per iteration, right after the last species' ion_finalize,
    into the products slot of species slot n_species - 1 (ensemble.py, "Products": dN/dp in the three frames, pressures, energy
    density, spectral slope; Ensemble.products_slot).  An ensemble without a slope window first gets one over all bins; set a
    narrower one before the run (Ensemble.set_slope_window, ensemble.slope_window).  Triggers may name its parts, with
    bins=(l_lo, l_hi) for a momentum window of one zone.
    photons: a consumers.PhotonSetup (photon shells, distance, redshift): at every species end, on the context that ran it, one
    ion_finalize of that species (the last species' is the one the finalize step uses: it is not run twice) and
    consumers.observed_spectra -- the species' emission folds and the spectra an observer sees per photon shell, on the device with a
    HIP backend (K9).  RunResult.photons holds the last iteration's ObservedSpectra, one per species.  With ensemble, one PHOTONS sample
    per species and iteration goes into Ensemble.photons_slot(i_ion - 1) (ensemble.py, "Photons"); an ensemble without a photon layout
    first gets consumers.stock_photon_layout(photons.n_shells); triggers may name its parts (zones= shell rows, bins= an energy window
    of one row).  Refused: a trigger on a photons slot without photons=, photons with species_backends, with an enabled communicator,
    or without finalize.  The spectrum an observer sees is the sum over species, and the species of an iteration are correlated (one
    profile, one energy-transfer pool), so its error bars do not follow from the species': every species' sample is also deposited
    into a pending vector (Ensemble.add_photons(deposit=True)), and after the last species of an iteration, before the iteration
    sample, the ensemble takes that vector as one SOURCE sample into Ensemble.photons_all_slot (ensemble.py, "The source"; same parts,
    zones= and bins= as a photons slot).  Deposits left by an iteration that raised are dropped at the top of the next.  Triggers may
    name the source slot; without photons= they are refused like triggers on a photons slot.
    escape: after every species' last pcut, on the context that transported it, consumers.escape_spectra: dN/dp of the particles that
    left through the upstream free-escape boundary or p_max and through the downstream end, in the shock frame, the plasma frame at
    that boundary and the ISM frame (K10 on a HIP backend).  RunResult.escape holds [(i_iter, i_ion, EscapeSpectra)].  With ensemble,
    one ESCAPE sample per species and iteration goes into Ensemble.escape_slot(i_ion - 1) (ensemble.py, "Escape": dNdp, number,
    slope; an ensemble without a slope window first gets one over all bins); triggers may name its parts, with
    zones=Ensemble.escape_row(door, frame) for one door and frame and bins= for a momentum window of that row.
    Refused: escape without finalize, a trigger on an escape slot without escape.
    angles: [(p_lo, p_hi), ...], up to eight momentum windows in cgs (consumers.momentum_windows).  After every species' last pcut, on
    the context that transported it, consumers.angle_distributions: the pitch-angle distribution of every grid zone over every window
    in the shock frame, the zone's plasma frame and the ISM frame, with <mu> and <mu^2> (K11 on a HIP backend).  RunResult.angles holds
    [(i_iter, i_ion, AngleDistributions)].  With ensemble, one ANGLES sample per species and iteration goes into
    Ensemble.angles_slot(i_ion - 1) (ensemble.py, "Angles": dist, number, mean_mu, mean_mu2; an ensemble without angle windows first
    gets the run's); triggers may name its parts, with zones=ensemble.angles_row(frame, zone, window) for one row and bins= for angle
    bins of that dist row.  Refused: angles without finalize, a trigger on an angles slot without angles.  None: nothing of this runs.
    tcuts: after every species' last pcut, on the context that transported it, consumers.tcut_spectra: per time cut the normalised
    spectrum of the weight still coupled at that time, its sum, the mean and three quantiles of log10 p ("p reached by time t") and
    their slopes against log10 t (K12 on a HIP backend; on another backend the numpy statement of the same rules).  It is what the
    tcut_print rewrite published, made from the species' own growth of spectra_coupled, so the tallies stay sums and an ensemble may
    sample it.  RunResult.tcuts holds [(i_iter, i_ion, TcutSpectra)].  With ensemble, one TCUTS sample per species and iteration goes
    into Ensemble.tcuts_slot(i_ion - 1) (ensemble.py, "Tcuts").  Refused: tcuts without finalize, on a problem without time cuts,
    together with tcut_print, with a communicator, a trigger on a tcuts slot without tcuts.  False: no new call is made.
    profile: in every iteration's finalize step, on the primary context, after the last species' ion_finalize and before the products
    sample, consumers.profile_update: the shock profile that smooth_grid_par WOULD write from this iteration's fluxes and pressures,
    with its intermediate rows (K13 on a HIP backend; on another backend the numpy statement of the same rules).  Nothing is applied:
    the host iter_finalize and what it writes into `prob` are unchanged.  RunResult.profile holds [(i_iter, ProfileUpdate)].  With
    smoothing= and smooth_shocks it is handed the q of the earlier iterations that iter_finalize averages; in a run with a fixed
    profile none, so that its samples stay independent, and with ensemble one PROFILE sample per iteration goes into
    Ensemble.profile_slot (ensemble.py, "Profile"; ensemble.profile_consistency reads it).  Refused: profile without finalize, with
    a communicator, a trigger on the profile slot without profile.  False: no new call is made.
    detectors: True, or a slope window (l_lo, l_hi) over the momentum bins (True: all bins).  After every species' last pcut,
    consumers.detector_spectra: per frame and XSPEC detector the normalised spectrum of what crossed it, its dN/dp, sum, mean and three
    quantiles of log10 p and its spectral slope, and per momentum bin the gradient of log10 of the growth over the upstream detectors
    in units of 1/rg0 -- ln 10 times it is u0 / D(p), the inverse e-fold length of the precursor (K14 on a HIP backend; on another
    backend the numpy statement of the same rules, with the base kept here).  RunResult.detectors holds [(i_iter, i_ion,
    DetectorSpectra)].  With ensemble, one DETECTORS sample per species and iteration goes into Ensemble.detectors_slot(i_ion - 1)
    (ensemble.py, "Detectors").  Refused: detectors without finalize, on a problem with no XSPEC, with a communicator, with
    species_backends (see the message), a trigger on a detectors slot without detectors.  False: no new call is made.
    """
    import torch
    comm = comm or Comm(False)
    cfg, P, L = prob.cfg, prob.params, backend.layout
    n_itrs = n_itrs if n_itrs is not None else cfg.num_iterations
    multi = comm.enabled          # (a forced one-rank group runs the multi-rank path too: bench.py MCS_BENCH_FORCE_COMM)
    if long_draws is None:
        long_draws = int(os.environ.get("MCS_LONG_DRAWS", "0")) if not multi else 0
    if long_imult_max is None:
        long_imult_max = int(os.environ.get("MCS_LONG_IMULT_MAX", "8"))
    if fused_pcuts is None:
        fused_pcuts = os.environ.get("MCS_FUSED_PCUTS", "1") != "0"
    if fused_chunk is None:
        fused_chunk = int(os.environ.get("MCS_FUSED_CHUNK", "12"))
    fused_chunk = max(1, int(fused_chunk))
    options = dict(backend.options()) if hasattr(backend, "options") else {}
    options.update(fused_pcuts=bool(fused_pcuts), fused_chunk=fused_chunk, long_draws=int(long_draws), long_imult_max=int(long_imult_max))
    secondaries = list(species_backends or [])
    # The state of the run, shared by the steps above.  dev_t: live device tensors of the tallies (HIP backend with torch_tallies):
    # the multi-GPU merge then runs in place on the device; otherwise (CPU test backends) through read_tallies / write_tallies.
    # G_f / G_i: the merged tallies of the latest species end; G_pool: its merged energy_transfer_pool (multi-rank).
    # rank > 0 keeps only its local partial sums: everything it contributes is a delta.
    rs = types.SimpleNamespace(
        prob=prob, L=L, backend=backend, ctxs=[backend] + secondaries, comm=comm, is_root=comm.rank == 0, multi=multi,
        dev_t=backend.tally_tensors() if (multi and hasattr(backend, "tally_tensors")) else None,
        n_pcuts=len(prob.pcuts) if max_pcuts is None else min(max_pcuts, len(prob.pcuts)), last_iter=first_iter + n_itrs - 1,
        verbose=verbose, gather_max=gather_max, skew_max=skew_max, fused_pcuts=fused_pcuts, fused_chunk=fused_chunk,
        long_draws=long_draws, long_imult_max=long_imult_max, species_tallies=species_tallies, final_full_read=final_full_read, on_species_end=on_species_end,
        photons=photons, photon_spectra=[None] * len(cfg.species), last_ion_fin=None, do_escape=bool(escape), escape=[],
        angle_windows=None, angles=[], do_tcuts=bool(tcuts), tcuts=[], tcut_base={}, profile=[],
        detector_window=None, detectors=[], detector_base={},
        G_f=None, G_i=None, G_pool=None, stats=[], per_species=[], local_steps=[], empty_launches=[], species_spans=[], iter_finals=[])
    # the step counters are never reset: this rank's running total.  A context that has run before (run() called again with
    # first_iter / iter_state, the documented way to step through the loop) starts from what its counters hold now.
    # (the two counter words only: run_overlapped calls run() once per iteration)
    rs.steps_seen = sum(_steps(rs.dev_t[1] if rs.dev_t is not None else _read_counters(backend), P.n_grid))
    rs.ensemble = ensemble
    if ensemble is not None:
        if tcut_print:
            raise ValueError("ensemble: not with tcut_print (its in-place rewrite makes the coupled spectra no longer sums over the iterations)")
        if smoothing is not None and smoothing.smooth_shocks:
            raise ValueError("ensemble: not with smooth_shocks (the iterations of a run with a changing profile are not independent)")
        if comm.enabled:
            raise ValueError("ensemble: one process without a communicator (the multi-rank case is left out)")
        if ensemble.n_species < len(cfg.species):
            raise ValueError(f"ensemble: {ensemble.n_species} species slots for {len(cfg.species)} species")
    triggers = list(triggers or [])
    _check_photon_triggers(triggers, photons)
    if photons is not None:
        if secondaries:
            raise ValueError("photons: not with species_backends (the spectra are made on the context that ran the species, one at a time)")
        if comm.enabled:
            raise ValueError("photons: one process without a communicator (the multi-rank case is left out)")
        if not (finalize or smoothing is not None):
            raise ValueError("photons: needs finalize=True (the spectra are made from ion_finalize's dN/dp)")
        if ensemble is not None and ensemble.photon_layout is None:
            ensemble.set_photon_layout(consumers.stock_photon_layout(photons.n_shells))
    if angles is not None:
        if not (finalize or smoothing is not None):
            raise ValueError("angles: needs finalize=True (the pitch-angle distributions belong to the iteration's finalize step)")
        rs.angle_windows = consumers.momentum_windows(prob, angles)
        if ensemble is not None and not ensemble.has_angle_windows():      # (before the triggers are held against the ensemble's parts)
            ensemble.set_angle_windows([w[0] for w in rs.angle_windows], [w[1] for w in rs.angle_windows])
    elif any(ens.Ensemble.is_angles(t.slot) for t in triggers):
        raise ValueError("triggers: a trigger on an angles slot needs angles=[...] (no sample would ever arrive)")
    if tcuts:
        if not (finalize or smoothing is not None):
            raise ValueError("tcuts: needs finalize=True (the time-cut spectra belong to the iteration's finalize step)")
        if not P.do_tcuts or len(prob.tcuts) < 1:
            raise ValueError("tcuts: the problem tracks no time cuts")
        if tcut_print:
            raise ValueError("tcuts: not with tcut_print (its in-place rewrite is what the time-cut spectra replace)")
        if comm.enabled:
            raise ValueError("tcuts: one process without a communicator (the multi-rank case is left out)")
        if ensemble is not None:      # (before the triggers are held against the ensemble's parts)
            ensemble.expect_tcuts(len(prob.tcuts))
    elif any(ens.Ensemble.is_tcuts(t.slot) for t in triggers):
        raise ValueError("triggers: a trigger on a tcuts slot needs tcuts=True (no sample would ever arrive)")
    if detectors is not False and detectors is not None:
        if not (finalize or smoothing is not None):
            raise ValueError("detectors: needs finalize=True (the detector spectra belong to the iteration's finalize step)")
        if len(prob.x_spec) < 1:
            raise ValueError("detectors: the problem has no detector (XSPEC)")
        if comm.enabled:
            raise ValueError("detectors: one process without a communicator (the multi-rank case is left out)")
        if species_backends:
            raise ValueError("detectors: one context only (no species_backends): spectra_sf and spectra_pf are shared by all species, so "
                             "accumulate_tallies would add a secondary's species into the primary's rows while another species may be current "
                             "there, and that species' growth over its base would include it")
        rs.detector_window = consumers.check_detector_window(P.num_psd_mom_bins, None if detectors is True else detectors)
        if ensemble is not None:      # (before the triggers are held against the ensemble's parts)
            ensemble.expect_detectors((len(prob.x_spec), rs.detector_window[0], rs.detector_window[1], np.float64(prob.rg0).tobytes(),
                                       np.ascontiguousarray(prob.x_spec, dtype=np.float64).tobytes()))
    elif any(ens.Ensemble.is_detectors(t.slot) for t in triggers):
        raise ValueError("triggers: a trigger on a detectors slot needs detectors=True (no sample would ever arrive)")
    if profile:
        if not (finalize or smoothing is not None):
            raise ValueError("profile: needs finalize=True (the profile update belongs to the iteration's finalize step)")
        if comm.enabled:
            raise ValueError("profile: one process without a communicator (the multi-rank case is left out)")
    elif any(ens.Ensemble.is_profile(t.slot) for t in triggers):
        raise ValueError("triggers: a trigger on the profile slot needs profile=True (no sample would ever arrive)")
    if triggers:
        _check_trigger_args(ensemble is not None, "ensemble=", min_iterations, check_every)
        for t in triggers:
            ensemble.check_trigger(t)
    checks, stopped_at, satisfied = [], first_iter + n_itrs - 1, False
    if secondaries:
        if comm.enabled:
            raise ValueError("species_backends: one process without a communicator (the species' merges are not collectives)")
        if long_draws:
            raise ValueError("species_backends: not with long_draws (the pipelined pcut loop takes the whole chip)")
        if before_pcut is not None:
            raise ValueError("species_backends: the per-pcut hook sets the launch geometry of overlapping species; no before_pcut")
        if len({id(be) for be in [backend] + secondaries}) != len(secondaries) + 1:
            raise ValueError("species_backends: every context must be a different one, and none the primary")
        for be in secondaries:
            Lb = be.layout
            if Lb.total != L.total or Lb.n_i64 != L.n_i64 or Lb.offsets != L.offsets:
                raise ValueError("species_backends: a secondary context's tally layout differs from the primary's")
            if getattr(be, "device", None) != getattr(backend, "device", None):
                raise ValueError("species_backends: every context must be on the primary's device")
    finalize = finalize or smoothing is not None
    if escape and not finalize:
        raise ValueError("escape: needs finalize=True (the escape spectra belong to the iteration's finalize step)")
    if not escape and any(ens.Ensemble.is_escape(t.slot) for t in triggers):
        raise ValueError("triggers: a trigger on an escape slot needs escape=True (no sample would ever arrive)")
    if not finalize and any(ens.Ensemble.is_products(t.slot) for t in triggers):
        raise ValueError("triggers: a trigger on a products slot needs finalize=True (ion_finalize makes the products; no sample would ever arrive)")
    it_state = None
    if finalize:
        sm = smoothing if smoothing is not None else itf.SmoothingConfig(smooth_shocks=False)
        it_state = iter_state if iter_state is not None else itf.IterState.create(prob, sm, P.n_itrs)

    for be in secondaries:          # (a context reused from an earlier call must add nothing stale)
        _zero_running_sums(L, be)
    for i_iter in range(first_iter, first_iter + n_itrs):
        backend.begin_iteration(i_iter)
        if ensemble is not None:
            ensemble.begin_iteration(backend)
            if photons is not None:
                ensemble.drop_pending_photons()      # (an iteration that raised after a deposit must not reach into this one)
        if multi and not rs.is_root:
            if rs.dev_t is not None:
                rs.dev_t[0].zero_()
            else:
                f, i = backend.read_tallies()
                f[:] = 0.0
                backend.write_tallies(f, i)
        _iteration_species(rs, i_iter, before_pcut)
        if photons is not None and ensemble is not None:
            ensemble.add_photons_all()               # the source sample: the sum of the species' spectra of this iteration
        if finalize:
            # ion_finalize of the last species (quirk Q2: only its fluxes and pressures reach iter_finalize) and
            # iter_finalize, on rank 0, whose device buffers hold the merged tallies
            changed = False
            if rs.is_root:
                # (with photons= the last species end has made it already)
                ion_fin = rs.last_ion_fin if photons is not None else consumers.ion_finalize(prob, backend, len(cfg.species))
                if profile:      # (before the products sample, which takes the pressures ion_finalize left on the device)
                    _iteration_profile(rs, backend, it_state, sm, i_iter, ion_fin)
                if ensemble is not None:
                    _add_products(ensemble, prob, backend, ion_fin)
                fin = itf.iter_finalize(prob, it_state, sm, i_iter, rs.G_f, L, ion_fin.P_psd_par, ion_fin.P_psd_perp, ion_fin.energy_density_psd)
                rs.iter_finals.append((i_iter, fin, ion_fin))
                changed = fin.profile_changed
            if multi and sm.smooth_shocks:
                tabs = torch.from_numpy(np.stack([prob.ux, prob.gam_sf, prob.utot, prob.beta_ef, prob.gam_ef, prob.btot]))
                dev = comm.device if comm.dist.get_backend() == "nccl" else None
                tabs = tabs.to(dev) if dev is not None else tabs
                comm.dist.broadcast(tabs, src=0)
                tabs = tabs.cpu().numpy()
                for k, name in enumerate(("ux", "gam_sf", "utot", "beta_ef", "gam_ef", "btot")):
                    getattr(prob, name)[:] = tabs[k]
                changed = True
            if changed:
                itf.populate_eps_target(prob)        # src/main_loops.jl:76-81, top of the next iteration
                for be in rs.ctxs:
                    be.set_grid(prob)
                    be.set_cuts(prob)
        if tcut_print and P.do_tcuts:
            # (after iter_finalize, as at src/main_loops.jl:363-389; G_f is the merged buffer of the last species, which holds the
            # coupled arrays of every species -- they are per-ion slices of one array).  The rewrite is applied to a COPY of the
            # buffer -- the entries already handed out in per_species / on_species_end stay the raw sums -- and on every rank, so
            # that all ranks return the same RunResult; only the root writes the device buffer.
            rs.G_f = rs.G_f.copy()
            wc, sc = L.view(rs.G_f, "weight_coupled"), L.view(rs.G_f, "spectra_coupled")
            itf.tcut_print(wc, sc, len(prob.tcuts), P.num_psd_mom_bins)
            if rs.is_root:
                backend.write_tally("weight_coupled", wc)
                backend.write_tally("spectra_coupled", sc)
        if ensemble is not None:
            ensemble.add_iteration(backend)
        done = i_iter - first_iter + 1
        if triggers and done >= min_iterations and (done - min_iterations) % check_every == 0:
            rows = _check_triggers(ensemble, triggers)
            checks.append((i_iter, rows))
            satisfied = all(row.met for row in rows)
        if on_iteration_end is not None:
            on_iteration_end(i_iter)
        if satisfied:
            stopped_at = i_iter
            break

    if satisfied and stopped_at < rs.last_iter and species_tallies == "light" and final_full_read:
        # the last species end did not know it was the last: its whole buffers now, as a run of this length hands them back
        rs.G_f, rs.G_i = backend.read_tallies()
        rs.per_species[-1] = rs.per_species[-1][:2] + (rs.G_f, rs.G_i)
    return RunResult(rs.G_f, rs.G_i, rs.per_species, rs.stats, *_steps(rs.G_i, P.n_grid), rs.iter_finals, it_state,
                     rs.local_steps, rs.empty_launches, rs.species_spans, options, ensemble,
                     Convergence(checks, stopped_at, satisfied) if triggers else None,
                     list(rs.photon_spectra) if photons is not None else None, rs.escape if escape else None,
                     tcuts=rs.tcuts if tcuts else None, profile=rs.profile if profile else None,
                     detectors=rs.detectors if rs.detector_window is not None else None,
                     angles=rs.angles if angles is not None else None)


# The never-reset tallies of the reference (esc_flux, esc_*_eff, spectra_coupled, spectra_sf / _pf accumulate over
# the iterations of a run; px_esc_feb / energy_esc_feb are indexed by iteration): sums over iterations, hence over contexts.
ACCUMULATED_OVER_ITERATIONS = ("esc_flux", "px_esc_feb", "energy_esc_feb", "esc_energy_eff", "esc_num_eff", "spectra_coupled",
                               "spectra_sf", "spectra_pf")


def run_overlapped(prob: Problem, backends, n_itrs: Optional[int] = None, max_pcuts: Optional[int] = None,
                   on_iteration_end: Optional[Callable] = None, first_iter: int = 1,
                   blocks_per_launch: Optional[int] = None, ensemble: bool = False, triggers: Optional[list] = None,
                   min_iterations: int = 2, check_every: int = 1, photons=None, escape: bool = False, angles=None,
                   tcuts: bool = False, profile: bool = False, detectors=False) -> RunResult:
    """The iterations of a run with a FIXED shock profile (smooth-shocks = false -- the stock mc_in.toml, BASELINE
    config[1]) are independent Monte-Carlo realisations: nothing an iteration computes enters the next one's transport
    (src/main_loops.jl:52-121: every tally the transport reads is reset at the top; the RNG keys carry i_iter).  Their
    launches can therefore share the GPU: len(backends) iterations are in flight at a time, each on its own context and
    HIP stream, driven by its own host thread; while one iteration's launch waits for its longest histories (the per-pcut
    tail, 40 % of an iteration at 10^6 particles) the blocks of the other's become resident on the CUs it has freed.
    Per-iteration results are those of run(): same keys, same populations; iter_finalize runs on the host in iteration
    order.  The tallies the reference never resets are sums over iterations and are merged over the contexts at the end.
    blocks_per_launch: workgroups of a K1 launch while iterations overlap; default 2 x #CU / len(backends), i.e. with two
    contexts ONE workgroup per CU each: the two launches are then resident side by side from the start (a CU holds two
    workgroups), each SIMD carries one wave of either, and a wave whose neighbour is in its launch's tail issues at the
    lone-wave rate -- measured 254 ms per iteration against 275 with full-chip launches, which let the other launch in only
    as whole workgroups retire (tools/gpu_concurrent.py).
    Single process only (no communicator): collectives issued from two threads would need an order.
    triggers: a list of ensemble.Trigger, the stop rule of run(triggers=...) for this path; needs ensemble=True.  Without triggers every
    iteration is submitted up front and the contexts run free of one another.  With triggers the run proceeds in ROUNDS of
    K = len(backends) iterations (the last one shorter when n_itrs, which stays the cap, is no multiple of K): iteration
    first_iter + r K + k runs on context k as always, and a round's iterations are all consumed, in iteration order, before the next
    round is submitted.  At the end of a round with `done` iterations finished a check is due at the first round end with
    done >= min_iterations and then at every round end with done - (done at the last check) >= check_every; with K = 1 that is run's
    schedule.  A check makes one Ensemble.summarize_merged per slot that has triggers over the contexts' ensembles in context order:
    the summary of their merge, reduced on the device straight from the K accumulators, none of which is changed (there is no
    scratch accumulator to merge into).  When every trigger is met no further round starts, and the run ends as a run of that length:
    the never-reset tallies summed over the contexts, the ensembles merged in context order into the first, the finalize statistics
    over the iterations that ran.  A run that stops after k iterations hands back what run_overlapped(n_itrs=k, ensemble=True) on
    fresh contexts hands back.  RunResult.convergence holds the checks (keyed by the round's last iteration), stopped_at (the last
    iteration done) and satisfied.  A round ends at a barrier: its last launches overlap with nothing, which costs a part of what
    overlapping gains -- measured at 10^6 protons with three contexts and one check per round: 237.6 ms per iteration against 236.8
    free-running (profiles/overlapped_stop.txt; small because a fixed profile's iterations take the same time, so that free-running
    contexts stay nearly in step anyway; iterations of unequal length would lose more).  Opt-in.  If anything raises after the
    ensembles were created -- a refused trigger, an iteration, on_iteration_end, a check -- they are destroyed before it propagates.  Refused: triggers without ensemble=True,
    min_iterations < 2, check_every < 1, a trigger whose slot or part the ensembles do not have -- before any iteration runs.
    ensemble: True -- every context feeds an ensemble of its own (ensemble.Ensemble.for_backend; run(ensemble=...)); at the end they
    are merged in context order into the first context's, which RunResult.ensemble hands back: per-cell mean and standard error of
    the tallies over the iterations.  Its finalize_mean / finalize_stderr / finalize_count are the same statistics, on the host, of
    the per-iteration ion_finalize of the last species (ensemble.FINALIZE_NAMES), in iteration order.  Every context's ensemble also
    takes the products sample of run(finalize=True, ensemble=...) right after that ion_finalize, inside the iteration's job, so that
    triggers on a products slot work through the rounds and the merged summary like any other.
    photons: a consumers.PhotonSetup, as in run(photons=...): every iteration's job makes each species' spectra at its species end, on
    the job's context (one ion_finalize per species; the last species' is the one handed to iter_finalize, it is not run a second
    time), and with ensemble=True feeds that context's ensemble -- one photons sample per species, deposited, and the source sample
    taken inside the job where the products sample is taken.  Rounds, checks and the final merge then cover the photons slots and the
    source slot like every other; an ensemble gets consumers.stock_photon_layout(photons.n_shells).  RunResult.photons holds the
    spectra of the last iteration consumed.  Refused: a trigger on a photons slot or on the source slot without photons=.  None:
    no spectra are made.
    escape: refused -- the escape spectra of run(escape=True) are left out of the overlapped path.
    angles: refused likewise -- the pitch-angle distributions of run(angles=[...]) are left out of the overlapped path.
    tcuts: refused likewise -- the time-cut spectra of run(tcuts=True) are left out of the overlapped path.
    profile: refused likewise -- the profile update of run(profile=True) is left out of the overlapped path.
    detectors: refused likewise -- the detector spectra of run(detectors=True) are left out of the overlapped path."""
    if (detectors is not False and detectors is not None) or any(ens.Ensemble.is_detectors(t.slot) for t in (triggers or [])):
        raise ValueError("detectors: the overlapped run leaves the detector spectra out; use run(finalize=True, detectors=True)")
    if profile or any(ens.Ensemble.is_profile(t.slot) for t in (triggers or [])):
        raise ValueError("profile: the overlapped run leaves the profile update out; use run(finalize=True, profile=True)")
    if tcuts or any(ens.Ensemble.is_tcuts(t.slot) for t in (triggers or [])):
        raise ValueError("tcuts: the overlapped run leaves the time-cut spectra out; use run(finalize=True, tcuts=True)")
    if angles is not None or any(ens.Ensemble.is_angles(t.slot) for t in (triggers or [])):
        raise ValueError("angles: the overlapped run leaves the pitch-angle distributions out; use run(finalize=True, angles=[...])")
    if escape or any(ens.Ensemble.is_escape(t.slot) for t in (triggers or [])):
        raise ValueError("escape: the overlapped run leaves the escape spectra out; use run(finalize=True, escape=True)")
    cfg, P = prob.cfg, prob.params
    n_itrs = n_itrs if n_itrs is not None else cfg.num_iterations
    K = len(backends)
    assert K >= 1
    if blocks_per_launch is None and K > 1 and hasattr(backends[0], "num_cus"):
        blocks_per_launch = max(2 * backends[0].num_cus() // K, 1)
    triggers = list(triggers or [])
    if triggers:
        _check_trigger_args(bool(ensemble), "ensemble=True", min_iterations, check_every)
    _check_photon_triggers(triggers, photons)
    enss = [ens.Ensemble.for_backend(be, len(cfg.species)) for be in backends] if ensemble else [None] * K
    try:
        if photons is not None and ensemble:
            for e in enss:
                e.set_photon_layout(consumers.stock_photon_layout(photons.n_shells))
        for t in triggers:
            enss[0].check_trigger(t)
        return _overlapped_rounds(prob, backends, enss, n_itrs, max_pcuts, on_iteration_end, first_iter, blocks_per_launch, triggers,
                                  min_iterations, check_every, photons)
    except BaseException:       # (a refused trigger, or whatever an iteration, a hook or a check raised: the run's accumulators go with it)
        for e in enss:
            if e is not None:
                e.destroy()
        raise


def _overlapped_rounds(prob, backends, enss, n_itrs, max_pcuts, on_iteration_end, first_iter, blocks_per_launch, triggers, min_iterations,
                       check_every, photons=None) -> RunResult:
    """run_overlapped once its arguments have passed: the rounds, the checks and the end of the run.  enss: one ensemble per context,
    or None each."""
    n_sp = len(prob.cfg.species)
    cfg, P = prob.cfg, prob.params
    K, L = len(backends), backends[0].layout
    ensemble = enss[0] is not None
    sm = itf.SmoothingConfig(smooth_shocks=False)
    st = itf.IterState.create(prob, sm, P.n_itrs)
    locks = [threading.Lock() for _ in backends]
    busy = _ChipShare()                       # iterations in flight

    def one(i_iter):
        k = (i_iter - first_iter) % K
        with locks[k]:                       # a context carries one iteration at a time
            be = backends[k]
            spectra, fins, at_species_end = [None] * n_sp, {}, None
            if photons is not None:
                if enss[k] is not None:
                    enss[k].drop_pending_photons()      # (an iteration that raised after a deposit must not reach into this one)

                def at_species_end(it, i_ion, G_f, G_i):
                    # run(photons=)'s species end, on this context: the spectra, the photons sample and its deposit
                    fins[i_ion], spectra[i_ion - 1] = _photons_of_species(prob, be, i_ion, photons, enss[k])
            busy.enter()
            with busy.geometry(be, lambda n: blocks_per_launch if n > 1 else 0, bool(blocks_per_launch) and K > 1) as geometry:
                # (long_draws=0: the pcuts are not pipelined here -- the other iterations' launches are what fills this one's tails, and
                # the per-pcut hook needs the per-pcut loop; MCS_LONG_DRAWS does not reach this call)
                res = run(prob, be, None, n_itrs=1, max_pcuts=max_pcuts, first_iter=i_iter, species_tallies="light", final_full_read=False,
                          before_pcut=geometry, long_draws=0, ensemble=enss[k], on_species_end=at_species_end)
                # K4, before the context is reused (with photons the last species end has made it already)
                ion_fin = fins[n_sp] if photons is not None else consumers.ion_finalize(prob, be, n_sp)
                if enss[k] is not None:
                    if photons is not None:
                        enss[k].add_photons_all()               # the source sample of this iteration
                    _add_products(enss[k], prob, be, ion_fin)
        return k, res, ion_fin, spectra

    stats, per_species, iter_finals, local_steps = [], [], [], []
    last = {}                                 # context -> its latest result (running totals of the never-reset tallies)
    ng = P.n_grid
    # the step counters are running totals of a context: where each one starts
    total = [sum(_steps(_read_counters(be), ng)) for be in backends]
    its = list(range(first_iter, first_iter + n_itrs))
    # without triggers one "round" of everything; with them rounds of K, each consumed whole before the next is submitted
    rounds = [its[r:r + K] for r in range(0, n_itrs, K)] if triggers else [its]
    checks, satisfied, done, done_at_check = [], False, 0, None
    with ThreadPoolExecutor(max_workers=K) as pool:
        for rnd in rounds:
            futs = [pool.submit(one, i) for i in rnd]
            for i_iter, fu in zip(rnd, futs):      # consumed in iteration order
                k, res, ion_fin, last_spectra = fu.result()
                fin = itf.iter_finalize(prob, st, sm, i_iter, res.tallies_f64, L, ion_fin.P_psd_par, ion_fin.P_psd_perp, ion_fin.energy_density_psd)
                local_steps.append((i_iter, len(cfg.species), res.steps_helix + res.steps_retro - total[k]))
                total[k] = res.steps_helix + res.steps_retro
                last[k] = res
                stats.extend(res.stats); per_species.extend(res.per_species); iter_finals.append((i_iter, fin, ion_fin))
                if on_iteration_end is not None:
                    on_iteration_end(i_iter)
            done += len(rnd)
            if triggers and (done >= min_iterations if done_at_check is None else done - done_at_check >= check_every):
                rows = _check_triggers(enss[0], triggers, enss[1:])
                checks.append((rnd[-1], rows))
                done_at_check = done
                satisfied = all(row.met for row in rows)
                if satisfied:
                    break
    n_done = done
    # the state after the last iteration: its context's buffer, with the never-reset tallies summed over the contexts
    k_last = (n_done - 1) % K
    f, i64 = backends[k_last].read_tallies()              # the only time the three histograms cross to the host
    for k in last:
        if k == k_last:
            continue
        fk, ik = _read_light(backends[k])
        for name in ACCUMULATED_OVER_ITERATIONS:
            L.view(f, name)[...] += L.view(fk, name)
        i64[ng:] += ik[ng:]                   # the event counters are running totals too (num_crossings is per species)
    if ensemble:
        for other in enss[1:]:
            enss[0].merge(other)
            other.destroy()
        for name in ens.FINALIZE_NAMES:
            enss[0].finalize_mean[name], enss[0].finalize_stderr[name], enss[0].finalize_count = ens.stats_over(
                [getattr(ion_fin, name) for _, _, ion_fin in iter_finals])
    return RunResult(f, i64, per_species, stats, *_steps(i64, ng), iter_finals, st, local_steps, ensemble=enss[0],
                     convergence=Convergence(checks, first_iter + n_done - 1, satisfied) if triggers else None,
                     photons=list(last_spectra) if photons is not None else None)
