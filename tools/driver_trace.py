"""What the host driver asks of its backends, as digests: for a list of configurations of driver.run / run_overlapped on the CPU oracle,
one digest per context of the sequence of backend calls (method name + a hash of the arguments, arrays by their bytes) and one of the
RunResult (every list, both tally arrays by their bytes; host times left out).  The driver is deterministic on the oracle, so two
versions of driver.py that ask the same of their backends print the same lines.  usage: python tools/driver_trace.py [part of a configuration's name ...] > trace.txt
`emulate`: the optional methods of the HIP backend the oracle lacks, restated from the oracle's own calls, so that the driver takes its
device-decided pcut loops, the light reads and the launch-geometry hooks without a GPU."""
import contextlib, ctypes, hashlib, io, os, re, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import torch
import _mcs_loader; m = _mcs_loader.load()
import orc


def digest(x, depth=0):
    """A short hash of a call's arguments or of a result: arrays and tensors by their bytes, objects by their fields."""
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    if isinstance(x, np.ndarray):
        return hashlib.sha1(str(x.dtype).encode() + str(x.shape).encode() + np.ascontiguousarray(x).tobytes()).hexdigest()[:12]
    if isinstance(x, ctypes.Structure):
        return hashlib.sha1(bytes(x)).hexdigest()[:12]
    if isinstance(x, (list, tuple)):
        return hashlib.sha1(",".join(digest(v, depth) for v in x).encode()).hexdigest()[:12]
    if isinstance(x, Traced):
        return "ctx"
    if hasattr(x, "__dict__") and depth < 2:
        return digest([(k, digest(v, depth + 1)) for k, v in sorted(vars(x).items()) if not callable(v)], depth)
    return repr(x) if isinstance(x, (int, float, str, bool, type(None), np.integer, np.floating)) else type(x).__name__


def _pcuts(be, first, last, targets, strag):
    """run_pcuts_fused / run_pcuts_pipelined from run_pcut + new_pcut: the counts of every pcut, empty launches after the last one."""
    nu, ns, im, n = [], [], [], be.pop_size()
    for ip, tg in zip(range(first, last + 1), targets):
        s = be.run_pcut(ip, 0) if n else 0
        nu.append(n); ns.append(s); im.append(max(int(tg) // s, 1) if s else 1)
        n = be.new_pcut(im[-1]) if s else 0
    out = (np.array(nu), np.array(ns), np.array(im), np.zeros(len(nu)))
    return out + (np.zeros((len(nu), 2), dtype=np.int64),) if strag else out


EMULATED = {
    "run_pcuts_fused": lambda be, a, b, tg: _pcuts(be, a, b, tg, False),
    "run_pcuts_pipelined": lambda be, a, b, tg, ld, lim=0: _pcuts(be, a, b, tg, True),
    "read_tallies_light": lambda be: be.read_tallies(),
    "read_counters": lambda be: be.read_tallies()[1],
    "set_launch": lambda be, blocks=0, threads=0: None,
    "num_cus": lambda be: 256,
    "k1_blocks_per_cu": lambda be: 2,
    "sync": lambda be: None,
}


class Traced:
    """An OracleBackend behind a __getattr__ proxy that records (method, digest of the arguments) of every call."""

    def __init__(self, prob, emulate=()):
        self._inner = orc.OracleBackend(m.capi, "det", 1)
        self._inner.create(prob)
        self._emulate, self.calls = set(emulate), []
        # "tally_tensors": host tensors kept equal to the oracle's buffers around every call stand in for the bound device tensors
        self._bound = tuple(torch.from_numpy(a) for a in self._inner.read_tallies()) if "tally_tensors" in self._emulate else None

    def __getattr__(self, name):
        if name == "tally_tensors" and self._bound is not None:
            return lambda: self._bound
        if name in EMULATED:
            if name not in self._emulate:
                raise AttributeError(name)
            fn = lambda *a, **k: EMULATED[name](self._inner, *a, **k)
        else:
            fn = getattr(self._inner, name)
            if not callable(fn):
                return fn

        if name in ("num_cus", "k1_blocks_per_cu"):       # (asked only while another launch is in flight: not part of the trace)
            return fn

        def rec(*a, **k):
            # (the geometry of a launch depends on what else is in flight at that moment: the call is recorded, not its arguments)
            self.calls.append(name + ":" + ("" if name == "set_launch" else digest([a, sorted(k.items())])))
            if self._bound is None:
                return fn(*a, **k)
            self._inner.write_tallies(*(t.numpy() for t in self._bound))
            out = fn(*a, **k)
            for t, new in zip(self._bound, self._inner.read_tallies()):
                t.copy_(torch.from_numpy(new))
            return out
        return rec


def result_digest(r, hooks):
    stats = [(s.i_iter, s.i_ion, s.i_pcut, s.n_pts_use, s.n_saved, s.i_mult, s.n_use_max, s.split) for s in r.stats]
    finals = [(it, digest(f), digest(g)) for it, f, g in r.iter_finals]
    spans = [tuple(s[:3]) for s in r.species_spans]
    return digest([r.tallies_f64, r.tallies_i64, [(a, b, digest(f), digest(i)) for a, b, f, i in r.per_species], stats, r.steps_helix,
                   r.steps_retro, finals, r.local_steps, [e[:3] for e in r.empty_launches], spans, hooks]) + f" pcuts={len(stats)} empty={len(r.empty_launches)}"


ME_MP = m.constants.ME / m.constants.MP
S = m.inputs.Species
MIX = dict(species=[S(1.0, 1.0, 1e6, 1.0), S(4.0, 2.0, 1e6, 0.1), S(ME_MP, -1.0, 1e6, 1.2)], energy_transfer_frac=0.1, radiation_losses=True,
           INJFR=[0.7, 1.0, 1.0], b_field_turbulence=1.0, shock_speed=3.0)
ALL = tuple(k for k in EMULATED if k != "sync")
SMOOTH = m.iter_finalize.SmoothingConfig(smooth_shocks=True)


ONLY = sys.argv[1:]


def case(name, cfg_kw=None, n_ctx=1, emulate=(), overlapped=False, comm=False, prior=False, env=None, **kw):
    """One configuration: N = 200 particles, 8 pcuts, 2 iterations unless told otherwise; prints its digests."""
    if ONLY and not any(o in name for o in ONLY):
        return
    prob = m.inputs.build_problem(m.inputs.Config(N_PTS_INJ=200, N_PTS_PCUT=200, N_PTS_PCUT_HI=200, num_iterations=4, **(cfg_kw or {})))
    ctxs = [Traced(prob, emulate) for _ in range(n_ctx)]
    hooks = []
    kw.setdefault("n_itrs", 2); kw.setdefault("max_pcuts", 8)
    if prior:       # iteration 1 and 2 in an earlier call: the second call carries its iter_state on
        kw.update(first_iter=3, iter_state=m.driver.run(prob, ctxs[0], None, n_itrs=2, max_pcuts=8, finalize=True).iter_state, finalize=True)
    out = io.StringIO()
    os.environ.update(env or {})
    with contextlib.redirect_stdout(out):
        if overlapped:
            r = m.driver.run_overlapped(prob, ctxs, on_iteration_end=lambda it: hooks.append(it), **kw)
        else:
            r = m.driver.run(prob, ctxs[0], m.driver.Comm(True) if comm else None, species_backends=ctxs[1:], verbose=True,
                             on_species_end=lambda it, ion, f, i: hooks.append((it, ion, digest(f), digest(i))),
                             on_iteration_end=lambda it: hooks.append(it), **kw)
    for k in env or {}:
        del os.environ[k]
    lines = sorted(re.sub(r"(kernel|wall)=[^ ]+ ms", r"\1=_", ln) for ln in out.getvalue().splitlines())      # (threads print in any order)
    print(f"{name}: result {result_digest(r, hooks)} verbose {digest(lines)} ({len(lines)} lines)")
    for k, be in enumerate(ctxs):
        print(f"    context {k}: {len(be.calls)} calls {digest(be.calls)}")


if __name__ == "__main__":
    case("one species, per-pcut loop (the oracle as it is)")
    case("one species, fused loop", emulate=ALL)
    case("one species, fused loop in chunks of 3 (MCS_FUSED_CHUNK)", emulate=ALL, env={"MCS_FUSED_CHUNK": "3"}, max_pcuts=None)
    case("one species, MCS_FUSED_PCUTS=0, MCS_LONG_DRAWS=4", emulate=ALL, env={"MCS_FUSED_PCUTS": "0", "MCS_LONG_DRAWS": "4"}, before_pcut=lambda *a: None)
    case("fused_pcuts=False", emulate=ALL, fused_pcuts=False)
    case("before_pcut hook", emulate=ALL, before_pcut=lambda *a: None)
    case("long_draws=4, set_long_draws", long_draws=4, long_imult_max=3)
    case("long_draws=4, pipelined loop", emulate=ALL, long_draws=4)
    case("long_draws=300 (some histories are long), set_long_draws", long_draws=300, long_imult_max=3, max_pcuts=None)
    case("mix, long_draws=300, pipelined loop", MIX, emulate=ALL, long_draws=300)
    case("mix, sequential", MIX)
    case("mix, sequential, fused", MIX, emulate=ALL)
    case("mix, one secondary", MIX, n_ctx=2)
    case("mix, two secondaries", MIX, n_ctx=3)
    case("mix, one secondary, launch shares", MIX, n_ctx=2, emulate=ALL, species_tallies="light")
    case("finalize with smoothing", smoothing=SMOOTH)
    case("mix, finalize with smoothing, one secondary", MIX, n_ctx=2, smoothing=SMOOTH)
    case("tcut_print with time cuts (the stock TCUTS)", tcut_print=True)
    case("light tallies, no final full read", emulate=ALL, species_tallies="light", final_full_read=False)
    case("first_iter=3 with a carried iter_state", prior=True)
    case("run_overlapped, two contexts", n_ctx=2, overlapped=True, n_itrs=3)
    case("run_overlapped, two contexts, launch shares", MIX, n_ctx=2, emulate=ALL, overlapped=True, n_itrs=3)
    import torch.distributed as dist
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "store"), rank=0, world_size=1)
        case("one-rank group, gather split", MIX, comm=True, gather_max=1 << 30)
        case("one-rank group, local split", MIX, comm=True, gather_max=0)
        case("one-rank group, smoothing", comm=True, gather_max=0, smoothing=SMOOTH)
        case("one-rank group, bound tally tensors", MIX, emulate=("tally_tensors", "sync"), comm=True, gather_max=0)
        case("one-rank group, bound tally tensors, light", MIX, emulate=("tally_tensors", "sync"), comm=True, species_tallies="light", smoothing=SMOOTH)
        dist.destroy_process_group()
