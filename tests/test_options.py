"""The run options of a context (enum mcs_option of include/mcs.h; the table of csrc/mcs_options.h): what the library says about
them, what mcs_create_with_options / mcs_set_option / mcs_get_option refuse before any device is touched -- the same with and
without a GPU --, and the table's header on its own in a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/native/options_main.cpp; nothing loaded into Python)."""
import ctypes as ct
import os
import subprocess

import pytest

from conftest import ROOT, mcs, make_problem
from test_sanitizers import _runtime

CSRC = os.path.join(ROOT, "montecarloscattering.jl_amd", "csrc")
I64_MAX = 2 ** 63 - 1

# name: (environment variable, built-in default, min, max, when, applies) -- the issue's table, checked against the code the option
# table replaced (the mcs_create of the parent commit: env_int ranges, member initialisers; mcs_set_tail_slicing's 0 .. 2^24)
EXPECTED = {
    "force_general": ("MCS_FORCE_GENERAL", 0, 0, 1, "between launches", "any"),
    "k1_ws": ("MCS_K1_WS", 2, 0, 2, "between launches", "any"),
    "ws_auto_min": ("MCS_WS_AUTO_MIN", 6_000_000, 0, I64_MAX, "between launches", "any"),
    "tail_merge": ("MCS_TAIL_MERGE", 1, 0, 1, "between launches", "any"),
    "park": ("MCS_PARK", 1, 0, 1, "between launches", "any"),
    "tail_ring": ("MCS_TAIL_RING", 1, 0, 1, "between launches", "any"),
    "tail_loop": ("MCS_TAIL_LOOP", 12, 0, 32, "between launches", "any"),
    "refill_min": ("MCS_REFILL_MIN", 12, 1, 48, "between launches", "any"),
    "defer_k": ("MCS_DEFER_K", 8, 1, 40, "between launches", "any"),
    "tail_budget": ("MCS_TAIL_BUDGET", 0, 0, 1 << 24, "between launches", "fp64 state when > 0"),
    "pipe_side_cus": ("MCS_PIPE_SIDE_CUS", 12, 0, 128, "before the first pipelined run", "any"),
    "tally_replicas": ("MCS_TALLY_REPLICAS_OFF", 1, 0, 1, "creation only", "any"),
    "f32_loop": ("MCS_F32_LOOP", 0, 0, 1, "between launches", "fp32 state"),
    "f32_exact": ("MCS_F32_EXACT", 0, 0, 1, "between launches", "fp32 state"),
}


@pytest.fixture(autouse=True)
def _no_mcs_environment(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MCS_")]:
        monkeypatch.delenv(k)


def _err(lib):
    return lib.mcs_last_error().decode()


def _create(lib, prob, options, use_env=0):
    keys = (ct.c_int32 * len(options))(*[k for k, _ in options])
    vals = (ct.c_int64 * len(options))(*[v for _, v in options])
    h = ct.c_void_p(None)
    rc = lib.mcs_create_with_options(ct.byref(prob.params), 0, None, keys, vals, len(options), use_env, ct.byref(h))
    if rc == 0:          # (a machine with a GPU and a list that is allowed)
        lib.mcs_destroy(h)
    return rc


def test_option_table():
    lib = mcs.capi.load_library()
    assert lib.mcs_option_count() == 14
    rows = []
    for key in range(14):
        d = mcs.capi.McsOptionDesc()
        assert lib.mcs_option_describe(key, ct.byref(d)) == 0
        assert d.key == key and d.reserved == 0
        rows.append(d.name.decode())
    assert len(set(rows)) == 14
    table = mcs.capi.option_table()
    assert list(table) == rows and set(table) == set(EXPECTED)
    assert sorted(d["env"] for d in table.values()) == sorted(e[0] for e in EXPECTED.values())
    for name, (env, dflt, lo, hi, when, applies) in EXPECTED.items():
        d = table[name]
        assert (d["env"], d["default"], d["min"], d["max"], d["when"], d["applies"]) == (env, dflt, lo, hi, when, applies), name
        assert d["name"] == name and mcs.capi.option_key(name) == d["key"]
    header = open(os.path.join(ROOT, "include", "mcs.h")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, (env, *_) in EXPECTED.items():
        key_name = "MCS_OPT_" + name.upper()
        assert key_name in header and env in header, key_name
        assert key_name in guide and env in guide, key_name
    d = mcs.capi.McsOptionDesc()
    for key in (-1, 14, 99):
        assert lib.mcs_option_describe(key, ct.byref(d)) != 0
        assert "unknown option key %d" % key in _err(lib)
    assert lib.mcs_option_describe(0, None) != 0 and "null" in _err(lib)
    with pytest.raises(KeyError):
        mcs.capi.option_key("no_such_option")


def test_bad_option_lists_fail_before_the_device():
    """The list is checked before the device is asked for: the same failure, with the same message, with and without a GPU."""
    lib = mcs.capi.load_library()
    K = {name: d["key"] for name, d in mcs.capi.option_table().items()}
    prob = make_problem(64)
    assert _create(lib, prob, [(K["park"], 0), (99, 1)]) != 0
    assert "mcs_create_with_options" in _err(lib) and "unknown option key 99" in _err(lib)
    assert _create(lib, prob, [(K["defer_k"], 99)]) != 0
    assert "defer_k" in _err(lib) and "MCS_OPT_DEFER_K" in _err(lib) and "1..40" in _err(lib) and "99" in _err(lib)
    assert _create(lib, prob, [(K["defer_k"], 0)], use_env=1) != 0 and "1..40" in _err(lib)
    assert _create(lib, prob, [(K["f32_exact"], 1)]) != 0
    assert "f32_exact" in _err(lib) and "fp32" in _err(lib)
    assert _create(lib, prob, [(K["f32_loop"], 0)]) != 0 and "f32_loop" in _err(lib)
    assert _create(lib, prob, [(K["tally_replicas"], 2)]) != 0 and "tally_replicas" in _err(lib) and "0..1" in _err(lib)
    p32 = make_problem(64)
    p32.params.state_fp32 = 1
    assert _create(lib, p32, [(K["tail_budget"], 4)]) != 0
    assert "tail_budget" in _err(lib) and "fp64" in _err(lib)
    # null lists
    h = ct.c_void_p(None)
    assert lib.mcs_create_with_options(ct.byref(prob.params), 0, None, None, None, 2, 0, ct.byref(h)) != 0
    assert "null" in _err(lib) and not h
    # a good list gets as far as the device: it succeeds with a GPU and fails on the missing device without one
    import torch
    rc = _create(lib, prob, [(K["k1_ws"], 1), (K["tally_replicas"], 0)])
    if torch.cuda.is_available():
        assert rc == 0
    else:
        assert rc != 0 and "option" not in _err(lib)


def test_environment_value_out_of_range_is_not_an_error(monkeypatch):
    """What the environment says is never refused: outside the range the default stays, silently -- the call fails, if it does, on
    the missing device only."""
    import torch
    lib = mcs.capi.load_library()
    monkeypatch.setenv("MCS_DEFER_K", "99")
    monkeypatch.setenv("MCS_F32_EXACT", "1")
    rc = _create(lib, make_problem(64), [], use_env=1)
    if torch.cuda.is_available():
        assert rc == 0
    else:
        assert rc != 0 and "option" not in _err(lib) and "defer_k" not in _err(lib)


def test_null_arguments():
    lib = mcs.capi.load_library()
    v = ct.c_int64(-7)
    assert lib.mcs_set_option(None, 0, 1) != 0
    assert "mcs_set_option" in _err(lib) and "null" in _err(lib)
    assert lib.mcs_get_option(None, 0, ct.byref(v)) != 0
    assert "mcs_get_option" in _err(lib) and "null" in _err(lib) and v.value == -7
    assert lib.mcs_set_tail_slicing(None, 1) != 0 and "null" in _err(lib)


def _status_entry_points_taking_a_context():
    """The entry points of capi.py's signature table that return a status and take the context first.  Not among them: the getters,
    whose int is a value; mcs_destroy, for which no context is nothing to destroy (0, like free(NULL)); the mcs_ens_* calls other
    than mcs_ens_create, whose first argument is the ensemble."""
    lib = mcs.capi.load_library()
    values = {"mcs_num_cus", "mcs_last_launches", "mcs_last_kernel", "mcs_k1_blocks_per_cu"}
    names = []
    for name in mcs.capi.EXPORTED_SYMBOLS:
        fn = getattr(lib, name)
        if fn.restype is not ct.c_int or not fn.argtypes or fn.argtypes[0] is not ct.c_void_p:
            continue
        if name in values or name == "mcs_destroy" or (name.startswith("mcs_ens_") and name != "mcs_ens_create"):
            continue
        names.append(name)
    return names


@pytest.mark.parametrize("name", _status_entry_points_taking_a_context())
def test_null_context_is_an_error_not_a_crash(name):
    lib = mcs.capi.load_library()
    fn = getattr(lib, name)
    assert lib.mcs_option_describe(-1, ct.byref(mcs.capi.McsOptionDesc())) != 0 and "null" not in _err(lib)      # (a stale message)
    assert fn(None, *[t() for t in fn.argtypes[1:]]) != 0, name
    assert "null" in _err(lib), (name, _err(lib))


def test_every_status_entry_point_is_covered():
    names = _status_entry_points_taking_a_context()
    assert len(names) >= 40 and {"mcs_sync", "mcs_run_pcut", "mcs_run_pcuts_fused", "mcs_run_pcuts_pipelined", "mcs_photon_ic",
                                 "mcs_set_launch", "mcs_accumulate_tallies"} <= set(names)


def test_hip_backend_refuses_unknown_option_names():
    from mcs_amd import hip_backend as hb
    with pytest.raises(KeyError, match="no_such_option"):
        hb.HipBackend(0, options={"no_such_option": 1})
    be = hb.HipBackend(0, options={"k1_ws": 1}, use_env=False)
    assert be._options == {mcs.capi.option_key("k1_ws"): 1} and be.use_env is False


def test_options_header_alone_under_sanitizers(tmp_path):
    if not all(_runtime(lib) for lib in ("libasan.so", "libubsan.so", "libasan.a", "libubsan.a")):
        pytest.skip("gcc sanitizer runtimes not installed")
    exe = str(tmp_path / "options_main")
    # (the host compiler, no HIP include path: the header must build alone.  The sanitizer runtimes are linked into the program.)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g",
                           os.path.join(ROOT, "tests", "native", "options_main.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("MCS_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "OPTIONS_OK" in r.stdout, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-3000:]


def test_driver_records_the_options_it_ran_with(monkeypatch):
    """RunResult.options on a backend without run options (the CPU oracle): the four driver-level values as used -- an argument
    wins over its variable, the variable is the default of an argument left out."""
    from conftest import oracle_backend
    N = 200
    prob = make_problem(N)
    ob = oracle_backend(prob)
    r = mcs.driver.run(prob, ob, n_itrs=1, max_pcuts=2)
    assert r.options == dict(fused_pcuts=True, fused_chunk=12, long_draws=0, long_imult_max=8)
    monkeypatch.setenv("MCS_FUSED_CHUNK", "5")
    monkeypatch.setenv("MCS_FUSED_PCUTS", "0")
    monkeypatch.setenv("MCS_LONG_IMULT_MAX", "3")
    prob = make_problem(N)
    ob = oracle_backend(prob)
    r2 = mcs.driver.run(prob, ob, n_itrs=1, max_pcuts=2)
    assert r2.options == dict(fused_pcuts=False, fused_chunk=5, long_draws=0, long_imult_max=3)
    prob = make_problem(N)
    ob = oracle_backend(prob)
    r3 = mcs.driver.run(prob, ob, n_itrs=1, max_pcuts=2, fused_pcuts=True, fused_chunk=3, long_imult_max=2)
    assert r3.options == dict(fused_pcuts=True, fused_chunk=3, long_draws=0, long_imult_max=2)
    assert [dataclass_row(s) for s in r.stats] == [dataclass_row(s) for s in r3.stats]


def dataclass_row(s):
    return (s.i_iter, s.i_ion, s.i_pcut, s.n_pts_use, s.n_saved, s.i_mult)
