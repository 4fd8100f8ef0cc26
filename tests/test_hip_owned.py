"""csrc/mcs_hip_owned.h -- the types through which the HIP context owns its device and pinned memory, streams and events, and the
rules by which it reads its environment -- in a stand-alone host program (tests/host/hip_owned_main.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer with leak detection.  The program defines the HIP calls itself, over malloc, and fails the k-th allocation
of every scenario in turn: a failed reserve leaves a buffer empty (a population's buffer: all nine arrays or none), a later one
succeeds, every block is freed exactly once.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_sanitizers import _runtime

CSRC = os.path.join(ROOT, "montecarloscattering.jl_amd", "csrc")
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_owned_buffers_handles_and_environment_rules(tmp_path):
    if not all(_runtime(lib) for lib in ("libasan.so", "libubsan.so", "libasan.a", "libubsan.a")):
        pytest.skip("gcc sanitizer runtimes not installed")
    exe = str(tmp_path / "hip_owned")
    # (the header must build without the HIP compiler and without hip_runtime.h: plain g++, the runtime API's declarations only.
    # The sanitizer runtimes are linked into the program: it then runs whatever else the environment preloads.)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE, "-I" + CSRC,
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g",
                           os.path.join(ROOT, "tests", "host", "hip_owned_main.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("MCS_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "HIP_OWNED_OK" in r.stdout, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-3000:]
