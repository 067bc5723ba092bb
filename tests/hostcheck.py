"""The host-only units of the library checked on the CPU: a tests/*_check.cpp program (its assertions are tests/check.h's CHECK)
built with plain g++ (no hipcc, no HIP runtime, no device) from the csrc sources it exercises, under the sanitizers where their
runtimes are installed, and run directly as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray_tracer_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")


def build(directory, name, sources, check, sanitize="address,undefined", fallback=True, opt=None, rocm=True, fp_contract_off=True, extra=()):
    """Compiles csrc/`sources` + the program `check` (a file of tests/, or a path) into `directory`/`name` and returns its path.
    Skips without g++. `sanitize`: the -fsanitize= list, or None; with `fallback`, a build that fails over a missing sanitizer
    runtime is made again without. `rocm`: ROCm's headers and -D__HIP_PLATFORM_AMD__, for units that see HIP's vector types.
    The compiler must not warn."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(directory / name)
    cc = ["g++", "-std=c++17"] + ([opt] if opt else []) + ["-Wall"] + (["-ffp-contract=off"] if fp_contract_off else [])
    if rocm:
        import __graft_entry__ as built
        cc += ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(built.HIPCC))), "include")]
    cc += ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + TESTS] + [os.path.join(CSRC, s) for s in sources]
    cc += [os.path.join(TESTS, str(check)), "-o", exe] + list(extra)
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=undefined"] if sanitize else []
    b = subprocess.run(cc + flags, capture_output=True, text=True, timeout=600)
    if fallback and flags and b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        b = subprocess.run(cc, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    assert "warning" not in b.stderr, b.stderr[-3000:]
    return exe


def run(exe, args=(), ok=None, timeout=120):
    """Runs the program: it must exit with 0 and print the line `ok` (what its check_finish() prints when no CHECK failed).
    Returns its stdout."""
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert ok is None or ok in p.stdout, (p.stdout + p.stderr)[-4000:]
    return p.stdout
