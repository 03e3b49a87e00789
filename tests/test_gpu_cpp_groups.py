"""Runs tests/cpp/test_groups.cpp: filter_kmers<K, S> of include/debruijn_mi355x.hpp with summarizers of the caller's own, from a
compiled C++ host, against the CountFilter overload."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_groups")


def build_cpp_groups():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_groups.cpp")
    inc = os.path.join(ROOT, "include")
    deps = [src] + [os.path.join(inc, h) for h in ("debruijn_mi355x.hpp", "dbg_mi355x.h", "dbg_mi355x_groups.h")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + inc, src, "-o", BIN, "-L" + os.path.join(ROOT, "rust-debruijn_amd"),
                           "-ldbg_mi355x", "-Wl,-rpath,$ORIGIN/../../../rust-debruijn_amd", "-Wl,-rpath,/opt/rocm/lib"])
    return BIN


def test_cpp_groups_compiles():
    build_cpp_groups()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_groups_runs():
    build_cpp_groups()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cpp groups ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
