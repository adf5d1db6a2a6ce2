"""The owners of device memory (csrc/pgbp_devmem.hpp) against a counting stand-in for the runtime: tests/devmem_check.cpp is
built with the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phylogaussianbeliefprop.jl_amd", "csrc")


def test_devbuf_and_event_pair_release_everything_and_acquire_groups_whole(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "devmem_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "devmem_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    for what in ("scope exit", "reset", "alloc", "move", "swap", "group of eight", "event pair"):
        assert "ok " + what in lines, out.stdout
    assert lines[-1] == "devmem ok", out.stdout
