"""The plane-split packed layout (csrc/pgbp_bs16.hpp) on the host: tests/bs16_planes_check.cpp is built with the host compiler
under the address and undefined-behaviour sanitizers and run as a process of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phylogaussianbeliefprop.jl_amd", "csrc")


def test_planes_are_contiguous_runs_and_the_record_tail_is_unchanged(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "bs16_planes_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "bs16_planes_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    for what in ("bijection", "tail", "planes", "p16"):
        assert "ok " + what in lines, out.stdout
    assert lines[-1] == "bs16 planes ok", out.stdout
