"""The combination-rank arithmetic of fs_mdr.h (mdr_unrank, mdr_next,
mdr_advance: what every lane of the MDR kernels runs to find and step its
combination) against a plain enumeration, on the host:
tools/mdr_rank_selftest.cpp is compiled with the plain host compiler and run as
a child process.  Every p <= 14 and k <= min(6, p), every rank, steps 1, 3, 4,
63, 255, 256, 257 and 1000.  The program's header gives the sanitizer build."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_arithmetic_selftest(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "mdr_rank_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "mdr_rank_selftest.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok" in run.stdout and "FAILED" not in run.stdout
