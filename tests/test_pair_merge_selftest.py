"""The host side of the pair screen's selection (fs_pairscan.h: the ordered key
of a score with both zeros on one key, the total order, the pair rank
arithmetic, the bounded list PairTopN and its threshold) against a plain sort,
on the host: tools/pair_merge_selftest.cpp is compiled with the plain host
compiler and run as a child process.  Random keys, masses of equal keys, zero
and negative scores, lists shorter than n_top, batches of 1 to the whole stream
under the GPU backend's threshold protocol and 1, 3 and 16 merged lists as the
CPU backend keeps them.  The program's header gives the sanitizer build."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_merge_selftest(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "pair_merge_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "pair_merge_selftest.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok" in run.stdout and "FAILED" not in run.stdout
