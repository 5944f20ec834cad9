"""Register report of k_score_sparse3 (no GPU needed, only hipcc).

The segment walk keeps every value that lives across a tile in a fixed
register of its one asm statement, so the kernel needs no scratch memory at
128 VGPRs (1024 threads: 4 waves per SIMD).  A spill creeping back -- the
per-tile statement had ScratchSize 68 and reloaded three f64 sums and the
tile list per tile -- costs time and nothing else shows it, so the compiler's
report lines are asserted here: ``make asm U=fs_pass2`` and, for both
instantiations, ``ScratchSize: 0`` and ``NumVgprs <= 128``.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastselect_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_score_sparse3_needs_no_scratch(tmp_path):
    build = str(tmp_path)
    r = subprocess.run(["make", "-C", CSRC, "asm", "U=fs_pass2", f"BUILD={build}", f"HIPCC={HIPCC}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(os.path.join(build, "fs_pass2.s")).read()
    for F in (8, 4):
        # the report follows the kernel's code: from its label to the next "Kernel info" block
        m = re.search(rf"^_ZN\S*k_score_sparse3ILi{F}E\S*:", text, re.M)
        assert m, f"k_score_sparse3<{F}> not in the assembly"
        info = text[m.end():]
        info = info[info.index("; Kernel info:"):]
        vgprs = int(re.search(r"^; NumVgprs: (\d+)", info, re.M).group(1))
        scratch = int(re.search(r"^; ScratchSize: (\d+)", info, re.M).group(1))
        print(f"k_score_sparse3<{F}>: NumVgprs {vgprs}, ScratchSize {scratch}")
        assert scratch == 0
        assert vgprs <= 128
