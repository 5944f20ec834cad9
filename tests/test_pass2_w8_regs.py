"""Register report of k_score_sparse3_w8 (no GPU needed, only hipcc).

The 8-wave form of the sparse pass 2 pays only while two 1024-thread
workgroups share a CU: 8 waves per SIMD.  That holds with at most 64 VGPRs,
an ``.sgpr_count`` of at most 80 (82 to 96 admit 7 waves per SIMD, which for
1024-thread workgroups is one workgroup per CU again), no scratch memory and
two row blocks in the CU's 160 KB of LDS.  A register creeping over any of
these costs half the occupancy and nothing else shows it, so the compiler's
report is asserted here from ``make asm U=fs_pass2``.
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
def test_score_sparse3_w8_fits_8_waves(tmp_path):
    build = str(tmp_path)
    r = subprocess.run(["make", "-C", CSRC, "asm", "U=fs_pass2", f"BUILD={build}", f"HIPCC={HIPCC}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(os.path.join(build, "fs_pass2.s")).read()
    m = re.search(r"^(_ZN\S*k_score_sparse3_w8\S*):", text, re.M)
    assert m, "k_score_sparse3_w8 not in the assembly"
    name = m.group(1)
    # the report follows the kernel's code: from its label to the next "Kernel info" block
    info = text[m.end():]
    info = info[info.index("; Kernel info:"):]
    vgprs = int(re.search(r"^; NumVgprs: (\d+)", info, re.M).group(1))
    scratch = int(re.search(r"^; ScratchSize: (\d+)", info, re.M).group(1))
    lds = int(re.search(r"^; LDSByteSize: (\d+)", info, re.M).group(1))
    # the kernel's entry in the code object's metadata
    meta = text[text.index(f".name:           {name}\n"):]
    meta = meta[:meta.index(".wavefront_size")]
    sgprs = int(re.search(r"\.sgpr_count:\s+(\d+)", meta).group(1))
    print(f"k_score_sparse3_w8: NumVgprs {vgprs}, .sgpr_count {sgprs}, ScratchSize {scratch}, LDS {lds}")
    assert scratch == 0
    assert vgprs <= 64
    assert sgprs <= 80
    assert lds <= 81920
