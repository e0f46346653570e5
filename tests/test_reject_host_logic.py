"""The run rules of rejection ABC (kissabc.jl_amd/csrc/reject_rules.hpp: what a run takes of a look's accepted rows
and how it finishes) need no GPU: tests/reject_host_check.cpp feeds a table with ties, NaN and +Inf costs to the
run state in looks of many sizes and compares every finished result, byte for byte, with a direct restatement.  The
program is stand-alone and is built with AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("c++") is None, reason="no c++ on PATH")
def test_reject_run_rules_on_cpu(tmp_path):
    exe = str(tmp_path / "reject_host_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kissabc.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "reject_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert r.stdout.count(" ok\n") == 7 * 6, r.stdout[-4000:]
