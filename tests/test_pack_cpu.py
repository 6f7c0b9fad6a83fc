"""The packed query form of host-pointer BM25 batches (seekstorm_amd/csrc/bm25_pack.h) on the CPU: the host-only header is compiled
with a stand-alone program (tests/pack_check.cpp, its own main) under AddressSanitizer and UBSan, and the program is run -- widths 1..32,
1 and 1000 queries, NOT terms, re-striding, the worst-case stride against the staging buffer's capacity rule."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_header_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "pack_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "pack_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pack ok" in r.stdout, r.stdout + r.stderr
