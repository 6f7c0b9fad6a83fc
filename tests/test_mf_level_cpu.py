"""The host pass over one committed level of a multi-field image (seekstorm_amd/csrc/mf_level.h, what ss_bm25_commit_level_fields runs
before anything reaches the device) on the CPU: the host-only header is compiled with a stand-alone program (tests/mf_level_check.cpp,
its own main) under AddressSanitizer and UBSan, and the program is run -- an empty term, one field only, all fields, a level of one doc
and of 65 536, npos given and NULL, every refusal of the validation.  And the entry's answers to missing arguments."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mf_level_header_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "mf_level_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "mf_level_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mf_level ok" in r.stdout, r.stdout + r.stderr


def test_commit_level_fields_refuses_missing_arguments():
    """ss_bm25_commit_level_fields checks its arguments before it touches a device or a shard: SS_EINVAL (-1)"""
    from seekstorm_amd import _native as N
    L = N.lib()
    offs = np.zeros(2, np.uint64)
    dl = np.zeros(2, np.uint8)
    assert L.ss_bm25_commit_level_fields(None, 0, 1, 2, N.ptr(dl, N.u8p), None, 1, N.ptr(offs, N.u64p), None, None, None, None, None, 0) == -1
    assert L.ss_bm25_commit_level_fields(None, 0, 1, 2, None, None, 1, None, None, None, None, None, None, 0) == -1


def test_shard_mirror_has_the_commit_method():
    import seekstorm_amd as S
    import inspect
    sig = inspect.signature(S.Shard.commit_level_fields)
    assert list(sig.parameters)[1:] == ["level", "level_doclen", "boost", "term_offsets", "doc_ids", "fields", "tfs", "positions", "npos"]
