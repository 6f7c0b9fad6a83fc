"""The host pass over one committed level of a multi-field sparse tier (seekstorm_amd/csrc/mf_sparse_level.h, what
ss_bm25_commit_sparse_level_fields runs before anything reaches the device) on the CPU: the host-only header is compiled with a
stand-alone program (tests/mf_sparse_level_check.cpp, its own main) under AddressSanitizer and UBSan, and the program is run -- an empty
list, a list of one entry, docs in all fields and in one, the first and the last doc of a level, npos given and NULL, an empty positions
pool, every refusal of the validation.  And the entry's answers to missing arguments, and the two Shard mirrors of the commit seam."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mf_sparse_level_header_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "mf_sparse_level_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "mf_sparse_level_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mf_sparse_level ok" in r.stdout, r.stdout + r.stderr


def test_commit_sparse_level_fields_refuses_missing_arguments():
    """ss_bm25_commit_sparse_level_fields checks its arguments before it touches a device or a shard: SS_EINVAL (-1)"""
    from seekstorm_amd import _native as N
    L = N.lib()
    offs = np.zeros(2, np.uint64)
    assert L.ss_bm25_commit_sparse_level_fields(None, 0, 1, N.ptr(offs, N.u64p), None, None, None, None, None, 0) == -1
    shard_stand_in = np.zeros(8, np.uint64)  # (never read: the offsets are missing)
    assert L.ss_bm25_commit_sparse_level_fields(shard_stand_in.ctypes.data, 0, 1, None, None, None, None, None, None, 0) == -1


def test_shard_mirror_has_the_tier_methods():
    import seekstorm_amd as S
    sig = inspect.signature(S.Shard.commit_sparse_level_fields)
    assert list(sig.parameters)[1:] == ["level", "offs", "docs", "fields", "tfs", "positions", "npos"]
    assert sig.parameters["positions"].default is None and sig.parameters["npos"].default is None
    sig = inspect.signature(S.Shard.commit_level_fields_tiered)
    assert list(sig.parameters)[1:] == ["level", "level_doclen", "boost", "term_offsets", "doc_ids", "fields", "tfs", "n_dense_terms", "positions",
                                        "npos"]
    assert sig.parameters["positions"].default is None and sig.parameters["npos"].default is None


def test_commit_level_fields_tiered_splits_a_level_between_the_tiers():
    """Shard.commit_level_fields_tiered: one CSR of all known terms in id order -> the dense terms' entries for ss_bm25_commit_level_fields,
    the rare terms' entries (offsets rebased, positions pool cut where the dense entries' positions end) for
    ss_bm25_commit_sparse_level_fields.  Host logic only: the two ABI calls are captured."""
    import seekstorm_amd as S
    calls = {}

    class Capture(S.Shard):
        def __init__(self):  # no device
            pass

        def commit_level_fields(self, level, level_doclen, boost, offs, docs, fields, tfs, positions=None, npos=None):
            calls["dense"] = (level, np.asarray(offs), np.asarray(docs), np.asarray(fields), np.asarray(tfs), positions, npos, np.asarray(level_doclen).shape,
                              list(boost))

        def commit_sparse_level_fields(self, level, offs, docs, fields, tfs, positions=None, npos=None):
            calls["sparse"] = (level, np.asarray(offs), np.asarray(docs), np.asarray(fields), np.asarray(tfs), positions, npos)

    offs = np.array([0, 3, 4, 4, 6, 7], np.uint64)            # 5 terms: 3 dense, 2 rare
    docs = np.array([70000, 70000, 70010, 70001, 70002, 70002, 70005], np.uint32)
    flds = np.array([0, 2, 1, 1, 0, 1, 2], np.uint8)
    tfs = np.array([2, 1, 1, 3, 1, 2, 1], np.uint16)
    pos = np.arange(int(tfs.sum()), dtype=np.uint16)
    dl = np.zeros((3, 100), np.uint8)
    sh = Capture()
    sh.commit_level_fields_tiered(1, dl, [2.0, 1.0, 0.5], offs, docs, flds, tfs, 3, positions=pos)
    lv, o, d, f, t, p, n, shape, boost = calls["dense"]
    assert lv == 1 and o.tolist() == [0, 3, 4, 4] and d.tolist() == [70000, 70000, 70010, 70001] and f.tolist() == [0, 2, 1, 1]
    assert t.tolist() == [2, 1, 1, 3] and p.tolist() == list(range(7)) and n is None and shape == (3, 100) and boost == [2.0, 1.0, 0.5]
    lv, o, d, f, t, p, n = calls["sparse"]
    assert lv == 1 and o.tolist() == [0, 2, 3] and d.tolist() == [70002, 70002, 70005] and f.tolist() == [0, 1, 2] and t.tolist() == [1, 2, 1]
    assert p.tolist() == [7, 8, 9, 10] and n is None
    # counts from npos where given (n-gram components): the cut follows them
    npos = np.array([2, 0, 1, 3, 1, 0, 1], np.uint16)
    sh.commit_level_fields_tiered(1, dl, [2.0, 1.0, 0.5], offs, docs, flds, tfs, 3, positions=np.arange(8, dtype=np.uint16), npos=npos)
    assert calls["dense"][5].tolist() == [0, 1, 2, 3, 4, 5] and calls["dense"][6].tolist() == [2, 0, 1, 3]
    assert calls["sparse"][5].tolist() == [6, 7] and calls["sparse"][6].tolist() == [1, 0, 1]
    # without positions neither call gets any
    sh.commit_level_fields_tiered(1, dl, [2.0, 1.0, 0.5], offs, docs, flds, tfs, 3)
    assert calls["dense"][5] is None and calls["sparse"][5] is None and calls["sparse"][1].tolist() == [0, 2, 3]
    calls.clear()
    sh.commit_level_fields_tiered(0, dl, [1.0, 1.0, 1.0], offs[:4], docs[:4], flds[:4], tfs[:4], 3)  # no rare term: the dense call alone
    assert "sparse" not in calls and calls["dense"][1].tolist() == [0, 3, 4, 4]
    with pytest.raises(ValueError):
        sh.commit_level_fields_tiered(0, dl, [1.0, 1.0, 1.0], offs[:3], docs[:4], flds[:4], tfs[:4], 3)  # fewer terms than the dense image holds
