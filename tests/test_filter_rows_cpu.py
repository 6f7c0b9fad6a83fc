"""The host side of a batch with a facet filter set per query (seekstorm_amd/csrc/filter_rows.h: what ss_bm25_search_each runs before
anything reaches the device, and the filter checks ssi_facet_build shares with it) on the CPU: the host-only header is compiled with a
stand-alone program (tests/filter_rows_check.cpp, its own main) under AddressSanitizer and UBSan, and the program is run -- grouping of
byte-equal sets, empty sets, the filter_begin edges, every refusal, a Point filter's Morton corners, the slow-path marks.  And the
entry's answers to arguments it refuses before it touches a shard."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_rows_header_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "filter_rows_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "filter_rows_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "filter_rows ok" in r.stdout, r.stdout + r.stderr


def test_search_each_refuses_bad_arguments_without_a_shard():
    """ss_bm25_search_each and the faceted coalescer's controls check their arguments before they touch a device: SS_EINVAL (-1)"""
    from seekstorm_amd import _native as N
    L = N.lib()
    cnt, tot, fb = np.zeros(1, np.uint32), np.zeros(1, np.uint64), np.zeros(2, np.uint32)
    q = np.zeros(1, N.BM25_QUERY_DTYPE)
    args = lambda s, rt, fbp: (s, 1, q.ctypes.data, 0, None, 10, rt, fbp, None, 0, None, None, None, None, None, None, None,
                               N.ptr(cnt, N.u32p), N.ptr(tot, N.u64p), None)
    assert L.ss_bm25_search_each(*args(None, N.RT_COUNT, N.ptr(fb, N.u32p))) == N.SS_EINVAL
    assert L.ss_bm25_search_each(*args(None, 3, N.ptr(fb, N.u32p))) == N.SS_EINVAL
    assert L.ss_shard_set_coalescing_faceted(None, 64, 0) == N.SS_EINVAL
    assert L.ss_shard_coalescing_stats_faceted(None, None, None) == N.SS_EINVAL


def test_shard_mirror_has_the_each_methods():
    import inspect
    import seekstorm_amd as S
    sig = inspect.signature(S.Shard.search_lexical_each)
    assert list(sig.parameters)[1:] == ["queries", "k", "result_type", "facet_filters_per_query", "result_sort", "query_facets"]
    assert hasattr(S.Shard, "set_coalescing_faceted") and hasattr(S.Shard, "coalescing_stats_faceted")
