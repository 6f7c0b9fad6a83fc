"""The C++ host mirror of the open level by level (Shard::open_index_bin(..., levels = true) through ssh_open_index_bin_levels of
host_capi.cpp): the corpus and file of tests/test_gpu_open_levels.py are opened through the C++ host, the partial last level is committed
again through Shard::commit_level, and the answers are those of a fresh shard given one array upload; an index opened WITHOUT levels
refuses the same commit with SS_ESTATE."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_open_levels as T  # noqa: E402
from test_host_cpp import H, P, u8p, u16p, u32p, u64p, f32p  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def test_cpp_host_opens_by_levels_and_commits(H):
    import seekstorm_amd as S
    H.ssh_open_index_bin_levels.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, u64p, C.c_uint32]
    corpus = T._Corpus()
    pix = T._index_bin(S, corpus, False)
    order, nd = corpus.lists_of(pix, False)
    data = np.frombuffer(corpus.file, np.uint8).copy()
    o, d, t, _, _ = T._csr(order, 2 * T.LV, 3 * T.LV)
    dl = np.ascontiguousarray(corpus.doclen[2 * T.LV:3 * T.LV])
    commit = lambda ix: H.ssh_commit_level(ix, 0, 2, T.LV, P(dl, u8p), len(order), len(order), P(o, u64p), P(d, u32p), P(t, u16p), None, 0)
    ix = H.ssh_index_create(1, None)
    fresh = T._fresh(S, corpus, order, len(order), 3 * T.LV, False)
    try:
        keys = np.zeros(pix.term_count, np.uint64)
        assert H.ssh_open_index_bin(ix, 0, data.ctypes.data, len(data), T.HEAD, P(keys, u64p), len(keys)) == pix.term_count
        assert commit(ix) == -5  # SS_ESTATE: an image opened whole keeps no levels
        assert H.ssh_open_index_bin_levels(ix, 0, data.ctypes.data, len(data), T.HEAD, 0, P(keys, u64p), len(keys)) == pix.term_count
        assert np.array_equal(keys, pix.term_keys)
        assert commit(ix) == 0
        for name in ("rle_full", "only_last", "a63", "m13", "bm_even"):
            term = np.asarray([corpus.term_id(order, name)], np.uint32)
            doc = np.zeros(10, np.uint64); sc = np.zeros(10, np.float32); meta = np.zeros(4, np.uint64)
            n = H.ssh_search_lexical_shard(ix, 0, P(term, u32p), 1, 1, 0, 10, 2, 10, P(doc, u64p), P(sc, f32p), P(meta, u64p))
            fd, fs, fc, ft = fresh.search_lexical_batch(fresh.make_queries([[int(term[0])]], S.QueryType.Union), 10, S.ResultType.TopkCount)
            assert int(meta[3]) == 0 and n == int(fc[0]) and int(meta[1]) == int(ft[0]), name
            assert int(ft[0]) == order[int(term[0])].cut(0, 3 * T.LV)[1], name
            assert np.allclose(sc[:n], fs[0][:n], rtol=1e-6) and sorted(doc[:n].tolist()) == sorted(fd[0][:n].tolist()), name
    finally:
        H.ssh_index_destroy(ix)
        fresh.close()
        pix.close()
