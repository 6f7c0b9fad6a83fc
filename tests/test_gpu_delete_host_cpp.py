"""The C++ mirror's Index::delete_documents_by_query through host_capi on two shards (-m gpu): one whole-set call (a dry run and a real
call per shard, ids mapped as local * 2 + shard) and one bounded call under a result sort (the merged search, then add_deleted per
shard), against numpy.  Doc g of the index lives in shard g % 2 as g // 2; the sort column is a permutation of range(n_docs) over the
whole index, so numpy alone decides the page.  What is left alive is read back with dry runs of wider queries."""
import ctypes as C

import numpy as np
import pytest

from host_mirror import HOST_LIB, P, SortC, u8p, u16p, u32p, u64p

pytestmark = pytest.mark.gpu

N_DOCS = 20_035
DF = [0.3, 0.1, 0.2]
ALL = 0xFFFFFFFFFFFFFFFF


def test_cpp_mirror_deletes_by_query_on_two_shards():
    from oracle import oracle as O
    from seekstorm_amd import _native as N
    N.lib()
    H = C.CDLL(HOST_LIB)
    H.ssh_index_create.restype = C.c_void_p
    H.ssh_index_create.argtypes = [C.c_int, C.POINTER(C.c_int)]
    H.ssh_index_destroy.argtypes = [C.c_void_p]
    H.ssh_upload_lexical.argtypes = [C.c_void_p, C.c_int, C.c_uint64, u8p, C.c_uint32, u64p, u32p, u16p]
    H.ssh_upload_facets.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p]
    H.ssh_set_deleted.argtypes = [C.c_void_p, C.c_int, u64p, C.c_uint64]
    H.ssh_delete_documents_by_query.argtypes = [C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                                C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_uint64, u64p, u64p]
    rng = np.random.default_rng(9)
    has = np.zeros((len(DF), N_DOCS), bool)
    for t, df in enumerate(DF):
        has[t, rng.choice(N_DOCS, int(df * N_DOCS), replace=False)] = True
    tf = rng.integers(1, 9, (len(DF), N_DOCS))
    perm = rng.permutation(N_DOCS).astype(np.uint32)
    gone = np.array([0, 1, 63, 64, 4095, 4096, N_DOCS - 1] + np.nonzero(has[0])[0][:5].tolist())
    alive = np.ones(N_DOCS, bool)
    alive[gone] = False
    ix = H.ssh_index_create(2, None)

    def delete(terms, qt, offset=0, length=ALL, sort=None, dry=False):
        t = np.ascontiguousarray(terms, np.uint32)
        sarr = (SortC * 1)()
        if sort is not None:
            sarr[0].facet_offset, sarr[0].facet_type, sarr[0].descending = 0, N.FACET_TYPES["u32"], 1 if sort else 0
        out, n = np.zeros(N_DOCS, np.uint64), C.c_uint64()
        rc = H.ssh_delete_documents_by_query(ix, P(t, u32p), len(t), qt, offset, length, 0, None, C.cast(sarr, C.c_void_p), 0 if sort is None else 1,
                                             None, 0, 1 if dry else 0, N_DOCS, P(out, u64p), C.byref(n))
        assert rc == 0
        return out[:n.value].astype(np.int64)

    try:
        for sid in range(2):
            g = np.arange(sid, N_DOCS, 2)
            n = len(g)
            offs, docs, tfs = [0], [], []
            for t in range(len(DF)):
                local = np.nonzero(has[t, g])[0]
                docs.append(local.astype(np.uint32)); tfs.append(tf[t, g[local]].astype(np.uint16)); offs.append(offs[-1] + len(local))
            offs, docs, tfs = np.asarray(offs, np.uint64), np.concatenate(docs), np.concatenate(tfs)
            dl = O.lex_doclen(n)
            assert H.ssh_upload_lexical(ix, sid, n, P(dl, u8p), len(DF), P(offs, u64p), P(docs, u32p), P(tfs, u16p)) == 0
            rec = np.ascontiguousarray(perm[g])
            assert H.ssh_upload_facets(ix, sid, n, 4, rec.ctypes.data) == 0
            lg = np.array([x // 2 for x in gone if x % 2 == sid], np.uint64)
            assert H.ssh_set_deleted(ix, sid, P(lg, u64p), len(lg)) == 0
        # the whole match set of a union: a dry run first, then for real
        expected = np.nonzero((has[0] | has[1]) & alive)[0]
        assert np.array_equal(delete([0, 1], 1, dry=True), expected)
        assert np.array_equal(delete([0, 1], 1, length=len(expected) + 3), expected)
        alive[expected] = False
        assert len(delete([0, 1], 1, dry=True)) == 0
        assert np.array_equal(delete([0, 1, 2], 1, dry=True), np.nonzero(has[2] & alive)[0])
        # a bounded page under the permutation column, descending: the merged search of both shards, add_deleted per shard
        live = np.nonzero(has[2] & alive)[0]
        order = live[np.argsort(perm[live])][::-1]
        page = np.sort(order[3:3 + 50])
        assert np.array_equal(delete([2], 1, offset=3, length=50, sort=True), page)
        alive[page] = False
        assert np.array_equal(delete([2], 1, dry=True), np.nonzero(has[2] & alive)[0])
        # no terms: nothing
        assert len(delete([], 1)) == 0
    finally:
        H.ssh_index_destroy(ix)
