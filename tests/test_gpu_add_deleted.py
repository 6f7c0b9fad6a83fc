"""ss_add_deleted: docs ADDED to the tombstone set on the device (-m gpu).

set_deleted(A) then add_deleted(B) on one shard answers as set_deleted(A | B) on another: every output is an integer or a stored bit
pattern, so every comparison is ==; the totals of the empty query are also n_docs - |A | B| in numpy.  A's largest id is 63 (a bitmap
of two words), B holds 64, 4 095, 4 096 and n_docs - 1 -- growth of the bitmap, the seams of a word and of a 4 096-doc sub-block --,
duplicates and members of A: the set's size stays the number of DISTINCT docs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_DOCS, DIM = 20_003, 64
DF = [0.6, 0.25, 0.05]
A = [0, 1, 5, 31, 32, 40, 63]
B = [64, 4095, 4096, N_DOCS - 1, 64, 64, 4096, 5, 63, 100, 101, 7000, 7000, 12_345]
SS_EINVAL = -1


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def corpus(O):
    rng = np.random.default_rng(5)
    offs, docs, tfs = [0], [], []
    for df in DF:
        d = np.sort(rng.choice(N_DOCS, int(df * N_DOCS), replace=False)).astype(np.uint32)
        docs.append(d); tfs.append(np.minimum(rng.geometric(0.6, len(d)), 60).astype(np.uint16)); offs.append(offs[-1] + len(d))
    return (O.lex_doclen(N_DOCS), np.asarray(offs, np.uint64), np.concatenate(docs), np.concatenate(tfs),
            O.vec_gen(O.VEC_SEED, 0, N_DOCS, DIM), O.vec_gen(O.VECQ_SEED, 0, 4, DIM))


def _shard(S, corpus):
    dl, offs, docs, tfs, rows, _ = corpus
    sh = S.Shard(0)
    sh.upload_lexical(N_DOCS, dl, offs, docs, tfs)
    sh.upload_vectors(rows)
    return sh


def _answers(S, sh, corpus):
    """everything a tombstone can change, as a flat list of integer arrays"""
    out = []
    for terms, qt in (([[0, 1, 2], [1, 2]], S.QueryType.Union), ([[0, 1], [0, 1, 2]], S.QueryType.Intersection)):
        d, s, c, t = sh.search_lexical_batch(sh.make_queries(terms, qt), 100, S.ResultType.TopkCount)
        out += [d, s.view(np.uint32), c, t]
    d, s, c, t, ncl, obs = sh.search_vector_batch(corpus[5], 50, with_observed=True)
    out += [d, s.view(np.uint32), c, t, np.asarray(ncl), np.asarray(obs)]
    for asc in (False, True):
        d, cnt, tot, _ = sh.search_docs(200, doc_ascending=asc)
        out += [d, np.array([cnt, tot])]
    d, cnt, tot, _ = sh.search_docs(50, skip=4000, doc_ascending=True)  # a page over the sub-block seam
    out += [d, np.array([cnt, tot])]
    return out


def _same(x, y):
    return len(x) == len(y) and all(np.array_equal(a, b) for a, b in zip(x, y))


def test_add_deleted_equals_set_deleted_of_the_union(S, corpus):
    from seekstorm_amd import _native as N
    one, two, none = _shard(S, corpus), _shard(S, corpus), _shard(S, corpus)
    try:
        union = sorted(set(A) | set(B))
        one.set_deleted(A)
        one.add_deleted(B)
        two.set_deleted(union)
        got, want = _answers(S, one, corpus), _answers(S, two, corpus)
        assert _same(got, want)
        assert not _same(got, _answers(S, none, corpus))  # (the tombstones do change these answers)
        alive = np.ones(N_DOCS, bool)
        alive[union] = False
        d, cnt, tot, _ = one.search_docs(N_DOCS, doc_ascending=True)
        assert tot == N_DOCS - len(union) and np.array_equal(d, np.nonzero(alive)[0])
        # nothing to add; every doc known already; an id that is no doc id: the answers stay
        one.add_deleted([])
        one.add_deleted(B + A)
        assert _same(_answers(S, one, corpus), want)
        bad = np.array([3, 0xFFFFFFFF, 9], np.uint64)
        assert N.lib().ss_add_deleted(one._h, N.ptr(bad, N.u64p), 3) == SS_EINVAL
        assert N.lib().ss_add_deleted(one._h, None, 3) == SS_EINVAL
        assert _same(_answers(S, one, corpus), want)
        # a shard without a set yet
        none.add_deleted(B)
        two.set_deleted(B)
        assert _same(_answers(S, none, corpus), _answers(S, two, corpus))
        d, cnt, tot, _ = none.search_docs(10)
        assert tot == N_DOCS - len(set(B))
        # and set_deleted after add_deleted replaces the whole set, as ever
        none.set_deleted([])
        d, cnt, tot, _ = none.search_docs(10)
        assert tot == N_DOCS
    finally:
        for sh in (one, two, none):
            sh.close()
