"""The shared threshold of the staged pruned kernel from a per-query HISTOGRAM of accepted scores (csrc/bm25_hist.h, bm25_probe_body.h
pb_publish_hist): every partition of a query counts the scores it accepts in 64 buckets between the query's seed (or a fixed share of the
most a doc can score) and that maximum, and any wave publishes the edge of the highest bucket above which k docs were counted.  A bucket
that counts a doc it must not -- a deleted one, one of a NOT list, the same doc twice, another query's -- or an edge above a counted score
lifts the threshold above the true k-th best score and the top-k loses docs: BM25_PRUNED must equal BM25_EXHAUSTIVE bit for bit (docs,
scores, counts, totals) and agree with the CPU oracle.  Every case goes through the staged kernel (the batch repeated to 300 queries) and
through the one-launch kernel of small batches, which keeps its own mechanism, on hand-built corpora of 90 000 docs = 22 sub-blocks, so
that a query of the staged batch runs as 16 partitions."""
import os
import sys

import numpy as np
import pytest

from test_gpu_probe_bound import _both_paths, _equal, _hand_corpus, _oracle, _shards
from test_gpu_pruned import _run

pytestmark = pytest.mark.gpu
N_DOCS = 90_000


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _pick(rng, n, among=None):
    return np.sort(rng.choice(N_DOCS if among is None else among, n, replace=False))


# ---- ties: hundreds of docs in different partitions share the k-th score --------------------------------------------------------------

@pytest.fixture(scope="module")
def tie_world(S, O):
    """all tf equal, all doc lengths equal: a doc's score is decided by WHICH lists hold it -- at most 15 distinct scores over four lists"""
    rng = np.random.default_rng(201)
    lists = [(d, np.ones(len(d), np.int64)) for d in (_pick(rng, int(df * N_DOCS)) for df in (0.30, 0.12, 0.05, 0.02))]
    arrays = _hand_corpus(O, N_DOCS, np.full(N_DOCS, 100), lists)
    sh, osh = _shards(S, O, N_DOCS, *arrays)
    yield sh, osh
    sh.close()


@pytest.mark.parametrize("k", [1, 10, 64, 100])
def test_ties_on_the_kth_score_across_partitions(S, O, tie_world, k):
    sh, osh = tie_world
    tl = [[0, 1, 2], [2, 1, 0], [0, 1], [3, 2], [0, 1, 2, 3], [3, 0, 2, 1], [1, 2, 3], [0, 3]]
    got = _both_paths(S, sh, tl, S.QueryType.Union, k, S.ResultType.Topk, what="ties")
    _oracle(O, osh, got, tl, O.OP_OR, k, S.ResultType.Topk, S, (0, 2, 4, 6))
    # the corpus does what it was built for: the k-th score of [0, 1] is shared by more docs than k
    od, os_, _ = osh.search_exhaustive([0, 1], O.OP_OR, 400)
    assert int((os_ == os_[k - 1]).sum()) > 100 and (got[1][2] == got[1][2][0]).all()


# ---- the main world: best docs deleted / in a NOT list, the clamp at hi, the seed itself, 2 - 4 terms, k beyond the matches ------------

@pytest.fixture(scope="module")
def main_world(S, O):
    """terms 0 - 4: lists of mixed length and tf; doc X (the shortest doc of the corpus) holds the largest tf of every one of them: its
    score is the sum of idf x (largest weight of the list).  term 5: the union of the 50 best docs of three queries over terms 0 - 4 (a
    NOT list, and the docs to delete).  terms 6 - 8: a rare list with large tf and two long lists of tf 1 that share no doc with it --
    the top-10 of [6, 7, 8] are the ten largest weights of list 6, and the 10th of them scores exactly the query's seed.  terms 9, 10: 7
    and 5 docs."""
    rng = np.random.default_rng(202)
    lens = rng.choice([60, 100, 160], N_DOCS)
    x = 40_001
    lens[x] = 20
    lists = []
    for df in (0.02, 0.05, 0.4, 0.15, 0.08):
        d = np.union1d(_pick(rng, int(df * N_DOCS)), [x])
        tf = rng.geometric(0.5, len(d)).clip(1, 40)
        tf[np.searchsorted(d, x)] = 60
        lists.append((d, tf))
    tops = [[0, 1, 2], [1, 2, 3, 4], [3, 4]]
    osh0 = O.Shard(N_DOCS, *_hand_corpus(O, N_DOCS, lens, lists))
    gone = np.unique(np.concatenate([osh0.search_exhaustive(t, O.OP_OR, 50)[0] for t in tops])).astype(np.int64)
    assert x in gone and len(gone) >= 50
    lists.append((gone, np.ones(len(gone), np.int64)))                                         # 5
    rare = _pick(rng, 300)
    others = np.setdiff1d(np.arange(N_DOCS), rare)
    lists.append((rare, rng.permutation(300) % 37 + 4))                                        # 6
    for df in (0.35, 0.2):                                                                     # 7, 8
        d = np.sort(rng.choice(others, int(df * N_DOCS), replace=False))
        lists.append((d, np.ones(len(d), np.int64)))
    lists.append((_pick(rng, 7), rng.integers(1, 9, 7)))                                       # 9
    lists.append((_pick(rng, 5), rng.integers(1, 9, 5)))                                       # 10
    arrays = _hand_corpus(O, N_DOCS, lens, lists)
    sh, osh = _shards(S, O, N_DOCS, *arrays)
    yield sh, osh, tops, gone, x
    sh.close()


@pytest.mark.parametrize("how", ["deleted", "not_list", "both"])
def test_the_best_docs_are_deleted_or_in_a_not_list(S, O, main_world, how):
    """counting one of the 50 best docs would lift the threshold above the truth; these queries have no seed (the seedless lo)"""
    from seekstorm_amd import _native as N
    sh, osh, tops, gone, _ = main_world
    nots = [[5] for _ in tops] if how != "deleted" else None
    dele = gone if how == "deleted" else gone[::2] if how == "both" else []
    try:
        sh.set_deleted(dele); osh.set_deleted([int(d) for d in dele])
        for k in (10, 64):
            for rt in (S.ResultType.Topk, S.ResultType.TopkCount):
                got = _both_paths(S, sh, tops, S.QueryType.Union, k, rt, nots, what=(how, k))
                _oracle(O, osh, got, tops, O.OP_OR, k, rt, S, range(len(tops)), nots)
                assert not set(got[0][got[0] != N.SS_NO_DOC].tolist()) & set(gone.tolist())
    finally:
        sh.set_deleted([]); osh.set_deleted([])


@pytest.mark.parametrize("k", [1, 10, 100])
def test_a_doc_of_every_lists_largest_weight_and_unions_of_2_to_4_terms(S, O, main_world, k):
    """doc X scores sum(idf x umax) up to rounding: the clamp at hi; TopkCount totals are what they were"""
    sh, osh, _, _, x = main_world
    tl = [[0, 1], [4, 2], [0, 1, 2], [2, 3, 4], [4, 0, 3], [0, 1, 2, 3], [4, 3, 2, 1], [1, 3]]
    for rt in (S.ResultType.Topk, S.ResultType.TopkCount):
        got = _both_paths(S, sh, tl, S.QueryType.Union, k, rt, what=("clamp", k))
        _oracle(O, osh, got, tl, O.OP_OR, k, rt, S, range(0, len(tl), 2))
        assert (got[0][:, 0] == x).all()


def test_a_doc_whose_score_equals_the_seed(S, O, main_world):
    sh, osh, _, _, _ = main_world
    tl = [[6, 7, 8], [7, 6], [8, 7, 6], [6, 8]]
    for k in (1, 10):
        got = _both_paths(S, sh, tl, S.QueryType.Union, k, S.ResultType.Topk, what=("seed", k))
        _oracle(O, osh, got, tl, O.OP_OR, k, S.ResultType.Topk, S, range(len(tl)))
    # the seed of [6, 7, 8] at k = 10 is idf x the 10th largest weight of list 6, and that is the 10th best score itself
    single = _run(S, sh, sh.make_queries([[6]], S.QueryType.Union), 10, S.ResultType.Topk, 0)
    assert got[1][0][9] == single[1][0][9] and np.array_equal(got[1][0], single[1][0])


@pytest.mark.parametrize("k", [10, 64, 100])
def test_k_larger_than_the_number_of_matches(S, O, main_world, k):
    sh, osh, _, _, _ = main_world
    tl = [[9, 10], [10, 9], [9], [10]]
    got = _both_paths(S, sh, tl, S.QueryType.Union, k, S.ResultType.TopkCount, what=("k > matches", k))
    _oracle(O, osh, got, tl, O.OP_OR, k, S.ResultType.TopkCount, S, range(len(tl)))
    assert int(got[2][2]) == int(got[3][2]) == 7 and int(got[2][3]) == int(got[3][3]) == 5 and 7 <= int(got[3][0]) <= 12


def test_adjacent_queries_of_far_apart_scores_and_calls_in_a_row(S, O, main_world):
    """counters must not leak between the queries of a batch (rows alternate between scores of the rare list's level and of the tf-1
    lists') nor between calls (batch A twice, then a batch B of lower scores on the same workspace)"""
    from seekstorm_amd import _native as N
    sh, osh, _, _, _ = main_world
    hi_q, lo_q = [[6, 7, 8], [6, 0, 1], [0, 1, 2]], [[7, 8], [8, 7], [7]]
    mixed = [q for pair in zip(hi_q, lo_q) for q in pair]
    got = _both_paths(S, sh, mixed, S.QueryType.Union, 10, S.ResultType.TopkCount, what="mixed rows")
    _oracle(O, osh, got, mixed, O.OP_OR, 10, S.ResultType.TopkCount, S, range(len(mixed)))
    assert got[1][0][9] > 2 * got[1][1][0]  # (far apart: the WORST kept score of a high row lies above the BEST of a low one)
    a, b = sh.make_queries(hi_q * 100, S.QueryType.Union), sh.make_queries(lo_q * 100, S.QueryType.Union)
    ea, eb = (_run(S, sh, q, 10, S.ResultType.Topk, N.BM25_EXHAUSTIVE) for q in (a, b))
    for q, e, what in ((a, ea, "A"), (a, ea, "A again"), (b, eb, "B after A"), (a, ea, "A after B")):
        _equal(_run(S, sh, q, 10, S.ResultType.Topk, N.BM25_PRUNED), e, S.ResultType.Topk, S, what)


# ---- two indexed fields: a doc in both fields' lists of a term is one doc --------------------------------------------------------------

def test_two_fields_with_docs_in_both_lists_of_a_term(S, O):
    from seekstorm_amd import _native as N
    rng = np.random.default_rng(203)
    dl = np.stack([O.lex_doclen(N_DOCS, seed=O.LEX_SEED + 5 * f) for f in range(2)])
    boost = np.array([2.0, 1.0], np.float32)
    offs, D, F, T = [0], [], [], []
    for df in (0.01, 0.06, 0.3, 0.12):
        d = _pick(rng, int(df * N_DOCS))
        where = rng.integers(0, 3, len(d))  # 0: field 0 only, 1: field 1 only, 2: both
        dd = np.concatenate([d[where != 1], d[where != 0]])
        ff = np.concatenate([np.zeros(int((where != 1).sum()), np.int64), np.ones(int((where != 0).sum()), np.int64)])
        o = np.lexsort((ff, dd))
        D.append(dd[o]); F.append(ff[o]); T.append(rng.geometric(0.5, len(o)).clip(1, 30)); offs.append(offs[-1] + len(o))
    offs, D, F, T = np.array(offs, np.uint64), np.concatenate(D).astype(np.uint32), np.concatenate(F).astype(np.uint8), np.concatenate(T).astype(np.uint16)
    sh = S.Shard(0)
    try:
        sh.upload_lexical_fields(N_DOCS, dl, boost, offs, D, F, T)
        tl = [[0, 1, 2], [2, 3], [3, 2, 1, 0], [1, 3, 0]]
        for k in (10, 64):
            got = _both_paths(S, sh, tl, S.QueryType.Union, k, S.ResultType.TopkCount, what=("two fields", k))
            for i, terms in enumerate(tl):
                od, os_, otot, _ = O.search_fields_exhaustive(N_DOCS, dl, boost, offs, D, F, T, terms, O.OP_OR, k)
                n = int(got[2][i])
                assert n == len(od) == len(set(got[0][i][:n].tolist())) and int(got[3][i]) == otot
                assert np.allclose(got[1][i][:n], os_, rtol=1e-4)
                band = abs(float(os_[-1])) * 2e-4
                assert {int(a) for a, b in zip(got[0][i][:n], got[1][i][:n]) if b > os_[-1] + band} <= set(od.tolist())
    finally:
        sh.close()


# ---- sub-block bounds in force: the SKIP instantiation ----------------------------------------------------------------------------------

def test_sub_block_bounds_in_force(S, O):
    """weights clustered by doc id (tools/probes/skew_corpus.py): batches of >= 128 queries run the body's SKIP instantiations, whose
    driver streams jump by the threshold the histogram publishes -- with and without tombstones (seedless)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probes"))
    import skew_corpus
    from seekstorm_amd import _native as N
    n_docs = 150_000
    arrays = skew_corpus.build(O, n_docs, [0.012, 0.035, 0.10, 0.02, 0.3], region_log2=12)
    sh, osh = _shards(S, O, n_docs, *arrays)
    tl = [[0, 1, 2], [2, 4, 0], [0, 2, 3, 1], [4, 3, 2, 1], [1, 3, 4], [4, 2]] * 50
    try:
        for gone in ([], list(range(12288, 12288 + 4096, 3))):
            sh.set_deleted(gone); osh.set_deleted(gone)
            for k in (10, 64):
                q = sh.make_queries(tl, S.QueryType.Union)
                p = _run(S, sh, q, k, S.ResultType.TopkCount, N.BM25_PRUNED)
                e = _run(S, sh, q, k, S.ResultType.TopkCount, N.BM25_EXHAUSTIVE)
                _equal(p, e, S.ResultType.TopkCount, S, ("skip", k, bool(gone)))
                _oracle(O, osh, p, tl, O.OP_OR, k, S.ResultType.TopkCount, S, (0, 2, 5))
    finally:
        sh.set_deleted([]); osh.set_deleted([])
        sh.close()
