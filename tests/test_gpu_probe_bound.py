"""The sparse stage of the pruned strategy in two phases (csrc/bm25_probe_body.h, queries of >= 3 terms): a survivor of the dense stage is
bounded by the lists it is actually IN before any rank-table entry or posting is fetched for it, and only what passes waits in a second
queue for those fetches.  Whatever that bound drops must be a doc the top-k never needed: BM25_PRUNED must equal BM25_EXHAUSTIVE bit for
bit (docs, scores, counts, totals) and agree with the CPU oracle, on corpora built where the rule can go wrong -- a rare list with large
tf (docs of the driver alone belong in the top-k), ties on the k-th score, 4-term unions and 3- / 4-term intersections with exact counts,
streams that end with either queue holding 0, 1, 63, 64 or 65 entries, tombstones and NOT terms on docs that pass the bound, sub-block
bounds in force, k beyond the match count -- through the staged kernel (device-resident queries; host batches beyond 256 queries) and
the one-launch kernel of small host-pointer batches."""
import numpy as np
import pytest

from test_gpu_pruned import REL, _corpus, _run
from test_gpu_small_batch import _dev_search

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _shards(S, O, n_docs, dl, offs, docs, tfs):
    sh = S.Shard(0)
    sh.upload_lexical(n_docs, dl, offs, docs, tfs)
    return sh, O.Shard(n_docs, dl, offs, docs, tfs)


def _hand_corpus(O, n_docs, lens, lists):
    """lists: [(sorted unique doc ids, tfs)] -> the arrays upload_lexical takes"""
    lens = np.asarray(lens, np.int64)
    lut = {int(x): int(O.lib().so_int_to_byte4(int(x))) for x in np.unique(lens)}
    doclen = np.array([lut[int(x)] for x in lens], np.uint8)
    offs = np.cumsum([0] + [len(d) for d, _ in lists]).astype(np.uint64)
    return doclen, offs, np.concatenate([np.asarray(d, np.uint32) for d, _ in lists]), np.concatenate([np.asarray(t, np.uint16) for _, t in lists])


def _equal(a, b, rt, S, what):
    """two answers of search_lexical_batch: counts, scores, docs -- and the totals where the request asks for them"""
    assert np.array_equal(a[2], b[2]), (what, "counts")
    if rt != S.ResultType.Count:
        assert np.array_equal(a[1], b[1]), (what, "scores")
        assert np.array_equal(a[0], b[0]), (what, "docs")
    if rt != S.ResultType.Topk:
        assert np.array_equal(a[3], b[3]), (what, "totals")


def _ops(is_and, nt, n_not=0):
    return (1 if is_and else 2) | ((nt + n_not) << 8) | (nt << 16) | (n_not << 24)


def _both_paths(S, sh, lists, qt, k, rt, nots=None, what=None):
    """PRUNED == EXHAUSTIVE on the one-launch kernel (the batch as it is, <= 64 queries) and on the staged kernel (the batch repeated
    to 300 queries: beyond what the one-launch path takes).  Returns the pruned answer of the batch as it is."""
    from seekstorm_amd import _native as N
    assert len(lists) <= 64
    q = sh.make_queries(lists, qt, nots)
    before = sh.one_launch_batches()
    p = _run(S, sh, q, k, rt, N.BM25_PRUNED)
    if rt != S.ResultType.Count:
        assert sh.one_launch_batches() == before + 1, "the batch did not take the one-launch path"
    e = _run(S, sh, q, k, rt, N.BM25_EXHAUSTIVE)
    _equal(p, e, rt, S, (what, "one launch", k, rt))
    rep = -(-300 // len(lists))
    big = sh.make_queries(lists * rep, qt, None if nots is None else nots * rep)
    before = sh.one_launch_batches()
    pb = _run(S, sh, big, k, rt, N.BM25_PRUNED)
    assert sh.one_launch_batches() == before, "the batch of 300 did not take the staged pipeline"
    eb = _run(S, sh, big, k, rt, N.BM25_EXHAUSTIVE)
    _equal(pb, eb, rt, S, (what, "staged", k, rt))
    n = len(lists)
    for x, y in zip(pb, p):  # every repetition answers like the first
        assert np.array_equal(x[:n], y) and np.array_equal(x[-n:], y), (what, "repetitions")
    return p


def _oracle(O, osh, got, lists, op, k, rt, S, picks, nots=None):
    doc, score, cnt, tot = got
    for i in picks:
        od, os_, otot = osh.search_exhaustive(lists[i], op, k, not_terms=nots[i] if nots else ())
        n = int(cnt[i])
        if rt != S.ResultType.Topk:
            assert int(tot[i]) == otot, (lists[i], "total")
        if rt == S.ResultType.Count:
            continue
        assert n == len(od), (lists[i], n, len(od))
        assert np.allclose(score[i][:n], os_, rtol=REL)
        if n:
            band = abs(float(os_[-1])) * REL
            assert {int(x) for x, y in zip(doc[i][:n], score[i][:n]) if y > os_[-1] + band} == \
                   {int(x) for x, y in zip(od, os_) if y > os_[-1] + band}, lists[i]


# ---- a rare list with large tf -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rare_world(S, O):
    """term 0: rare, half of its postings with tf 20 .. 300 -- its docs ALONE outrank docs of all lists with tf 1; term 1 middle, term 2
    common, term 3 a further list; every list but the rare one has tf 1 or 2.  22 sub-blocks."""
    n_docs = 90_000
    rng = np.random.default_rng(41)
    lens = rng.choice([60, 100, 160], n_docs)
    lists = []
    for df, big in ((0.004, True), (0.05, False), (0.4, False), (0.15, False)):
        d = np.sort(rng.choice(n_docs, int(df * n_docs), replace=False))
        tf = rng.integers(1, 3, len(d))
        if big:
            m = rng.random(len(d)) < 0.5
            tf[m] = rng.integers(20, 300, int(m.sum()))
        lists.append((d, tf))
    arrays = _hand_corpus(O, n_docs, lens, lists)
    sh, osh = _shards(S, O, n_docs, *arrays)
    yield sh, osh, lists
    sh.close()


@pytest.mark.parametrize("k", [1, 10, 64, 100])
def test_rare_list_with_large_tf(S, O, rare_world, k):
    sh, osh, lists = rare_world
    tl = [[0, 1, 2], [2, 1, 0], [1, 0, 2], [0, 1, 2, 3], [3, 2, 1, 0], [0, 2, 3], [1, 2, 3]]
    got = _both_paths(S, sh, tl, S.QueryType.Union, k, S.ResultType.Topk, what="rare list")
    _oracle(O, osh, got, tl, O.OP_OR, k, S.ResultType.Topk, S, (0, 3, 5))
    # the corpus does what it was built for: docs that are in the rare list and NOT in the middle one stand in the top-k of [0, 1, 2]
    in1 = set(lists[1][0].tolist())
    if k >= 64:
        assert any(int(d) not in in1 for d in got[0][0][:int(got[2][0])])
    got = _both_paths(S, sh, tl, S.QueryType.Union, k, S.ResultType.TopkCount, what="rare list")
    _oracle(O, osh, got, tl, O.OP_OR, k, S.ResultType.TopkCount, S, (1, 4))


# ---- ties on the k-th score -------------------------------------------------------------------------------------------------------------

def test_tie_heavy_weights(S, O):
    n_docs = 40_000
    dfs = [0.002, 0.01, 0.03, 0.08, 0.2, 0.45, 0.005, 0.12]
    arrays = _corpus(O, n_docs, dfs, 77, tie_heavy=True)
    sh, osh = _shards(S, O, n_docs, *arrays)
    rng = np.random.default_rng(5)
    tl = [[int(x) for x in rng.choice(len(dfs), int(rng.integers(3, 5)), replace=False)] for _ in range(30)] + [[0, 6, 1], [5, 4, 3, 7]]
    for k in (1, 10, 100):
        got = _both_paths(S, sh, tl, S.QueryType.Union, k, S.ResultType.Topk, what="ties")
        _oracle(O, osh, got, tl, O.OP_OR, k, S.ResultType.Topk, S, (0, 9, len(tl) - 1))
    sh.close()


# ---- 4-term unions, 3- and 4-term intersections, exact counts; filters --------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed_world(S, O):
    n_docs = 80_000
    dfs = [0.003, 0.02, 0.06, 0.15, 0.35, 0.6, 0.01, 0.09]
    arrays = _corpus(O, n_docs, dfs, 123, big_tf=1)
    sh, osh = _shards(S, O, n_docs, *arrays)
    rng = np.random.default_rng(17)
    tl3 = [[int(x) for x in rng.choice(len(dfs), 3, replace=False)] for _ in range(20)] + [[0, 6, 1], [5, 4, 3]]
    tl4 = [[int(x) for x in rng.choice(len(dfs), 4, replace=False)] for _ in range(20)] + [[0, 6, 1, 2], [5, 4, 3, 7]]
    yield sh, osh, tl3, tl4, n_docs
    sh.close()


@pytest.mark.parametrize("shape", ["or4", "and3", "and4"])
def test_unions_and_intersections_with_exact_counts(S, O, mixed_world, shape):
    sh, osh, tl3, tl4, _ = mixed_world
    tl = tl3 if shape == "and3" else tl4
    qt, op = (S.QueryType.Union, O.OP_OR) if shape == "or4" else (S.QueryType.Intersection, O.OP_AND)
    for rt in (S.ResultType.Topk, S.ResultType.TopkCount, S.ResultType.Count):
        got = _both_paths(S, sh, tl, qt, 10, rt, what=shape)
        _oracle(O, osh, got, tl, op, 10, rt, S, (0, 7, len(tl) - 2, len(tl) - 1))


@pytest.mark.parametrize("shape", ["or3", "or4", "and3"])
def test_tombstones_and_not_terms_on_docs_that_pass(S, O, mixed_world, shape):
    """the docs deleted are the unfiltered top-k themselves (they pass every bound) and a random fiftieth; the NOT list is a long one"""
    from seekstorm_amd import _native as N
    sh, osh, tl3, tl4, n_docs = mixed_world
    tl = [t for t in (tl4 if shape == "or4" else tl3) if 4 not in t][:12]
    qt, op = (S.QueryType.Intersection, O.OP_AND) if shape == "and3" else (S.QueryType.Union, O.OP_OR)
    top = _run(S, sh, sh.make_queries(tl, qt), 10, S.ResultType.Topk, N.BM25_PRUNED)
    gone = np.unique(np.concatenate([top[0][top[0] != N.SS_NO_DOC].astype(np.uint64),
                                     np.random.default_rng(3).integers(0, n_docs, n_docs // 50).astype(np.uint64)]))
    nots = [[4] for _ in tl]
    try:
        for with_del, with_not in ((True, False), (False, True), (True, True)):
            sh.set_deleted(gone if with_del else []); osh.set_deleted([int(x) for x in gone] if with_del else [])
            for rt in (S.ResultType.Topk, S.ResultType.TopkCount):
                got = _both_paths(S, sh, tl, qt, 10, rt, nots if with_not else None, what=(shape, with_del, with_not))
                _oracle(O, osh, got, tl, op, 10, rt, S, (0, len(tl) // 2, len(tl) - 1), nots if with_not else None)
                if with_del:
                    assert not set(got[0][got[0] != N.SS_NO_DOC].tolist()) & set(gone.tolist())
    finally:
        sh.set_deleted([]); osh.set_deleted([])


def test_sub_block_bounds_in_force(S, O):
    """weights clustered by doc id (tools/probes/skew_corpus.py, regions of one sub-block): the image turns the per-partition maxima and
    the sub-block skip on by itself for batches of >= 128 queries -- the body's SKIP instantiations, with and without tombstones"""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probes"))
    import skew_corpus
    from seekstorm_amd import _native as N
    n_docs = 150_000
    arrays = skew_corpus.build(O, n_docs, [0.012, 0.035, 0.10, 0.02, 0.3], region_log2=12)
    sh, osh = _shards(S, O, n_docs, *arrays)
    tl = [[0, 1, 2], [2, 4, 0], [0, 2, 3, 1], [4, 3, 2, 1], [1, 3, 4]] * 60
    try:
        for gone in ([], list(range(12288, 12288 + 4096, 3))):  # (a third of one short-doc region, where the top-k lives)
            sh.set_deleted(gone); osh.set_deleted(gone)
            for k in (10, 100):
                q = sh.make_queries(tl, S.QueryType.Union)
                p = _run(S, sh, q, k, S.ResultType.Topk, N.BM25_PRUNED)
                e = _run(S, sh, q, k, S.ResultType.Topk, N.BM25_EXHAUSTIVE)
                _equal(p, e, S.ResultType.Topk, S, ("skip", k, bool(gone)))
                _oracle(O, osh, p, tl, O.OP_OR, k, S.ResultType.Topk, S, (0, 2, 4))
    finally:
        sh.set_deleted([]); osh.set_deleted([])
        sh.close()


# ---- queue edges --------------------------------------------------------------------------------------------------------------------------

EDGES = [(1, 0), (1, 1), (63, 1), (63, 63), (64, 0), (64, 63), (64, 64), (65, 1), (65, 64), (65, 65), (127, 65), (128, 64), (129, 128), (200, 129)]


@pytest.fixture(scope="module")
def edge_world(S, O):
    """For every (n1, n2) of EDGES three lists D < A < C in size: D = 300 docs inside ONE sub-block (one wave reads the whole stream,
    however the partitions are cut), A holds exactly n1 of them, C exactly n2 of those n1.  An intersection [D, A, C] pushes n1 entries to
    the first queue and n2 to the second, so the stream ends with n1 mod 64 and n2 mod 64 entries waiting, after 0 .. 3 full batches;
    its exact count is n2.  One more list E (every doc of the first 12 sub-blocks) makes the 4-term form.  22 sub-blocks."""
    n_docs = 90_000
    rng = np.random.default_rng(8)
    lens = rng.choice([50, 90, 130, 400], n_docs)
    lists = []
    for c, (n1, n2) in enumerate(EDGES):
        sb = c % 11
        d = np.sort(rng.choice(4096, 300, replace=False)) + sb * 4096
        in_a = rng.choice(d, n1, replace=False)
        in_c = rng.choice(in_a, n2, replace=False)
        rest = np.setdiff1d(np.arange(n_docs), d)
        a = np.sort(np.concatenate([in_a, rng.choice(rest, 500, replace=False)]))
        cc = np.sort(np.concatenate([in_c, rng.choice(rest, 1500, replace=False)]))
        for x in (d, a, cc):
            lists.append((x, rng.geometric(0.5, len(x)).clip(1, 60)))
    e = np.arange(12 * 4096)
    lists.append((e, rng.geometric(0.5, len(e)).clip(1, 60)))
    arrays = _hand_corpus(O, n_docs, lens, lists)
    sh, osh = _shards(S, O, n_docs, *arrays)
    yield sh, osh
    sh.close()


@pytest.mark.parametrize("nt", [3, 4])
def test_queue_edges(S, O, edge_world, nt):
    from seekstorm_amd import _native as N
    sh, osh = edge_world
    e_term = 3 * len(EDGES)
    tl = [[3 * c + 2, 3 * c, 3 * c + 1] + ([e_term] if nt == 4 else []) for c in range(len(EDGES))]  # (query order != processing order)
    want = np.array([n2 for _, n2 in EDGES], np.uint64)
    for qt, op in ((S.QueryType.Intersection, O.OP_AND), (S.QueryType.Union, O.OP_OR)):
        is_and = qt == S.QueryType.Intersection
        for k in (10, 100):
            for rt in (S.ResultType.TopkCount, S.ResultType.Topk):
                # the whole set: one launch (14 queries) and staged (300)
                got = _both_paths(S, sh, tl, qt, k, rt, what=("edges", nt, is_and))
                if is_and and rt == S.ResultType.TopkCount:
                    assert np.array_equal(got[3], want)
                    assert np.array_equal(got[2], np.minimum(want, k).astype(np.uint32))
                _oracle(O, osh, got, tl, op, k, rt, S, (0, 6, 9, 13))
        exh = _run(S, sh, sh.make_queries(tl, qt), 10, S.ResultType.TopkCount, N.BM25_EXHAUSTIVE)
        # one-launch batches of 1, 8 and 64 queries through host pointers
        for nq in (1, 8, 64):
            idx = [(5 + i) % len(tl) for i in range(nq)]
            before = sh.one_launch_batches()
            got = _run(S, sh, sh.make_queries([tl[i] for i in idx], qt), 10, S.ResultType.TopkCount, N.BM25_PRUNED)
            assert sh.one_launch_batches() == before + 1
            _equal(got, tuple(x[idx] for x in exh), S.ResultType.TopkCount, S, ("edges, host batch", nq, nt, is_and))
        # a single device-resident query: the staged kernel, many partitions of one sub-block each
        sh.set_strategy(N.BM25_PRUNED)
        try:
            for c in range(len(tl)):
                got = _dev_search(S, sh, sh.make_queries([tl[c]], qt), 10, S.ResultType.TopkCount, _ops(is_and, nt))
                _equal(got, tuple(x[c:c + 1] for x in exh), S.ResultType.TopkCount, S, ("edges, single staged query", c, nt, is_and))
        finally:
            sh.set_strategy(N.BM25_AUTO)
    # intersections under Count
    got = _both_paths(S, sh, tl, S.QueryType.Intersection, 10, S.ResultType.Count, what=("edges, count", nt))
    assert np.array_equal(got[3], want)


# ---- k beyond the number of matches -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [10, 64, 128])
def test_k_larger_than_the_number_of_matches(S, O, edge_world, k):
    sh, osh = edge_world
    e_term = 3 * len(EDGES)
    # intersections with 0, 1, 63, 64 and 65 matches (EDGES' n2), of three and of four lists
    tl = [[3 * c, 3 * c + 1, 3 * c + 2] for c in (0, 1, 3, 6, 9)] + [[3 * c + 1, 3 * c, 3 * c + 2, e_term] for c in (1, 8)]
    for rt in (S.ResultType.Topk, S.ResultType.TopkCount):
        got = _both_paths(S, sh, tl, S.QueryType.Intersection, k, rt, what="k > matches")
        _oracle(O, osh, got, tl, O.OP_AND, k, rt, S, range(len(tl)))
        assert [int(x) for x in got[2]] == [min(k, EDGES[c][1]) for c in (0, 1, 3, 6, 9, 1, 8)]
