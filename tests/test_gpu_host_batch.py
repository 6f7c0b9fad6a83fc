"""Host-pointer BM25 batches of more than 256 queries (the staged pipeline of ss_bm25_search: queries packed on the host --
csrc/bm25_pack.h --, expanded from the packed form through LDS, phrase batches in the full form, answers home through the pinned
block).  Every answer is compared BIT FOR BIT with ss_bm25_search_dev on the same queries (device-resident queries in the full
form, answers left on the device), one case with the CPU oracle too."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_DOCS = 300_000
# list 8 and 9: fewer docs than the larger k's (rows padded, counts below k)
DFS = [0.004, 0.012, 0.03, 0.05, 0.09, 0.15, 0.0005, 0.22, 0.00004, 0.000025]


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _corpus(O, seed=29):
    rng = np.random.default_rng(seed)
    lens = np.clip(np.round(np.exp(np.log(120) + 0.6 * rng.standard_normal(N_DOCS))), 8, 2000).astype(np.int64)
    lut = {int(x): int(O.lib().so_int_to_byte4(int(x))) for x in np.unique(lens)}
    doclen = np.array([lut[int(x)] for x in lens], np.uint8)
    offs, docs, tfs, term_of = [0], [], [], []
    for t, df in enumerate(DFS):
        n = max(1, int(round(df * N_DOCS)))
        docs.append(np.sort(rng.choice(N_DOCS, n, replace=False)).astype(np.uint32))
        tfs.append(rng.geometric(0.55, n).clip(1, 300).astype(np.uint16))
        term_of.append(np.full(n, t, np.int64))
        offs.append(offs[-1] + n)
    docs, tfs, term_of = np.concatenate(docs), np.concatenate(tfs), np.concatenate(term_of)
    # positions: occurrence j of term t stands at 8 j + t, so term t + 1 follows term t wherever a doc holds both
    start = np.cumsum(tfs.astype(np.int64)) - tfs
    j = np.arange(int(tfs.sum()), dtype=np.int64) - np.repeat(start, tfs)
    positions = (8 * j + np.repeat(term_of, tfs)).astype(np.uint16)
    return doclen, np.asarray(offs, np.uint64), docs, tfs, positions


@pytest.fixture(scope="module")
def world(S, O):
    dl, offs, docs, tfs, positions = _corpus(O)
    sh = S.Shard(0)
    sh.upload_lexical(N_DOCS, dl, offs, docs, tfs, positions)
    osh = O.Shard(N_DOCS, dl, offs, docs, tfs)
    yield sh, osh
    sh.close()


def _dev(sh, q, k, rt, ops):
    """device-resident queries and answers: ss_bm25_search_dev"""
    import ctypes as C
    import torch
    from seekstorm_amd import _native as N
    dev = torch.device("cuda", 0)
    nq, kk = len(q), max(k, 1)
    qd = torch.from_numpy(q.view(np.uint8).reshape(nq, -1).copy()).to(dev)
    o_doc = torch.zeros((nq, kk), dtype=torch.int32, device=dev); o_score = torch.zeros((nq, kk), dtype=torch.float32, device=dev)
    o_cnt = torch.zeros((nq,), dtype=torch.int32, device=dev); o_tot = torch.zeros((nq,), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev)
    N.check(N.lib().ss_bm25_search_dev(sh._h, nq, qd.data_ptr(), k, int(rt), ops, o_doc.data_ptr(), o_score.data_ptr(), o_cnt.data_ptr(),
                                       o_tot.data_ptr(), C.c_void_p(st.cuda_stream)), "ss_bm25_search_dev")
    torch.cuda.synchronize()
    return (o_doc.cpu().numpy().view(np.uint32), o_score.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint32), o_tot.cpu().numpy().view(np.uint64))


def _ops(S, lists, nots, qts):
    """the batch's description for the device entry, as the host path works it out from the queries"""
    has_and = any(int(qt) != int(S.QueryType.Union) and len(tl) > 1 for tl, qt in zip(lists, qts))
    has_or = any(int(qt) == int(S.QueryType.Union) and len(tl) > 1 for tl, qt in zip(lists, qts))
    np_max, nn_max = max(len(tl) for tl in lists), max(len(nl) for nl in nots)
    nt_max = max(len(tl) + len(nl) for tl, nl in zip(lists, nots))
    if nn_max and nt_max == np_max:
        nt_max += 1  # "the batch holds NOT terms" travels as nt > np
    phrase = any(int(qt) == int(S.QueryType.Phrase) for qt in qts)
    return (1 if has_and else 0) | (2 if has_or or not has_and else 0) | (16 if phrase else 0) | (nt_max << 8) | (np_max << 16) | (nn_max << 24)


def _same(S, got, ref, rt, what):
    assert np.array_equal(got[2], ref[2]), ("count", what)
    if rt != S.ResultType.Count:  # whole rows, padding included
        assert np.array_equal(got[0], ref[0]), ("doc", what)
        assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), ("score", what)
    if rt != S.ResultType.Topk:
        assert np.array_equal(got[3], ref[3]), ("total", what)


def _batch(S, sh, lists, nots=None, qts=None):
    nots = nots if nots is not None else [[] for _ in lists]
    qts = qts if qts is not None else [S.QueryType.Union] * len(lists)
    return sh.make_queries(lists, qts, nots), _ops(S, lists, nots, qts)


def _check(S, sh, lists, k, rt, nots=None, qts=None, what=None):
    q, ops = _batch(S, sh, lists, nots, qts)
    before = sh.one_launch_batches()
    got = sh.search_lexical_batch(q, k, rt, reference_shortcuts=False)
    assert sh.one_launch_batches() == before, "a batch of more than 256 queries took the one-launch path"
    _same(S, got, _dev(sh, q, k, rt, ops), rt, what)
    return got


def _terms(rng, n, lo, hi, n_lists=8):
    """n term lists of lo .. hi terms out of the first n_lists lists"""
    return [[int(x) for x in rng.choice(n_lists, int(rng.integers(lo, hi + 1)), replace=False)] for _ in range(n)]


@pytest.mark.parametrize("nq", [257, 258, 259, 385])
def test_batch_sizes_k_and_result_types(S, world, nq):
    """257: the first staged size; 258 / 259: a merge block of four queries partly filled; 385: expansion blocks partly filled.
    k = 1, 10, 32: the tournament merge; 33, 64: the merge tree; Count: no lists."""
    sh, _ = world
    rng = np.random.default_rng(nq)
    lists = _terms(rng, nq, 1, 4)
    for k in (1, 10, 32, 33, 64):
        for rt in (S.ResultType.Topk, S.ResultType.TopkCount):
            _check(S, sh, lists, k, rt, what=(nq, k, rt))
    _check(S, sh, lists, 10, S.ResultType.Count, what=(nq, "count"))


def test_one_term_queries(S, world):
    sh, _ = world
    rng = np.random.default_rng(1)
    for k in (10, 33):
        _check(S, sh, _terms(rng, 300, 1, 1), k, S.ResultType.TopkCount, what=("W=1", k))


def test_intersections_and_mixed_operators(S, world):
    sh, _ = world
    rng = np.random.default_rng(2)
    lists = _terms(rng, 300, 2, 3)
    for qts in ([S.QueryType.Intersection] * 300, [S.QueryType.Intersection if i % 3 else S.QueryType.Union for i in range(300)]):
        for k in (10, 33):
            _check(S, sh, lists, k, S.ResultType.TopkCount, qts=qts, what=("and", k))


def test_widest_query_has_not_terms(S, world):
    """W = n_terms + NOT terms of a query that is not the one with the most scored terms"""
    sh, _ = world
    rng = np.random.default_rng(3)
    lists = _terms(rng, 300, 1, 3, n_lists=6)
    nots = [[] for _ in lists]
    lists[17], nots[17] = [0, 1], [6, 7]   # 4 slots; nobody else has more than 3
    lists[299], nots[299] = [2], [7]
    for k in (10, 64):
        for rt in (S.ResultType.Topk, S.ResultType.TopkCount):
            _check(S, sh, lists, k, rt, nots=nots, what=("not", k, rt))


def test_five_term_query_in_the_batch(S, world):
    """one query of five terms sends the batch to the scan kernels: W = 5, the expansion must still be right"""
    sh, _ = world
    rng = np.random.default_rng(4)
    lists = _terms(rng, 260, 1, 4)
    lists[259] = [0, 1, 2, 3, 4]
    for k in (10, 33):
        _check(S, sh, lists, k, S.ResultType.TopkCount, what=("five", k))


def test_fewer_matches_than_k(S, world):
    """unions of the two tiny lists: counts below k, rows padded with SS_NO_DOC / 0 -- by the tournament merge (k = 32) and by the tree (k = 64)"""
    sh, _ = world
    from seekstorm_amd import _native as N
    rng = np.random.default_rng(5)
    lists = _terms(rng, 257, 1, 3)
    lists[0], lists[128], lists[256] = [8, 9], [9], [8]
    for k in (32, 64):
        d, s, c, t = _check(S, sh, lists, k, S.ResultType.TopkCount, what=("short", k))
        for i in (0, 128, 256):
            assert 0 < int(c[i]) < k and int(c[i]) == int(t[i])
            assert np.all(d[i][int(c[i]):] == N.SS_NO_DOC) and np.all(s[i][int(c[i]):] == 0.0)


def test_phrase_query_in_the_batch(S, world):
    """one phrase among 300 unions: the batch runs as two (the phrase part in the full form), the answers come back in place"""
    sh, _ = world
    rng = np.random.default_rng(6)
    lists = _terms(rng, 301, 1, 3)
    lists[100] = [3, 4]  # term 4 follows term 3 in every doc that holds both (_corpus)
    qts = [S.QueryType.Union] * 301
    qts[100] = S.QueryType.Phrase
    q = sh.make_queries(lists, qts)
    rest = [i for i in range(301) if i != 100]
    for k in (10, 33):
        got = sh.search_lexical_batch(q, k, S.ResultType.TopkCount, reference_shortcuts=False)
        ref_u = _dev(sh, q[rest], k, S.ResultType.TopkCount, _ops(S, [lists[i] for i in rest], [[]] * 300, [S.QueryType.Union] * 300))
        ref_p = _dev(sh, q[100:101], k, S.ResultType.TopkCount, _ops(S, [lists[100]], [[]], [S.QueryType.Phrase]))
        assert int(ref_p[2][0]) > 0
        _same(S, tuple(a[rest] for a in got), ref_u, S.ResultType.TopkCount, ("phrase batch, unions", k))
        _same(S, tuple(a[100:101] for a in got), ref_p, S.ResultType.TopkCount, ("phrase batch, phrase", k))


def test_calls_back_to_back_on_one_shard(S, world):
    """the flag sequence, the pinned answer block (layout, growth) and the query staging across calls of changing size, k and merge"""
    sh, _ = world
    rng = np.random.default_rng(7)
    a, b, big = _terms(rng, 385, 1, 4), _terms(rng, 257, 1, 2), _terms(rng, 1100, 1, 3)
    T, TC = S.ResultType.Topk, S.ResultType.TopkCount
    for step, (lists, k, rt) in enumerate(((a, 32, TC), (b, 1, T), (a, 32, T),        # tournament merge, sizes and k change
                                           (a, 33, TC), (b, 10, TC), (a, 64, T),      # tree / merge / tree
                                           (b, 10, S.ResultType.Count), (a, 10, TC),
                                           (big, 32, TC), (b, 32, TC), (big, 64, T))):  # both staging blocks grow
        _check(S, sh, lists, k, rt, what=("step", step))


def test_error_code_and_the_call_after(S, world):
    sh, _ = world
    from seekstorm_amd import _native as N
    rng = np.random.default_rng(8)
    lists = _terms(rng, 300, 1, 3)
    q, ops = _batch(S, sh, lists)
    bad = q.copy()
    bad["term"][211, 0] = len(DFS) + 5  # no such term
    for k in (10, 33):
        with pytest.raises(N.SeekStormHipError) as e:
            sh.search_lexical_batch(bad, k, S.ResultType.TopkCount, reference_shortcuts=False)
        assert e.value.code == N.SS_EINVAL
        got = sh.search_lexical_batch(q, k, S.ResultType.TopkCount, reference_shortcuts=False)
        _same(S, got, _dev(sh, q, k, S.ResultType.TopkCount, ops), S.ResultType.TopkCount, ("after the error", k))


def test_two_host_threads_on_one_shard(S, world):
    sh, _ = world
    rng = np.random.default_rng(9)
    sets = [[_terms(rng, 300, 1, 3) for _ in range(3)] for _ in range(2)]
    batches = [[_batch(S, sh, lists) for lists in mine] for mine in sets]
    refs = [[_dev(sh, q, 10, S.ResultType.TopkCount, ops) for q, ops in mine] for mine in batches]
    got = [[None] * 3 for _ in range(2)]

    def run(t):
        for _ in range(2):
            for j, (q, _ops_) in enumerate(batches[t]):
                got[t][j] = sh.search_lexical_batch(q, 10, S.ResultType.TopkCount, reference_shortcuts=False)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t in range(2):
        for j in range(3):
            _same(S, got[t][j], refs[t][j], S.ResultType.TopkCount, ("thread", t, j))


def test_against_the_oracle(S, O, world):
    sh, osh = world
    rng = np.random.default_rng(10)
    lists = _terms(rng, 257, 1, 3)
    lists[1] = [8, 9]
    k = 10
    d, s, c, t = _check(S, sh, lists, k, S.ResultType.TopkCount, what="oracle")
    for i in range(8):
        od, os_, otot = osh.search_exhaustive(lists[i], O.OP_OR, k)
        n = int(c[i])
        assert n == len(od) and int(t[i]) == otot, (i, n, len(od))
        assert np.allclose(s[i][:n], os_, rtol=1e-4)
        if n:  # ids outside the k-th score's tie band
            band = abs(float(os_[-1])) * 2e-4
            clear = lambda dd, ss: {int(x) for x, y in zip(dd, ss) if y > os_[-1] + band}
            assert clear(d[i][:n], s[i][:n]) <= set(od.tolist()) and clear(od, os_) <= set(d[i][:n].tolist())
