"""A SORTED search with its query_facets in one call (ss_bm25_search_sorted_facets; csrc/facet.hip facet_sort_first_kernel; -m gpu).

Yardsticks: the library's own two entries on the same shard, which the other suites pin against the oracle -- the four hit outputs ==
ss_bm25_search_sorted's bit for bit, the counters == ss_bm25_search_facets(SS_RT_COUNT)'s -- and, in shapes A and D, the counters also ==
numpy histograms over the oracle's match sets, built as tests/test_gpu_query_facets.py builds them.  No case skips on SS_ENOTSUP: at
these sizes the default probe budget covers every list; only the refusal test expects that code.  Every case runs with SS_SORT_FUSED
at its default; shape A runs once more in a child process with SS_SORT_FUSED=0."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_query_facets import _oracle, _want_counts
from test_query_facets_host import _spec, host_lib, parse_facets_text

pytestmark = pytest.mark.gpu

OR, AND = "or", "and"
REC = np.dtype([("u8", "u1"), ("u16", "<u2"), ("i32", "<i4"), ("f32", "<f4"), ("u64", "<u8"), ("s16", "<u2"), ("loc", "<u8"), ("u32", "<u4")])
OFF = {n: REC.fields[n][1] for n in REC.names}
BASE, UNIT = (38.8951, 30.25), "km"
WORDS = ["w%03d" % ((i * 37) % 101) for i in range(128)]  # (ids 27 apart share a string: equal ranks)


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


class World:
    pass


def _records(O, n_docs, seed, s16_max=80):
    rng = np.random.default_rng(seed)
    v = np.zeros(n_docs, REC)
    v["u8"] = rng.integers(0, 256, n_docs)
    v["u16"] = rng.integers(0, 65536, n_docs)
    v["i32"] = rng.integers(-(1 << 31), 1 << 31, n_docs)
    f = rng.normal(0.0, 50.0, n_docs)
    v["f32"] = np.where(rng.integers(0, 4, n_docs) == 0, np.array([0.0, -0.0, 1.0, -1.0])[rng.integers(0, 4, n_docs)], f).astype(np.float32)
    v["u64"] = rng.integers(0, 1 << 63, n_docs, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n_docs).astype(np.uint64)
    v["s16"] = rng.integers(0, s16_max, n_docs)
    v["loc"] = O.morton_encode(rng.random(n_docs) * 50.0 + 10.0, rng.random(n_docs) * 60.0 + 5.0)
    v["u32"] = rng.integers(0, 1 << 32, n_docs, dtype=np.uint64)
    return v


def _raw(v):
    return np.ascontiguousarray(v.view(np.uint8).reshape(len(v), v.dtype.itemsize))


def _world(S, O, n_docs, lists, seed, gone=(), v=None, sparse=None, positions=None, shard_id=0, oracle=True):
    """lists: the dense terms' sorted doc arrays; sparse: further lists for the sparse tier; positions: {term: position of its single
    occurrence per posting} -- then every tf is 1 and every other term sits at position 40 + term"""
    rng = np.random.default_rng(seed)
    W = World()
    W.n_docs = n_docs
    W.dl = O.lex_doclen(n_docs)
    lists = [np.asarray(d, np.uint32) for d in lists]
    W.offs = np.concatenate([[0], np.cumsum([len(d) for d in lists])]).astype(np.uint64)
    W.docs = np.concatenate(lists)
    if positions is None:
        W.tfs = np.minimum(rng.geometric(0.6, len(W.docs)), 60).astype(np.uint16)
        pos = None
    else:
        W.tfs = np.ones(len(W.docs), np.uint16)
        pos = np.concatenate([np.asarray(positions[t](d) if t in positions else np.full(len(d), 40 + t), np.uint16) for t, d in enumerate(lists)])
    W.v = _records(O, n_docs, seed + 1) if v is None else v
    W.off = OFF
    W.gone = sorted(gone)
    W.sh = S.Shard(0, shard_id=shard_id)
    W.sh.upload_lexical(n_docs, W.dl, W.offs, W.docs, W.tfs, pos)
    offs, docs, tfs = W.offs, W.docs, W.tfs
    if sparse:
        sl = [np.asarray(d, np.uint32) for d in sparse]
        s_offs = np.concatenate([[0], np.cumsum([len(d) for d in sl])]).astype(np.uint64)
        s_tfs = np.ones(int(s_offs[-1]), np.uint16)
        assert W.sh.append_sparse(s_offs, np.concatenate(sl), s_tfs, positions=None if pos is None else np.full(int(s_offs[-1]), 7, np.uint16)) == len(lists)
        offs, docs, tfs = np.concatenate([offs, offs[-1] + s_offs[1:]]), np.concatenate([docs] + sl), np.concatenate([tfs, s_tfs])
    W.sh.upload_facets(_raw(W.v))
    if W.gone:
        W.sh.set_deleted(W.gone)
    if oracle:
        W.osh = O.Shard(n_docs, W.dl, offs, docs, tfs)
        W.dist = O.geo_distances(W.v["loc"], BASE, UNIT)
    return W


def _make(S, W, qs):
    return W.sh.make_queries([t for _, t, _ in qs], [S.QueryType.Union if op == OR else S.QueryType.Intersection for op, _, _ in qs],
                             [n for _, _, n in qs])


def _ranges(bounds):
    return [("r%d" % i, b) for i, b in enumerate(bounds)]


def _facets(n_strings=64):
    """one facet of every type of the record: u8 (<= 16 buckets: lane-aggregated), u16, i32, f32 around +-0.0, u64, string16, Point"""
    return [
        {"field": "u8", "offset": OFF["u8"], "type": "u8", "ranges": _ranges([1, 50, 200, 255]), "range_type": "within"},
        {"field": "u16", "offset": OFF["u16"], "type": "u16", "ranges": _ranges(list(range(0, 65536, 2048))), "range_type": "within"},
        {"field": "i32", "offset": OFF["i32"], "type": "i32", "ranges": _ranges([-(1 << 31), -1_000_000_000, -5, 0, 7, 1_500_000_000]), "range_type": "within"},
        {"field": "f32", "offset": OFF["f32"], "type": "f32", "ranges": _ranges([-np.inf, -50.0, -1.0, 0.0, 1.0, 25.0]), "range_type": "within"},
        {"field": "u64", "offset": OFF["u64"], "type": "u64", "ranges": _ranges([1 << 20, 1 << 62, 1 << 63, (1 << 64) - 5]), "range_type": "within"},
        {"field": "s16", "offset": OFF["s16"], "type": "string16", "values": ["a%d" % i for i in range(n_strings)], "prefix": "", "length": 10},
        {"field": "loc", "offset": OFF["loc"], "type": "point", "ranges": _ranges([0.0, 500.0, 1000.0, 2000.0, 3000.0]), "range_type": "within",
         "base": BASE, "unit": UNIT},
    ]


def _same(S, W, q, sorts, k, qfs, flt=None, rt=None, what=""):
    """the new entry == the two entries it stands for; -> its outputs"""
    rt = S.ResultType.TopkCount if rt is None else rt
    doc, score, cnt, tot, per = W.sh.search_lexical_sorted_facets(q, sorts, k, qfs, rt, flt)
    d2, s2, c2, t2 = W.sh.search_lexical_sorted_batch(q, sorts, k, flt)
    _, _, _, t3, per3 = W.sh.search_lexical_facets(q, 0, qfs, S.ResultType.Count, flt, reference_shortcuts=False)
    assert np.array_equal(doc, d2), (what, "docs")
    assert np.array_equal(score.view(np.uint32), s2.view(np.uint32)), (what, "scores")
    assert np.array_equal(cnt, c2) and np.array_equal(tot, t2) and np.array_equal(tot, t3), (what, "counts / totals")
    assert len(per) == len(per3) == len(qfs)
    for f, qf in enumerate(qfs):
        assert np.array_equal(per[f], per3[f]), (what, qf["field"], np.argwhere(per[f] != per3[f])[:8])
    return doc, score, cnt, tot, per


# ------------------------------------------------------------------------------------------------ A: bit edges
N_A = 3 * 4096 + 37
NUMERIC = ["u8", "u16", "i32", "f32", "u64"]


def _world_a(S, O):
    rng = np.random.default_rng(41)
    pick = lambda df: np.sort(rng.choice(N_A, int(df * N_A), replace=False))
    lists = [pick(0.5), pick(0.1), pick(0.01), [0, 63, 64, 4095, 4096], [N_A - 1], np.arange(0, N_A, 14), np.arange(7, N_A, 14)]
    return _world(S, O, N_A, lists, 42, gone=[63, 4096, 5000])


def _queries_a(n):
    base = [(OR, [0], []), (OR, [0, 1, 2], []), (AND, [0, 1], []), (OR, [3], []), (OR, [4], []), (AND, [5, 6], []), (OR, [5, 6], [0]),
            (AND, [0, 1], [2]), (OR, [3, 4], []), (OR, [1, 2, 3, 4], [5]), (AND, [0, 5], [1]), (OR, [2], [3])]
    return [base[i % len(base)] for i in range(n)]


def _shape_a(S, O, W):
    qfs = _facets()
    qs65 = _queries_a(65)
    q65 = _make(S, W, qs65)
    want = {}
    for i, qq in enumerate(qs65[:12]):  # the counters of the distinct queries from the oracle's match sets
        md, _, otot = _oracle(W, O, qq, None, 1)
        want[i] = (otot, [_want_counts(W, qf, md) for qf in qfs])
    assert want[5][0] == 0 and want[4][0] == 1 and want[0][0] > 1024 and 0 < want[3][0] <= 5  # the mix is what it says

    def against_oracle(tot, per, n, what):
        for i in range(n):
            otot, counts = want[i % 12]
            assert int(tot[i]) == otot, (what, i)
            for f in range(len(qfs)):
                assert np.array_equal(per[f][i], counts[f]), (what, i, qfs[f]["field"])

    for name in NUMERIC:  # every numeric type both ways (u8: the fused pass is the select's only radix pass; u64: eight passes)
        for desc in (False, True):
            what = ("A sort", name, desc)
            _, _, _, tot, per = _same(S, W, q65, [(OFF[name], name, desc)], 10, qfs, what=what)
            against_oracle(tot, per, 65, what)
    for nq in (1, 3, 64, 65):
        what = ("A nq", nq)
        _, _, _, tot, per = _same(S, W, q65[:nq], [(OFF["u16"], "u16", True)], 10, qfs, what=what)
        against_oracle(tot, per, nq, what)
    for k in (1, 10, 128, 129, 1024, want[2][0] + 3):  # (the last: above the match count of query 2)
        for sort in ([(OFF["u8"], "u8", True)], [(OFF["u64"], "u64", False)]):
            what = ("A k", k, sort[0][1])
            _, _, cnt, tot, per = _same(S, W, q65[:3], sort, k, qfs, what=what)
            against_oracle(tot, per, 3, what)
            assert int(cnt[2]) == min(k, want[2][0])


@pytest.fixture(scope="module")
def WA(S, O):
    W = _world_a(S, O)
    yield W
    W.sh.close()


def test_a_bit_edges(S, O, WA):
    _shape_a(S, O, WA)


def test_a_bit_edges_with_the_fused_pass_switched_off():
    """the same checks in a child process under SS_SORT_FUSED=0 (the switch is read once per process)"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_sorted_facets as t; t.run_shape_a()" % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SS_SORT_FUSED="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shape A ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def run_shape_a():
    import seekstorm_amd
    from oracle import oracle
    assert os.environ.get("SS_SORT_FUSED") == "0"
    W = _world_a(seekstorm_amd, oracle)
    try:
        _shape_a(seekstorm_amd, oracle, W)
    finally:
        W.sh.close()
    print("shape A ok")


# ------------------------------------------------------------------------------------------------ B: slice and level borders
def test_b_slice_and_level_borders_under_tombstones_and_a_filter(S, O):
    n = 70_001  # crosses the 16 384-doc slices of the compaction and the 65 536-doc level
    rng = np.random.default_rng(51)
    edges = [0, 16383, 16384, 32767, 32768, 49151, 49152, 65535, 65536, n - 1]
    lists = [np.sort(rng.choice(n, n // 3, replace=False)), np.sort(rng.choice(n, n // 50, replace=False)), edges, np.arange(16380, 16390),
             np.arange(65530, 65540)]
    W = _world(S, O, n, lists, 52, gone=[16384, 65535, 65536] + list(range(11, n, 89)), oracle=False)
    try:
        flt = [(OFF["u16"], "u16", 10_000, 52_000)]
        qs = [(OR, [0], []), (OR, [2], []), (AND, [0, 1], []), (OR, [3, 4], []), (OR, [1, 2, 3, 4], [0])]
        q = _make(S, W, qs)
        qfs = _facets()
        for f in (None, flt):
            for sort in ([(OFF["i32"], "i32", True)], [(OFF["u16"], "u16", False), (OFF["u8"], "u8", True)]):
                _, _, cnt, tot, _ = _same(S, W, q, sort, 10, qfs, flt=f, what=("B", f is not None, sort))
                assert int(tot[0]) > 10 and int(cnt[0]) == 10
        _, _, _, tot, _ = _same(S, W, q, [(OFF["i32"], "i32", True)], 10, qfs, what="B edges")
        assert int(tot[1]) == len(set(edges) - set(W.gone))
    finally:
        W.sh.close()


# ------------------------------------------------------------------------------------------------ C: two words per thread
def test_c_two_words_per_thread(S, O):
    """the smallest image at which the launch rule gives a 64-query chunk two bitmap words per thread: the rule is
    ceil(groups / 512) * nq >= 2048 with groups = 64 * ceil(n_docs / 4096), i.e. ceil(n_docs / 4096) >= 249 for nq = 64"""
    n = 248 * 4096 + 1
    assert -(-(64 * -(-n // 4096)) // 512) * 64 >= 2048 > -(-(64 * -(-(n - 1) // 4096)) // 512) * 64
    rng = np.random.default_rng(61)
    rec = np.dtype([("u32", "<u4"), ("u8", "u1"), ("s16", "<u2")])
    v = np.zeros(n, rec)
    v["u32"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    v["u8"] = rng.integers(0, 256, n)
    v["s16"] = rng.integers(0, 40, n)
    lists = [np.sort(rng.choice(n, int(df * n), replace=False)) for df in (0.002, 0.001, 0.0005, 0.002)] + [[0, 8191, 8192, n - 1]]
    W = _world(S, O, n, lists, 62, v=v, oracle=False)
    try:
        qfs = [{"field": "u8", "offset": rec.fields["u8"][1], "type": "u8", "ranges": _ranges([0, 64, 128, 192]), "range_type": "within"},
               {"field": "s16", "offset": rec.fields["s16"][1], "type": "string16", "values": ["a%d" % i for i in range(32)], "prefix": "", "length": 10}]
        base = [(OR, [0], []), (OR, [0, 1, 2], []), (AND, [0, 3], []), (OR, [4], []), (OR, [1, 3], [0]), (OR, [2, 4], [])]
        q = _make(S, W, [base[i % len(base)] for i in range(64)])
        _, _, cnt, tot, per = _same(S, W, q, [(rec.fields["u32"][1], "u32", True)], 10, qfs, what="C")
        assert int(tot[0]) == len(lists[0]) and int(tot[3]) == 4 and int(cnt[3]) == 4 and int(per[0][3].sum()) == 4
    finally:
        W.sh.close()


# ------------------------------------------------------------------------------------------------ D: ties
def test_d_ties(S, O):
    n = 9000
    rng = np.random.default_rng(71)
    v = _records(O, n, 72)
    v["u8"] = 7                                             # every doc has the same key
    v["u16"] = np.array([1, 2, 2, 2, 2, 2, 3, 2])[rng.integers(0, 8, n)]  # three values, the middle group far larger than k
    v["f32"] = np.where(rng.integers(0, 2, n) == 0, np.float32(-0.0), np.float32(0.0))
    v["f32"][::50] = rng.normal(0.0, 5.0, len(v["f32"][::50])).astype(np.float32)
    lists = [np.sort(rng.choice(n, n // 2, replace=False)), np.sort(rng.choice(n, n // 10, replace=False))]
    W = _world(S, O, n, lists, 73, v=v, gone=[5, 64])
    try:
        qfs = _facets()
        qs = [(OR, [0], []), (AND, [0, 1], []), (OR, [0, 1], [])]
        q = _make(S, W, qs)
        want = []
        for qq in qs:
            md, _, otot = _oracle(W, O, qq, None, 1)
            want.append((otot, [_want_counts(W, qf, md) for qf in qfs]))
        sorts = [[(OFF["u8"], "u8", False)], [(OFF["u8"], "u8", True)], [(OFF["u16"], "u16", False)], [(OFF["u16"], "u16", True)],
                 [(OFF["f32"], "f32", True)], [(OFF["f32"], "f32", False)], [(OFF["u8"], "u8", False), (OFF["i32"], "i32", True)],
                 [(OFF["u16"], "u16", False), (OFF["i32"], "i32", False)], [(OFF["f32"], "f32", True), (OFF["u64"], "u64", True)]]
        for sort in sorts:
            for k in (10, 200):
                doc, _, cnt, tot, per = _same(S, W, q, sort, k, qfs, what=("D", sort, k))
                for i in range(len(qs)):
                    assert int(tot[i]) == want[i][0] and int(cnt[i]) == k
                    for f in range(len(qfs)):
                        assert np.array_equal(per[f][i], want[i][1][f]), (sort, k, i, qfs[f]["field"])
                if len(sort) == 2 and sort[0][1] == "u8":  # the second field decides alone: strictly ordered by it
                    x = v["i32"][doc[0][:cnt[0]]].astype(np.int64)
                    assert np.all(x[:-1] >= x[1:])
    finally:
        W.sh.close()


# ------------------------------------------------------------------------------------------------ E: LDS budget
def test_e_lds_budget(S, O):
    n = 20_011
    rng = np.random.default_rng(81)
    lists = [np.sort(rng.choice(n, n // 2, replace=False)), np.sort(rng.choice(n, n // 20, replace=False))]
    W = _world(S, O, n, lists, 82, v=_records(O, n, 83, s16_max=2100), oracle=False)
    try:
        strings = lambda m: {"field": "s%d" % m, "offset": OFF["s16"], "type": "string16", "values": ["a%d" % i for i in range(m)], "prefix": "", "length": 10}
        small = {"field": "u8", "offset": OFF["u8"], "type": "u8", "ranges": _ranges(list(range(0, 240, 16))), "range_type": "within"}  # 15 buckets
        assert len(small["ranges"]) == 15
        q = _make(S, W, [(OR, [0], []), (AND, [0, 1], []), (OR, [0, 1], [])])
        # 2047 ids + "other" = 2048 LDS counters exactly; 2048 ids: global memory; the small one: lane-aggregated, LDS already full
        _same(S, W, q, [(OFF["u32"], "u32", True)], 10, [strings(2047), strings(2048), small], what="E strings first")
        # 16 + 2032 = 2048 exactly, the small one in LDS; 2048 ids beside them in global memory
        _same(S, W, q, [(OFF["i32"], "i32", False)], 10, [small, strings(2031), strings(2048)], what="E small first")
    finally:
        W.sh.close()


# ------------------------------------------------------------------------------------------------ F: other key sources
def test_f_string_rank_and_point_sorts(S, O, WA):
    W = WA
    qfs = _facets()
    q = _make(S, W, _queries_a(12))
    W.sh.set_string_facet_ranks(OFF["s16"], "string16", WORDS)
    for sort in ([(OFF["s16"], "string16", False), (OFF["i32"], "i32", True)], [(OFF["s16"], "string16", True), (OFF["u8"], "u8", False)],
                 [(OFF["loc"], "point", False, BASE)], [(OFF["loc"], "point", True, (10.0, 20.0))]):
        for k in (10, 300):
            _same(S, W, q, sort, k, qfs, what=("F", sort, k))


# ------------------------------------------------------------------------------------------------ G: mixed chunk
def test_g_plain_phrase_and_sparse_tier_in_one_chunk(S, O):
    n = 12_325
    rng = np.random.default_rng(91)
    lists = [np.sort(rng.choice(n, n // 3, replace=False)), np.sort(rng.choice(n, n // 4, replace=False)), np.sort(rng.choice(n, n // 20, replace=False))]
    sparse = [np.sort(rng.choice(n, 40, replace=False)), [3, 64, 4097, n - 1]]
    # term 0 sits at position 0; term 1 at position 1 in even docs, 5 in odd ones: the phrase [0, 1] matches the even docs of both lists
    positions = {0: lambda d: np.zeros(len(d)), 1: lambda d: np.where(d % 2 == 0, 1, 5)}
    W = _world(S, O, n, lists, 92, positions=positions, sparse=sparse, oracle=False)
    try:
        plain = _make(S, W, [(OR, [0, 2], []), (AND, [0, 1], [])])
        phrase = W.sh.make_queries([[0, 1]], S.QueryType.Phrase)
        tiered = _make(S, W, [(OR, [2, 3], []), (OR, [4], [])])
        q = np.concatenate([plain[:1], phrase, tiered[:1], plain[1:], tiered[1:]])
        qfs = _facets()
        for sort in ([(OFF["u16"], "u16", True)], [(OFF["u8"], "u8", False), (OFF["f32"], "f32", True)]):
            _, _, _, tot, _ = _same(S, W, q, sort, 10, qfs, what=("G", sort))
            both = np.intersect1d(lists[0], lists[1])
            assert int(tot[1]) == int((both % 2 == 0).sum()) and int(tot[3]) == len(both) and int(tot[4]) == 4
    finally:
        W.sh.close()


# ------------------------------------------------------------------------------------------------ H: delegation, deep page, result types
def test_h_deep_page_result_types_and_delegations(S, O, WA):
    W = WA
    qfs = _facets()
    qs = _queries_a(5)
    q = _make(S, W, qs)
    sort = [(OFF["u16"], "u16", True), (OFF["i32"], "i32", False)]
    flt = [(OFF["u8"], "u8", 16, 240)]
    for f in (None, flt):  # a deep page: the facets once, then the passes of the sorted entry
        _, _, cnt, tot, _ = _same(S, W, q, sort, 1500, qfs, flt=f, what=("H deep", f is not None))
        assert int(cnt[0]) == 1500 < int(tot[0]) and int(cnt[3]) == int(tot[3]) < 10
    full = _same(S, W, q, sort, 10, qfs, what="H topkcount")
    topk = W.sh.search_lexical_sorted_facets(q, sort, 10, qfs, S.ResultType.Topk)
    for a, b in zip(full[:4], topk[:4]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert all(np.array_equal(a, b) for a, b in zip(full[4], topk[4]))  # Topk: counted all the same
    # Count: no docs, no select; the doc outputs may be NULL
    from seekstorm_amd import _native as N
    n_sorts, sarr = W.sh._result_sorts(sort)
    off, ty, nb, allb, bases, stride = W.sh._query_facet_args(qfs)
    cnt, tot, out = np.zeros(len(q), np.uint32), np.zeros(len(q), np.uint64), np.zeros((len(q), stride), np.uint64)
    rc = N.lib().ss_bm25_search_sorted_facets(W.sh._h, len(q), q.ctypes.data_as(C.c_void_p), n_sorts, C.cast(sarr, C.c_void_p), 0, int(S.ResultType.Count),
                                              0, None, len(qfs), N.ptr(off, N.u32p), N.ptr(ty, N.u32p), N.ptr(nb, N.u32p), N.ptr(allb, N.u64p),
                                              C.cast(bases, C.c_void_p), None, None, N.ptr(cnt, N.u32p), N.ptr(tot, N.u64p), N.ptr(out, N.u64p))
    assert rc == 0 and np.array_equal(tot, full[3]) and np.array_equal(out, np.concatenate(full[4], axis=1))
    # n_sorts = 0: ss_bm25_search_facets; n_facets = 0: ss_bm25_search_sorted
    d1, s1, c1, t1, p1 = W.sh.search_lexical_sorted_facets(q, [], 10, qfs, S.ResultType.TopkCount, flt)
    d2, s2, c2, t2, p2 = W.sh.search_lexical_facets(q, 10, qfs, S.ResultType.TopkCount, flt, reference_shortcuts=False)
    assert np.array_equal(d1, d2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32)) and np.array_equal(c1, c2) and np.array_equal(t1, t2)
    assert all(np.array_equal(a, b) for a, b in zip(p1, p2))
    d1, s1, c1, t1, p1 = W.sh.search_lexical_sorted_facets(q, sort, 10, [], S.ResultType.TopkCount, flt)
    d2, s2, c2, t2 = W.sh.search_lexical_sorted_batch(q, sort, 10, flt)
    assert p1 == [] and np.array_equal(d1, d2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32)) and np.array_equal(c1, c2) and np.array_equal(t1, t2)


# ------------------------------------------------------------------------------------------------ I: refusals
def _raw_call(S, sh, q, sorts, k=10, rt=2, n_sorts=None, qfs=None, n_facets=None, ty=None, nb=None, off=None, bounds="own", bases="own", outs=True,
              null_queries=False, nq=None):
    from seekstorm_amd import _native as N
    qfs = _facets()[:3] + _facets()[6:] if qfs is None else qfs  # (u8, u16, i32, Point)
    ns, sarr = S.Shard._result_sorts(sorts)
    o, t, b, allb, bs, stride = sh._query_facet_args(qfs)
    o = o if off is None else np.asarray(off, np.uint32)
    t = t if ty is None else np.asarray(ty, np.uint32)
    b = b if nb is None else np.asarray(nb, np.uint32)
    allb = allb if bounds == "own" else bounds
    bs = bs if bases == "own" else bases
    n = len(q) if nq is None else nq
    doc, score = np.zeros((max(n, 1), max(k, 1)), np.uint32), np.zeros((max(n, 1), max(k, 1)), np.float32)
    cnt, tot, out = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint64), np.zeros((max(n, 1), stride + 4096), np.uint64)
    return N.lib().ss_bm25_search_sorted_facets(sh._h, n, None if null_queries else q.ctypes.data_as(C.c_void_p), ns if n_sorts is None else n_sorts,
                                                C.cast(sarr, C.c_void_p), k, rt, 0, None, len(qfs) if n_facets is None else n_facets, N.ptr(o, N.u32p),
                                                N.ptr(t, N.u32p), N.ptr(b, N.u32p), N.ptr(allb, N.u64p), None if bs is None else C.cast(bs, C.c_void_p),
                                                N.ptr(doc, N.u32p) if outs else None, N.ptr(score, N.f32p) if outs else None, N.ptr(cnt, N.u32p),
                                                N.ptr(tot, N.u64p), N.ptr(out, N.u64p))


def test_i_refusals(S, O, WA):
    from seekstorm_amd import _native as N
    W = WA
    q = _make(S, W, _queries_a(3))
    sort = [(OFF["i32"], "i32", True)]
    call = lambda **kw: _raw_call(S, W.sh, kw.pop("q", q), kw.pop("sorts", sort), **kw)
    assert call() == N.SS_OK  # (the arguments the cases below vary are valid)
    # SS_EINVAL: both entries' argument checks
    assert call(rt=3) == N.SS_EINVAL
    assert call(null_queries=True) == N.SS_EINVAL
    assert call(nq=0) == N.SS_EINVAL
    assert call(k=0) == N.SS_EINVAL
    assert call(outs=False) == N.SS_EINVAL
    doc = np.zeros((3, 10), np.uint32)
    assert call(ty=[13, 1, 6, 12]) == N.SS_EINVAL                      # a facet type beyond SS_FACET_POINT
    assert call(bases=None) == N.SS_EINVAL                            # a Point facet without bases
    assert call(bounds=None) == N.SS_EINVAL                           # bounds missing
    assert call(nb=[0, 32, 6, 5]) == N.SS_EINVAL                      # no buckets
    assert call(nb=[(1 << 24) + 1, 32, 6, 5]) == N.SS_EINVAL
    many = [_facets()[0]] * (N.SS_MAX_QUERY_FACETS + 1)
    assert call(qfs=many) == N.SS_EINVAL
    # SS_ENOTSUP: more sort fields than the call takes; a string sort field without a rank table
    five = [(OFF["u8"], "u8", True)] * (N.SS_MAX_SORT_FIELDS + 1)
    assert call(sorts=five) == N.SS_ENOTSUP
    fresh = _world(S, O, 5000, [np.arange(0, 5000, 3), np.arange(0, 5000, 7)], 17, oracle=False)
    bare = S.Shard(0)
    try:
        qf = fresh.sh.make_queries([[0, 1]], S.QueryType.Union)
        assert _raw_call(S, fresh.sh, qf, [(OFF["s16"], "string16", False)]) == N.SS_ENOTSUP
        assert _raw_call(S, fresh.sh, qf, [(OFF["s16"], "string16", False)], rt=0) == N.SS_ENOTSUP  # (checked for SS_RT_COUNT too)
        # a sort type beyond SS_FACET_POINT
        ns, sarr = S.Shard._result_sorts(sort)
        sarr[0].facet_type = 13
        cnt, tot = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
        assert N.lib().ss_bm25_search_sorted_facets(fresh.sh._h, 1, qf.ctypes.data_as(C.c_void_p), 1, C.cast(sarr, C.c_void_p), 10, 2, 0, None, 0, None, None,
                                                    None, None, None, N.ptr(doc, N.u32p), N.ptr(doc.view(np.float32), N.f32p), N.ptr(cnt, N.u32p),
                                                    N.ptr(tot, N.u64p), None) == N.SS_EINVAL
        # SS_ESTATE: an offset beyond the record (a sort field's, a facet's); facet records for fewer docs than the image; no image
        assert _raw_call(S, fresh.sh, qf, [(REC.itemsize - 3, "i32", True)]) == N.SS_ESTATE
        assert _raw_call(S, fresh.sh, qf, sort, off=[OFF["u8"], OFF["u16"], REC.itemsize - 3, OFF["loc"]]) == N.SS_ESTATE
        assert _raw_call(S, fresh.sh, qf, sort, k=1500, off=[OFF["u8"], OFF["u16"], REC.itemsize - 3, OFF["loc"]]) == N.SS_ESTATE  # (deep page)
        fresh.sh.upload_facets(_raw(fresh.v[:4000]))
        assert _raw_call(S, fresh.sh, qf, sort) == N.SS_ESTATE
        assert _raw_call(S, bare, qf, sort) == N.SS_ESTATE
        # SS_ENOTSUP for the whole call: one phrase on an image without positions inside a batch
        ph = W.sh.make_queries([[0, 1]], S.QueryType.Phrase)
        assert call(q=np.concatenate([q, ph])) == N.SS_ENOTSUP
        assert call() == N.SS_OK  # (and the shard answers the next call)
    finally:
        fresh.sh.close()
        bare.close()


# ------------------------------------------------------------------------------------------------ J: Index.search over two shards
def _cpp(shards, which, terms, qt, offset, length, rt, sorts, qfs, flt_arr, n_flt):
    u32p = C.POINTER(C.c_uint32)
    H = host_lib()
    H.ssh_index_adopt.restype = C.c_void_p
    H.ssh_index_adopt.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    H.ssh_index_destroy.argtypes = [C.c_void_p]
    H.ssh_index_search_sorted_facets.restype = C.c_int
    H.ssh_index_search_sorted_facets.argtypes = [C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                 C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p,
                                                 C.c_uint32, C.POINTER(C.c_int)]
    H.ssh_index_search_sorted.restype = C.c_int
    H.ssh_index_search_sorted.argtypes = [C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    H.ssh_index_search_facets.restype = C.c_int
    H.ssh_index_search_facets.argtypes = [C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_char_p,
                                          C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_int)]
    handles = (C.c_void_p * len(shards))(*[sh._h for sh in shards])
    ix = H.ssh_index_adopt(len(shards), handles, (C.c_int * len(shards))(*([0] * len(shards))))
    try:
        t = np.asarray(terms, np.uint32)
        cap = offset + length
        doc, score, meta = np.zeros(cap, np.uint64), np.zeros(cap, np.float32), np.zeros(4, np.uint64)
        buf = C.create_string_buffer(1 << 20)
        flen = C.c_int(0)
        _, sarr = S_result_sorts(sorts)
        fp = None if flt_arr is None else C.cast(flt_arr, C.c_void_p)
        if which == "both":
            n = H.ssh_index_search_sorted_facets(ix, t.ctypes.data_as(u32p), len(t), int(qt), offset, length, int(rt), n_flt, fp, C.cast(sarr, C.c_void_p),
                                                 len(sorts), _spec(qfs), cap, doc.ctypes.data, score.ctypes.data, meta.ctypes.data, buf, len(buf),
                                                 C.byref(flen))
        elif which == "sorted":
            n = H.ssh_index_search_sorted(ix, t.ctypes.data_as(u32p), len(t), int(qt), offset, length, n_flt, fp, C.cast(sarr, C.c_void_p), len(sorts), cap,
                                          doc.ctypes.data, score.ctypes.data, meta.ctypes.data)
        else:
            n = H.ssh_index_search_facets(ix, t.ctypes.data_as(u32p), len(t), int(qt), offset, length, int(rt), n_flt, fp, _spec(qfs), cap, doc.ctypes.data,
                                          score.ctypes.data, meta.ctypes.data, buf, len(buf), C.byref(flen))
        assert n >= 0 and flen.value >= 0 and int(meta[3]) == 0, (which, n, flen.value, meta)
        return doc[:n].copy(), score[:n].copy(), int(meta[1]), parse_facets_text(buf.value.decode())
    finally:
        H.ssh_index_destroy(ix)


def S_result_sorts(sorts):
    """(n, array) laid out as host_capi's ssh_result_sort: the same 32 bytes as ss_result_sort"""
    import seekstorm_amd
    return seekstorm_amd.Shard._result_sorts(sorts)


def test_j_index_search_over_two_shards(S, O, WA):
    n1 = 9001
    rng = np.random.default_rng(101)
    lists = [np.sort(rng.choice(n1, int(df * n1), replace=False)) for df in (0.5, 0.1, 0.01)] + [[0, 63, 64, 4095, 4096], [n1 - 1],
                                                                                                 np.arange(0, n1, 14), np.arange(7, n1, 14)]
    W1 = _world(S, O, n1, lists, 102, gone=[1, 64], shard_id=1, oracle=False)
    try:
        ix = S.Index([WA.sh, W1.sh])
        qfs = _facets()
        qfs[5] = dict(qfs[5], prefix="a1", length=7)
        qfs[2] = dict(qfs[2], range_type="above")
        flt = [(OFF["u8"], "u8", 16, 240)]
        farr, nflt = WA.sh.facet_filters(flt)
        TC = S.ResultType.TopkCount
        for terms, qt, neg in (([0, 1, 2], S.QueryType.Union, []), ([0, 1], S.QueryType.Intersection, []), ([3, 4], S.QueryType.Union, []),
                               ([5, 6], S.QueryType.Intersection, []), ([0, 5], S.QueryType.Union, [1])):
            for sort in ([(OFF["u16"], "u16", True)], [(OFF["u8"], "u8", False), (OFF["f32"], "f32", True)]):
                for offset, length, f in ((0, 10, None), (5, 20, flt)):
                    kw = dict(query_type_default=qt, offset=offset, length=length, not_terms=neg, facet_filter=f)
                    ro = ix.search(terms, result_sort=sort, query_facets=qfs, **kw)
                    hits = ix.search(terms, result_sort=sort, **kw)
                    fac = ix.search(terms, query_facets=qfs, strict=True, **kw)
                    what = (terms, sort, offset)
                    assert [(r.doc_id, r.score) for r in ro.results] == [(r.doc_id, r.score) for r in hits.results], what
                    assert ro.result_count_total == hits.result_count_total == fac.result_count_total and ro.result_count == hits.result_count, what
                    assert ro.facets == fac.facets and (ro.facets or not ro.result_count_total), what
                    if neg:
                        continue  # (the C++ entries of this comparison take no NOT terms)
                    fa, na = (farr, nflt) if f else (None, 0)
                    bd, bs, bt, bf = _cpp([WA.sh, W1.sh], "both", terms, qt, offset, length, TC, sort, qfs, fa, na)
                    sd, ss, st, _ = _cpp([WA.sh, W1.sh], "sorted", terms, qt, offset, length, TC, sort, qfs, fa, na)
                    _, _, ft, ff = _cpp([WA.sh, W1.sh], "facets", terms, qt, offset, length, TC, sort, qfs, fa, na)
                    assert np.array_equal(bd, sd) and np.array_equal(bs.view(np.uint32), ss.view(np.uint32)) and bt == st == ft, ("c++",) + what
                    assert bf == ff, ("c++",) + what
                    assert bd.tolist() == [r.doc_id for r in ro.results], ("c++ == python",) + what
        ro = ix.search([0, 1, 2], result_sort=[(OFF["u16"], "u16", True)], query_facets=qfs, result_type=S.ResultType.Topk)
        assert ro.facets == {} and ro.result_count == 10  # search.rs:1748
        ro = ix.search([0, 1, 2], result_sort=[(OFF["u16"], "u16", True)], query_facets=qfs, result_type=S.ResultType.Count)
        fac = ix.search([0, 1, 2], query_facets=qfs, result_type=S.ResultType.Count, strict=True)
        assert ro.results == [] and ro.facets == fac.facets and ro.result_count_total == fac.result_count_total > 0
        for mode in (S.SearchMode.Hybrid, S.SearchMode.Vector):
            with pytest.raises(ValueError):
                ix.search([0, 1], np.zeros(4, np.float32), search_mode=mode, result_sort=[(OFF["u16"], "u16", True)], query_facets=qfs)
    finally:
        W1.sh.close()
