"""A sorted search with its query_facets on the host, no device: the symbol's declarations, and Index.search(result_sort=...,
query_facets=...) of the Python mirror over stub shards -- every shard asked once through search_lexical_sorted_facets, the sorted
hits merged as the result_sort branch merges them, the counters through finish_facets / merge_facets."""
import os

import numpy as np
import pytest

from seekstorm_amd.search import Index, QueryType, ResultType, SearchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_declared_everywhere():
    from seekstorm_amd import _native as N
    assert "ss_bm25_search_sorted_facets" in [name for name, _, _ in N.SYMBOLS]
    args = [a for name, _, a in N.SYMBOLS if name == "ss_bm25_search_sorted_facets"][0]
    assert len(args) == 20
    header = open(os.path.join(ROOT, "include", "seekstorm_hip.h")).read()
    assert "int ss_bm25_search_sorted_facets(" in header
    assert "#define SS_ABI_VERSION 7\n" in header  # an additive entry: the version stays
    assert "pub fn ss_bm25_search_sorted_facets(" in open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()


class StubShard:
    """one shard in numpy: term t matches the docs whose value is a multiple of t + 2; scores fall with the doc id"""
    lexical_field_count = 1

    def __init__(self, shard_id, values):
        self.shard_id = shard_id
        self.values = np.asarray(values, np.int64)
        self.calls = []

    def make_queries(self, term_lists, query_types, not_lists=None, idf_of=None, field_filter=None):
        return [(tuple(term_lists[0]), int(query_types), tuple((not_lists or [[]])[0]))]

    def _matches(self, q, facet_filter):
        terms, qt, neg = q
        hit = [self.values % (t + 2) == 0 for t in terms]
        m = np.logical_and.reduce(hit) if qt == int(QueryType.Intersection) else np.logical_or.reduce(hit)
        for t in neg:
            m &= self.values % (t + 2) != 0
        if facet_filter:
            m &= (self.values >= facet_filter[0][2]) & (self.values < facet_filter[0][3])
        return np.nonzero(m)[0]

    def _order(self, docs, result_sort):
        score = 1.0 / (1.0 + docs)
        cols = [(-self.values[docs] if sf[2] else self.values[docs]) for sf in result_sort]
        return docs[np.lexsort([docs, -score] + cols[::-1])]

    def search_lexical_sorted_facets(self, queries, result_sort, k, query_facets, result_type=ResultType.TopkCount, facet_filter=None):
        self.calls.append((len(queries), tuple(result_sort), int(k), int(result_type), facet_filter))
        docs = self._matches(queries[0], facet_filter)
        page = self._order(docs, result_sort)[:k] if int(result_type) != int(ResultType.Count) else docs[:0]
        kk = max(int(k), 1)
        doc = np.full((1, kk), 0xFFFFFFFF, np.uint32)
        score = np.zeros((1, kk), np.float32)
        doc[0, :len(page)] = page
        score[0, :len(page)] = 1.0 / (1.0 + page)
        per = [np.array([[int((self.values[docs] < 0).sum()), int((self.values[docs] >= 0).sum()), 0]], np.uint64) for _ in query_facets]
        return doc, score, np.array([len(page)], np.uint32), np.array([len(docs)], np.uint64), per

    def search_lexical_sorted(self, query, result_sort, k, facet_filter=None):
        docs = self._matches(query[0], facet_filter)
        page = self._order(docs, result_sort)[:k]
        return page.astype(np.uint32), (1.0 / (1.0 + page)).astype(np.float32), len(docs)

    def facet_values(self, doc_ids, facet_offset, facet_type):
        return (self.values[np.asarray(doc_ids, np.int64)] & 0xFFFFFFFF).astype(np.uint64)  # stored bits of an i32 column


QF = [{"field": "v", "offset": 0, "type": "i32", "ranges": [("neg", -(1 << 31)), ("pos", 0)], "range_type": "within"}]


def _index(sizes=(60, 41, 53), seed=5):
    rng = np.random.default_rng(seed)
    shards = [StubShard(i, rng.integers(-30, 31, n)) for i, n in enumerate(sizes)]
    return Index(shards), shards


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("offset,length", [(0, 10), (4, 7), (0, 500)])
def test_sorted_hits_and_facets_in_one_shard_call(desc, offset, length):
    ix, shards = _index()
    S = len(shards)
    sort = [(0, "i32", desc)]
    for terms, qt, neg in (([0, 1], QueryType.Union, []), ([0, 1], QueryType.Intersection, []), ([1], QueryType.Union, [0])):
        ro = ix.search(terms, query_type_default=qt, offset=offset, length=length, result_sort=sort, query_facets=QF, not_terms=neg)
        hits = ix.search(terms, query_type_default=qt, offset=offset, length=length, result_sort=sort, not_terms=neg)
        assert [(r.doc_id, r.score) for r in ro.results] == [(r.doc_id, r.score) for r in hits.results] and ro.results
        assert ro.result_count == len(ro.results) == hits.result_count and ro.result_count_total == hits.result_count_total
        # the order, from numpy over the whole index: (key, score desc, global id)
        rows = []
        for sh in shards:
            d = sh._matches((tuple(terms), int(qt), tuple(neg)), None)
            rows += [((-1 if desc else 1) * int(sh.values[x]), -np.float32(1.0 / (1.0 + x)), int(x) * S + sh.shard_id) for x in d]
        rows.sort()
        assert [r.doc_id for r in ro.results] == [g for _, _, g in rows[offset:offset + length]]
        n_neg = sum(1 for key, _, _ in rows if (-key if desc else key) < 0)
        assert set(ro.facets) == {"v"} and dict(ro.facets["v"]) == {a: c for a, c in (("neg", n_neg), ("pos", len(rows) - n_neg)) if c}
        # every shard asked ONCE, for offset + length, through the combined call
        assert all(len(sh.calls) == 1 and sh.calls[0][:4] == (1, tuple(sort), offset + length, int(ResultType.TopkCount)) for sh in shards)
        for sh in shards:
            sh.calls.clear()


def test_result_types_and_the_filter_reach_the_shards():
    ix, shards = _index()
    sort = [(0, "i32", True)]
    flt = [(0, "i32", -10, 10)]
    ro = ix.search([0, 1], result_sort=sort, query_facets=QF, facet_filter=flt, length=5)
    assert all(sh.calls[-1][4] == flt for sh in shards) and all(-10 <= shards[r.doc_id % 3].values[r.doc_id // 3] < 10 for r in ro.results)
    topk = ix.search([0, 1], result_sort=sort, query_facets=QF, result_type=ResultType.Topk, length=5)
    assert topk.facets == {} and [r.doc_id for r in topk.results] == [r.doc_id for r in ix.search([0, 1], result_sort=sort, length=5).results]
    cnt = ix.search([0, 1], result_sort=sort, query_facets=QF, result_type=ResultType.Count, length=5)
    full = ix.search([0, 1], result_sort=sort, query_facets=QF, length=5)
    assert cnt.results == [] and cnt.facets == full.facets and cnt.result_count_total == full.result_count_total
    assert all(sh.calls[-2][3] == int(ResultType.Count) for sh in shards)


def test_what_keeps_raising():
    ix, _ = _index()
    sort = [(0, "i32", True)]
    for mode in (SearchMode.Hybrid, SearchMode.Vector):
        with pytest.raises(ValueError):
            ix.search([0, 1], np.zeros(4, np.float32), search_mode=mode, result_sort=sort, query_facets=QF)
        with pytest.raises(ValueError):
            ix.search([0, 1], np.zeros(4, np.float32), search_mode=mode, result_sort=sort)
    with pytest.raises(ValueError):
        ix.search([], result_sort=sort, query_facets=QF)
    with pytest.raises(ValueError):
        Index([]).search([1, 2], result_sort=sort, query_facets=QF)  # no shard: no facet schema to resolve the sort field against
    Index([]).search([1, 2], query_facets=QF)
