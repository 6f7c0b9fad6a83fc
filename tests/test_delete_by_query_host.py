"""delete_documents_by_query on the host, no device: which route Index.delete_documents_by_query of the Python mirror takes over stub
shards -- no shard for no terms, one call for one shard, a dry run and a real call per shard for the whole match set, the merged search
plus per-shard add_deleted for a bounded page or a shard that answers SS_ENOTSUP -- and the entry point's declarations."""
import os

import numpy as np

from seekstorm_amd import _native as N
from seekstorm_amd.search import Index, QueryType, Result, ResultObject, ResultSource


class StubShard:
    """a shard whose one query matches `match` (local ids) with a score per doc; doc g of the index is local g // S here"""
    lexical_field_count = 1
    compose_filtered_unions = False

    def __init__(self, shard_id, n_shards, match, gone=(), notsup=False):
        self.shard_id, self.S = shard_id, n_shards
        self.match, self.gone, self.notsup = sorted(match), set(gone), notsup
        self.calls = []

    def score(self, d):  # distinct over the whole index: the merge has no ties to break
        return 1.0 + ((d * self.S + self.shard_id) * 7919 % 1009) / 1009.0 + (d * self.S + self.shard_id) * 1e-6

    def ranked(self):
        return sorted((d for d in self.match if d not in self.gone), key=lambda d: (-self.score(d), d))

    def make_queries(self, term_lists, query_types, not_lists=None, idf_of=None, field_filter=None):
        return np.zeros(len(term_lists), N.BM25_QUERY_DTYPE)

    def mark_all_terms_frequent(self, queries, k):
        return queries

    def delete_by_query(self, queries, offset=0, length=None, facet_filter=None, result_sort=None, dry_run=False, return_docs=False):
        self.calls.append(("delete_by_query", int(offset), length, bool(dry_run), bool(return_docs)))
        if self.notsup:
            raise N.SeekStormHipError(N.SS_ENOTSUP, "stub")
        live = self.ranked()
        page = sorted(live[offset:] if length is None else live[offset:offset + length])
        if not dry_run:
            self.gone |= set(page)
        out = (np.array([len(live)], np.uint64), np.array([len(page)], np.uint64), len(page))
        return out + (np.array(page, np.uint32),) if return_docs else out

    def search_lexical_shard(self, query_terms, query_type_default=QueryType.Union, offset=0, length=10, result_type=None, strict=False,
                             not_terms=(), field_filter=None, facet_filter=None, query_facets=None, shard_number=1):
        self.calls.append(("search", int(offset), int(length)))
        live = self.ranked()
        ro = ResultObject()
        ro.results = [Result(d, self.score(d), ResultSource.Lexical) for d in live[:offset + length]][offset:]
        ro.result_count = len(ro.results)
        ro.result_count_total = len(live)
        return ro

    def add_deleted(self, doc_ids):
        self.calls.append(("add_deleted", sorted(int(d) for d in doc_ids)))
        self.gone |= set(int(d) for d in doc_ids)


def _index(n_shards, notsup_shard=None, seed=4):
    rng = np.random.default_rng(seed)
    shards = []
    for i in range(n_shards):
        match = rng.choice(60, 25, replace=False).tolist()
        shards.append(StubShard(i, n_shards, match, gone=match[:4], notsup=(i == notsup_shard)))
    return Index(shards), shards


def _live_global(shards):
    S = len(shards)
    rows = [(-sh.score(d), d * S + sh.shard_id) for sh in shards for d in sh.ranked()]
    return [g for _, g in sorted(rows)]


def test_no_terms_ask_no_shard():
    ix, shards = _index(3)
    assert ix.delete_documents_by_query([]) == [] and ix.delete_documents_by_query(None, length=5) == []
    assert all(sh.calls == [] for sh in shards)


def test_one_shard_is_one_call():
    for offset, length in ((0, None), (3, 6)):
        ix, (sh,) = _index(1)
        ranked = sh.ranked()
        want = sorted(ranked[offset:] if length is None else ranked[offset:offset + length])
        assert ix.delete_documents_by_query([7, 9], offset=offset, length=length) == want
        assert sh.calls == [("delete_by_query", offset, length, False, True)]
        assert not set(want) & set(sh.ranked())


def test_three_shards_whole_set_on_every_shard():
    for length in (None, 10_000):
        ix, shards = _index(3)
        want = sorted(_live_global(shards))
        assert len(want) == 63
        assert ix.delete_documents_by_query([1, 2], QueryType.Intersection, length=length) == want  # local * S + shard, ascending
        for sh in shards:
            assert sh.calls == [("delete_by_query", 0, None, True, False), ("delete_by_query", 0, None, False, True)]
            assert sh.ranked() == []
    # a dry run of the whole: the same ids, nothing deleted
    ix, shards = _index(3)
    want = sorted(_live_global(shards))
    assert ix.delete_documents_by_query([1, 2], dry_run=True) == want and sorted(_live_global(shards)) == want
    assert all(c[3] for sh in shards for c in sh.calls)


def test_three_shards_bounded_page_is_the_merged_search():
    ix, shards = _index(3)
    order = _live_global(shards)
    offset, length = 4, 17
    want = sorted(order[offset:offset + length])
    assert ix.delete_documents_by_query([1, 2], offset=offset, length=length) == want
    for sh in shards:
        local = sorted(g // 3 for g in want if g % 3 == sh.shard_id)
        assert [c for c in sh.calls if c[0] == "search"] == [("search", 0, offset + length)]  # ONE Index.search: every shard asked once
        assert [c for c in sh.calls if c[0] == "add_deleted"] == ([("add_deleted", local)] if local else [])
        assert [c for c in sh.calls if c[0] == "delete_by_query"] == [("delete_by_query", 0, None, True, False)]  # the dry run alone
    assert sorted(_live_global(shards)) == sorted(set(order) - set(want))
    # a page that ends beyond the matches, and one that begins there
    ix, shards = _index(3)
    order = _live_global(shards)
    assert ix.delete_documents_by_query([1, 2], offset=60, length=50) == sorted(order[60:])
    assert ix.delete_documents_by_query([1, 2], offset=60, length=50) == []


def test_a_shard_that_answers_enotsup_takes_the_search_route():
    for length in (None, 12):
        ix, shards = _index(3, notsup_shard=1)
        order = _live_global(shards)
        want = sorted(order if length is None else order[:length])
        assert ix.delete_documents_by_query([1, 2], length=length) == want
        assert not any(c[0] == "delete_by_query" and not c[3] for sh in shards for c in sh.calls)  # no real device delete anywhere
        for sh in shards:
            local = sorted(g // 3 for g in want if g % 3 == sh.shard_id)
            assert [c for c in sh.calls if c[0] == "add_deleted"] == [("add_deleted", local)]
    # one shard, the same answer
    ix, (sh,) = _index(1, notsup_shard=0)
    want = sorted(sh.ranked()[2:9])
    assert ix.delete_documents_by_query([5], offset=2, length=7) == want
    assert [c[0] for c in sh.calls] == ["delete_by_query", "search", "add_deleted"]


def test_the_entry_point_is_declared_everywhere():
    import seekstorm_amd
    root = os.path.dirname(os.path.dirname(seekstorm_amd.__file__))
    assert "ss_bm25_delete_by_query" in [name for name, _, _ in N.SYMBOLS]
    assert "int ss_bm25_delete_by_query(" in open(os.path.join(root, "include", "seekstorm_hip.h")).read()
    assert "pub fn ss_bm25_delete_by_query(" in open(os.path.join(root, "integration", "hip_ffi.rs")).read()
    q = np.zeros(1, N.BM25_QUERY_DTYPE)
    deleted = np.full(1, 7, np.uint64)
    assert N.lib().ss_bm25_delete_by_query(None, 1, q.ctypes.data, 0, None, 0, 10, 0, None, 0, None, None, N.ptr(deleted, N.u64p), None, 0) == N.SS_EINVAL
    assert int(deleted[0]) == 0
