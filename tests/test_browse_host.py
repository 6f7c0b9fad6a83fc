"""The empty query on the host, no device: Index.search(enable_empty_query=...) of the Python mirror over stub shards -- which path it
takes, how it spells `_id`, how it merges the shards' rows -- and the flag's default, under which nothing changes."""
import numpy as np
import pytest

from seekstorm_amd.search import Index, ResultType, SearchMode, Shard

from test_query_facets_host import _range_facet


class StubShard:
    """search_iterator_shard in numpy: docs = the live ones, ordered by (value asc / desc, doc id in the tie direction)"""
    lexical_field_count = 1

    def __init__(self, shard_id, values, gone):
        self.shard_id = shard_id
        self.values = np.asarray(values, np.int64)
        self.indexed_doc_count = len(self.values)
        self.alive = np.ones(len(self.values), bool)
        self.alive[list(gone)] = False
        self.calls = []

    def search_docs_raw(self, k, result_type=ResultType.TopkCount, facet_filter=None, result_sort=None, query_facets=None, doc_ascending=False,
                        skip=0):
        sorts, asc = Shard.split_id_sort(result_sort, doc_ascending)
        self.calls.append((int(k), int(result_type), facet_filter, tuple(sorts), asc))
        keep = self.alive if not facet_filter else self.alive & (self.values >= facet_filter[0][2]) & (self.values < facet_filter[0][3])
        docs = np.nonzero(keep)[0]
        cols = [(-self.values[docs] if sf[2] else self.values[docs]) for sf in sorts]
        docs = docs[np.lexsort([docs if asc else -docs] + cols[::-1])]
        per = [np.array([len(docs), 0], np.uint64)] if query_facets else []
        page = docs[skip:skip + k] if int(result_type) != int(ResultType.Count) else docs[:0]
        return page.astype(np.uint32), len(page), len(docs), per

    def search_docs(self, k, result_type=ResultType.TopkCount, facet_filter=None, result_sort=None, query_facets=None, doc_ascending=False, skip=0):
        d, c, t, _ = self.search_docs_raw(k, result_type, facet_filter, result_sort, query_facets, doc_ascending, skip)
        return d, c, t, {}

    def facet_values(self, doc_ids, facet_offset, facet_type):
        return (self.values[np.asarray(doc_ids, np.int64)] & 0xFFFFFFFF).astype(np.uint64)  # stored bits of an i32 column


def _index(seed=3, sizes=(40, 23, 31)):
    rng = np.random.default_rng(seed)
    shards = [StubShard(i, rng.integers(-3, 4, n), rng.choice(n, n // 4, replace=False)) for i, n in enumerate(sizes)]
    S = len(shards)
    gid = np.concatenate([np.nonzero(sh.alive)[0] * S + sh.shard_id for sh in shards])
    val = np.concatenate([sh.values[sh.alive] for sh in shards])
    return Index(shards), shards, gid, val


def test_the_flag_is_off_by_default_and_nothing_changes():
    qf = [_range_facet("within")]
    ix, shards, _, _ = _index()
    with pytest.raises(ValueError):
        Index([]).search([], query_facets=qf)
    with pytest.raises(ValueError):
        ix.search([], query_facets=qf)
    with pytest.raises(ValueError):
        ix.search([], result_sort=[(0, "i32", False)])
    with pytest.raises(ValueError):
        ix.search([], query_facets=qf, enable_empty_query=False)
    ro = ix.search([])  # no terms, no flag: an empty answer, no shard is asked
    assert ro.results == [] and ro.result_count_total == 0 and all(sh.calls == [] for sh in shards)
    # Vector and Hybrid searches without terms are not the flag's business
    ro = ix.search([], search_mode=SearchMode.Hybrid, enable_empty_query=True)
    assert ro.results == [] and all(sh.calls == [] for sh in shards)


@pytest.mark.parametrize("sorts,ascending", [(None, False), ([("_id", True)], False), ([("_id", False)], True), ([("_score", True)], False),
                                             ([("_score", False)], True)])
def test_index_path_by_global_id(sorts, ascending):
    ix, shards, gid, _ = _index()
    n_all = sum(sh.indexed_doc_count for sh in shards)
    order = np.sort(gid) if ascending else np.sort(gid)[::-1]
    for offset, length in ((0, 10), (4, 7), (len(gid) - 3, 10), (len(gid), 4)):
        ro = ix.search([], enable_empty_query=True, offset=offset, length=length, result_sort=sorts)
        assert [r.doc_id for r in ro.results] == order[offset:offset + length].tolist()
        assert all(r.score == 0.0 for r in ro.results) and ro.result_count == len(ro.results)
        assert ro.result_count_total == n_all > len(gid)  # tombstoned docs included: the crate's figure
    assert all(c[0] == len(gid) + 4 and c[1] == int(ResultType.Topk) and c[2] is None and c[3] == () and c[4] == ascending
               for sh in shards for c in sh.calls[-1:])  # every shard asked for offset + length by id alone
    ro = ix.search([], enable_empty_query=True, result_type=ResultType.Count, result_sort=sorts)
    assert ro.results == [] and ro.result_count_total == n_all


@pytest.mark.parametrize("sorts,ascending", [([(0, "i32", False)], False), ([(0, "i32", True)], False), ([(0, "i32", False), ("_id", False)], True),
                                             ([(0, "i32", True), ("_id", True)], False), ([(0, "i32", True), ("_score", False)], False)])
def test_shard_path_merges_by_keys_then_global_id(sorts, ascending):
    ix, shards, gid, val = _index()
    col = -val if sorts[0][2] else val
    order = gid[np.lexsort([gid if ascending else -gid, col])]
    for offset, length in ((0, 10), (5, 20), (len(gid) - 2, 10)):
        ro = ix.search([], enable_empty_query=True, offset=offset, length=length, result_sort=sorts, field_filter=[1])
        assert [r.doc_id for r in ro.results] == order[offset:offset + length].tolist(), (sorts, offset)
        assert ro.result_count_total == len(gid) and all(r.score == 0.0 for r in ro.results)  # live matches only on this path
    assert all(sh.calls[-1][3] == (sorts[0],) and sh.calls[-1][4] == ascending for sh in shards)  # the marker never reaches a shard as a field


def test_a_filter_or_facets_take_the_shard_path():
    ix, shards, gid, val = _index()
    flt = [(0, "i32", -1, 2)]
    keep = (val >= -1) & (val < 2)
    for sorts, ascending in ((None, False), ([("_id", False)], True)):
        ro = ix.search([], enable_empty_query=True, length=15, facet_filter=flt, result_sort=sorts)
        want = np.sort(gid[keep]) if ascending else np.sort(gid[keep])[::-1]
        assert [r.doc_id for r in ro.results] == want[:15].tolist() and ro.result_count_total == int(keep.sum())
    qf = [{"field": "v", "offset": 0, "type": "i32", "ranges": [("all", -(1 << 31))], "range_type": "within"}]
    ro = ix.search([], enable_empty_query=True, length=5, query_facets=qf)
    assert ro.result_count_total == len(gid) and ro.facets == {"v": [("all", len(gid))]}  # summed over the shards
    assert ix.search([], enable_empty_query=True, length=5, query_facets=qf, result_type=ResultType.Topk).facets == {}
    ro = ix.search([], enable_empty_query=True, length=5, query_facets=qf, result_type=ResultType.Count)
    assert ro.results == [] and ro.result_count_total == len(gid) and ro.facets == {"v": [("all", len(gid))]}


def test_id_marker_only_as_the_last_entry():
    assert Shard.split_id_sort(None) == ([], False)
    assert Shard.split_id_sort([(4, "u32", True)], True) == ([(4, "u32", True)], True)
    assert Shard.split_id_sort([(4, "u32", True), ("_id", False)]) == ([(4, "u32", True)], True)
    assert Shard.split_id_sort([(4, "u32", True), ("_id", True)], True) == ([(4, "u32", True)], False)
    assert Shard.split_id_sort([("_score", False)], True) == ([], True)
    for bad in ([("_id", True), (4, "u32", True)], [("_id", True), ("_id", True)], [("price", True)]):
        with pytest.raises(ValueError):
            Shard.split_id_sort(bad)
    ix, _, _, _ = _index()
    with pytest.raises(ValueError):
        ix.search([], enable_empty_query=True, result_sort=[("_id", True), (0, "i32", False)])


def test_the_symbol_is_declared_everywhere():
    import os
    import seekstorm_amd
    from seekstorm_amd import _native as N
    root = os.path.dirname(os.path.dirname(seekstorm_amd.__file__))
    assert "ss_docs_search" in [name for name, _, _ in N.SYMBOLS]
    assert "int ss_docs_search(" in open(os.path.join(root, "include", "seekstorm_hip.h")).read()
    assert "pub fn ss_docs_search(" in open(os.path.join(root, "integration", "hip_ffi.rs")).read()
