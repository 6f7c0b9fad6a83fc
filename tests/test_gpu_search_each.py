"""A batch whose queries each carry their OWN facet filters (ss_bm25_search_each; csrc/facet.hip facet_filter_rows_kernel and
match_exclude_rows_kernel; -m gpu).

Yardstick: the entry's contract -- query i gets exactly what ss_bm25_search_sorted_facets returns for that query alone under its
filters, bit for bit: docs and scores (as u32) of the rows' first `count` slots, counts, totals and counters.  Independently, the totals
and counters of the TopkCount rows == numpy histograms over (the oracle's match set and the numpy statement of the query's filter),
built as tests/test_gpu_query_facets.py builds them.  The image, the 71 queries (two chunks: 64 + 7) and the nine filter sets dealt
round-robin stand in tests/search_each_world.py."""
import numpy as np
import pytest

import search_each_world as EW
from test_gpu_query_facets import _want_counts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def W(S, O):
    W = EW.build(S, O)
    W.qs = EW.queries()
    W.q = EW.make(S, W, W.qs)
    W.sets = EW.filter_sets(O, W)
    W.flt = [W.sets[i % 9][1] for i in range(len(W.qs))]
    W.keep = [W.sets[i % 9][2] for i in range(len(W.qs))]
    W.sh.set_coalescing_faceted(0)  # (the yardstick is the single entries' direct path; tests/test_gpu_faceted_callers.py has the callers)
    yield W
    W.sh.close()


@pytest.fixture(scope="module")
def want(O, W):
    """per query: the oracle's match set under the tombstones and the numpy statement of its filter -> (total, counters per facet)"""
    out = []
    gone = np.zeros(W.n_docs, bool)
    gone[W.gone] = True
    dead = [np.nonzero(gone | ~keep)[0] for _, _, keep in W.sets]
    for i, (op, terms, neg) in enumerate(W.qs):
        W.osh.set_deleted(dead[i % 9])
        if op == EW.PHRASE:
            md, _, tot = W.osh.search_phrase(terms, list(range(len(terms))), W.n_docs)
        else:
            md, _, tot = W.osh.search_exhaustive(terms, O.OP_OR if op == EW.OR else O.OP_AND, W.n_docs, neg)
        assert len(md) == tot
        out.append((tot, [_want_counts(W, qf, md.astype(np.int64)) for qf in EW.facets()]))
    return out


SPECS = {"facets": ([], True), "sorts+facets": (EW.SORTS, True), "sorts": (EW.SORTS, False), "plain": ([], False)}


def _alone(S, W, i, sorts, k, qfs, rt):
    return W.sh.search_lexical_sorted_facets(W.q[i:i + 1], sorts, k, qfs, rt, W.flt[i] or None)


def _rows_equal(got, i, one, rt, S, what):
    doc, score, cnt, tot, per = got
    d1, s1, c1, t1, p1 = one
    assert int(cnt[i]) == int(c1[0]) and int(tot[i]) == int(t1[0]), (what, i, "count / total", int(cnt[i]), int(c1[0]), int(tot[i]), int(t1[0]))
    n = int(cnt[i])
    if rt != S.ResultType.Count:
        assert np.array_equal(doc[i][:n], d1[0][:n]), (what, i, "docs")
        assert np.array_equal(score[i][:n].view(np.uint32), s1[0][:n].view(np.uint32)), (what, i, "scores")
    assert len(per) == len(p1)
    for f in range(len(per)):
        assert np.array_equal(per[f][i], p1[f][0]), (what, i, "counters of facet", f)


@pytest.mark.parametrize("k", [10, 129])
@pytest.mark.parametrize("spec", list(SPECS))
def test_every_query_gets_its_own_answer(S, W, want, spec, k):
    """(no sort, three facets), (two sort fields, three facets), (sort, no facets), (no sort, no facets) x Topk, TopkCount, Count x
    k = 10, 129 over 71 queries under nine filter sets: every row == the existing entry called with that query alone; the TopkCount
    rows' totals and counters == the oracle's match sets under the numpy statement of the filters"""
    sorts, with_facets = SPECS[spec]
    qfs = EW.facets() if with_facets else []
    nq = len(W.qs)
    for rt in (S.ResultType.Topk, S.ResultType.TopkCount, S.ResultType.Count):
        what = (spec, k, int(rt))
        got = W.sh.search_lexical_each(W.q, k, rt, W.flt, sorts, qfs)
        for i in range(nq):
            _rows_equal(got, i, _alone(S, W, i, sorts, k, qfs, rt), rt, S, what)
        if rt == S.ResultType.TopkCount:
            for i in range(nq):
                otot, counts = want[i]
                assert int(got[3][i]) == otot, (what, i, "total against the oracle")
                assert int(got[2][i]) == min(k, otot), (what, i)
                for f in range(len(qfs)):
                    assert np.array_equal(got[4][f][i], counts[f]), (what, i, qfs[f]["field"])
    # the mix is what it says: some query matches nothing under its filter, some more than k, and a filter that passes everything
    # leaves its query's total where the empty set leaves it
    tots = [t for t, _ in want]
    assert min(tots) == 0 and max(tots) > 1024 and sum(1 for t in tots if t > 129) > 20


def test_a_filter_that_passes_nothing(S, W, want):
    """count 0, total 0, all-zero counters -- and the neighbours' rows are their own: the same batch with that set emptied changes no
    other row"""
    qfs = EW.facets()
    got = W.sh.search_lexical_each(W.q, 10, S.ResultType.TopkCount, W.flt, EW.SORTS, qfs)
    hit = [i for i in range(len(W.qs)) if i % 9 == 1]
    assert len(hit) == 8
    for i in hit:
        assert int(got[2][i]) == 0 and int(got[3][i]) == 0 and all(int(p[i].sum()) == 0 for p in got[4]), i
    flt2 = [[] if i % 9 == 1 else f for i, f in enumerate(W.flt)]
    got2 = W.sh.search_lexical_each(W.q, 10, S.ResultType.TopkCount, flt2, EW.SORTS, qfs)
    for i in range(len(W.qs)):
        if i % 9 == 1:
            continue
        n = int(got[2][i])
        assert int(got2[2][i]) == n and int(got2[3][i]) == int(got[3][i]) and np.array_equal(got2[0][i][:n], got[0][i][:n]), i
        assert all(np.array_equal(p2[i], p[i]) for p2, p in zip(got2[4], got[4])), i


def test_a_deep_page_takes_the_single_entries_route(S, W):
    """k = SS_MAX_K + 5 on three queries: every query through the existing entry, in passes -- equal answers"""
    from seekstorm_amd import _native as N
    k, qfs = N.SS_MAX_K + 5, EW.facets()
    pick = [0, 6, 13]  # (the 6-term OR under no filter, queries under the two-filter set and under the 8-id set)
    q = np.ascontiguousarray(W.q[pick])
    flt = [W.flt[i] for i in pick]
    for sorts in ([], EW.SORTS):
        got = W.sh.search_lexical_each(q, k, S.ResultType.TopkCount, flt, sorts, qfs)
        assert int(got[2].max()) > N.SS_MAX_K
        for j, i in enumerate(pick):
            _rows_equal(got, j, _alone(S, W, i, sorts, k, qfs, S.ResultType.TopkCount), S.ResultType.TopkCount, S, ("deep", bool(sorts)))


def test_one_refused_query_fails_the_call(S, O):
    """a phrase on the same image without positions: the facet entries refuse it (SS_ENOTSUP), and so does the whole batch"""
    from seekstorm_amd import _native as N
    W2 = EW.build(S, O, positions=False, oracle=False)
    try:
        W2.sh.set_coalescing_faceted(0)
        qs = [(EW.OR, [3], []), (EW.PHRASE, [0, 1], []), (EW.AND, [0, 2], [])]
        q = EW.make(S, W2, qs)
        flt = [[], [(EW.OFF["u32"], "u32", 0, 1 << 31)], []]
        with pytest.raises(S.SeekStormHipError) as e:
            W2.sh.search_lexical_sorted_facets(q[1:2], [], 10, EW.facets(), S.ResultType.TopkCount, flt[1])
        assert e.value.code == N.SS_ENOTSUP
        for sorts in ([], EW.SORTS):
            with pytest.raises(S.SeekStormHipError) as e:
                W2.sh.search_lexical_each(q, 10, S.ResultType.TopkCount, flt, sorts, EW.facets())
            assert e.value.code == N.SS_ENOTSUP, sorts
        # without the phrase the batch is answered
        keep = np.ascontiguousarray(q[[0, 2]])
        got = W2.sh.search_lexical_each(keep, 10, S.ResultType.TopkCount, [flt[0], flt[2]], EW.SORTS, EW.facets())
        assert int(got[3][0]) > 0
    finally:
        W2.sh.close()


def test_filter_begin_must_ascend(S, W):
    from seekstorm_amd import _native as N
    n, arr = W.sh._result_sorts(EW.SORTS)
    flat = W.flt[3] + W.flt[4]
    ok = W.sh.search_lexical_each_raw(np.ascontiguousarray(W.q[3:5]), 10, S.ResultType.TopkCount, [0, 1, 2], flat, n, arr, EW.facets())
    assert int(ok[3][0]) > 0
    for begin in ([0, 2, 1], [1, 0, 2], [0, 10, 11]):  # (the last: ascending, but more than SS_MAX_FACET_FILTERS in a set)
        with pytest.raises(S.SeekStormHipError) as e:
            W.sh.search_lexical_each_raw(np.ascontiguousarray(W.q[3:5]), 10, S.ResultType.TopkCount, begin, flat, n, arr, EW.facets())
        assert e.value.code == N.SS_EINVAL, begin


def test_count_with_a_sort_field_beyond_the_record_is_the_single_entrys_verdict(S, W):
    """SS_RT_COUNT reads no sort key: ss_bm25_search_sorted_facets checks the sort fields' types and rank tables and then counts, whatever
    their offsets -- and so does the batch; with docs wanted both refuse the field (SS_ESTATE)"""
    from seekstorm_amd import _native as N
    far = [(EW.REC.itemsize - 2, "u32", False)]  # 22 + 4 > 24

    def outcome(fn):
        try:
            r = fn()
            return ("ok", [int(x) for x in r[3]], [p.tolist() for p in r[4]])
        except S.SeekStormHipError as e:
            return ("error", e.code)

    q, flt = np.ascontiguousarray(W.q[2:5]), W.flt[2:5]
    for rt in (S.ResultType.Count, S.ResultType.TopkCount):
        each = outcome(lambda: W.sh.search_lexical_each(q, 10, rt, flt, far, EW.facets()))
        alone = [outcome(lambda: W.sh.search_lexical_sorted_facets(q[i:i + 1], far, 10, EW.facets(), rt, flt[i] or None)) for i in range(3)]
        if rt == S.ResultType.Count:
            assert each[0] == "ok" and all(a[0] == "ok" for a in alone)
            assert each[1] == [a[1][0] for a in alone]
            assert all(each[2][f][i] == alone[i][2][f][0] for f in range(3) for i in range(3))
        else:
            assert each == ("error", N.SS_ESTATE) and all(a == ("error", N.SS_ESTATE) for a in alone)
