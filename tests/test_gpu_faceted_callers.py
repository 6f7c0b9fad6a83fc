"""Concurrent faceted, filtered and sorted callers share device batches (the faceted kind of the coalescer, csrc/api_coalesce.hip:
ss_shard_set_coalescing_faceted; -m gpu): one query per call from many threads, every caller with its own facet filter, and every
answer is the one the same call returns alone with the kind off.  The image is tests/search_each_world.py's."""
import threading

import numpy as np
import pytest

import search_each_world as EW

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
    W = EW.build(S, O, oracle=False)
    W.dist = O.geo_distances(W.v["loc"], EW.BASE, EW.UNIT)
    W.qs = EW.queries()
    W.q = EW.make(S, W, W.qs)
    W.sets = [f for _, f, _ in EW.filter_sets(O, W)][:8]  # (without the extern id set: such a call is not the coalescer's)
    yield W
    W.sh.close()


FACETS2 = EW.facets()[:2]  # the other spec


def _call(S, W, kind, i, j):
    """caller j's one-query call: query i under filter set j"""
    q, flt = W.q[i:i + 1], W.sets[j % len(W.sets)] or None
    if kind == "filtered":  # (without a filter the call is the lexical kind's)
        flt = W.sets[1 + j % (len(W.sets) - 1)]
    if kind == "sorted_facets":
        return W.sh.search_lexical_sorted_facets(q, EW.SORTS, 10, EW.facets(), S.ResultType.TopkCount, flt)
    if kind == "facets":
        return W.sh.search_lexical_facets(q, 10, FACETS2, S.ResultType.TopkCount, flt, reference_shortcuts=False)
    if kind == "sorted":
        return W.sh.search_lexical_sorted_batch(q, EW.SORTS, 10, flt) + ([],)
    return W.sh.search_lexical_batch(q, 10, S.ResultType.TopkCount, False, flt) + ([],)


def _same(a, b):
    n = int(a[2][0])
    return (n == int(b[2][0]) and int(a[3][0]) == int(b[3][0]) and np.array_equal(a[0][0][:n], b[0][0][:n]) and
            np.array_equal(a[1][0][:n].view(np.uint32), b[1][0][:n].view(np.uint32)) and len(a[4]) == len(b[4]) and
            all(np.array_equal(x, y) for x, y in zip(a[4], b[4])))


def _threads(n, fn):
    th = [threading.Thread(target=fn, args=(j,)) for j in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join()


def test_callers_that_arrive_together_share_batches(S, W):
    sh = W.sh
    # 16 callers: 12 sorted pages with one spec and 6 different filters, 4 unsorted ones with another spec
    plan = [("sorted_facets", 4 + j, j % 6) if j < 12 else ("facets", 20 + j, j) for j in range(16)]
    sh.set_coalescing_faceted(0)
    want = [_call(S, W, kind, i, f) for kind, i, f in plan]
    assert sum(int(w[3][0]) > 10 for w in want) >= 8  # (most callers have a full page to compare)
    stats0, lex0 = sh.coalescing_stats_faceted(), sh.coalescing_stats()
    sh.set_coalescing_faceted(64, 50000)
    bar, got, errors = threading.Barrier(16), {}, []

    def burst(j):
        try:
            kind, i, f = plan[j]
            bar.wait()
            got[j] = _call(S, W, kind, i, f)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    _threads(16, burst)
    assert not errors, errors[:3]
    b1, q1 = sh.coalescing_stats_faceted()
    assert q1 - stats0[1] == 16 and 1 <= b1 - stats0[0] <= 4, (b1 - stats0[0], q1 - stats0[1])
    assert sh.coalescing_stats() == lex0  # the lexical and vector kinds did not move
    for j in range(16):
        assert _same(got[j], want[j]), (j, plan[j])

    # an invalid request inside a merged batch fails ALONE: its batch-mates get their answers
    bar, outcome = threading.Barrier(6), {}

    def mixed(j):
        q = W.q[4 + j:5 + j].copy()
        if j == 2:
            q["term"][0][0] = 0xFFFFFF  # no such term
        bar.wait()
        try:
            outcome[j] = sh.search_lexical_sorted_facets(q, EW.SORTS, 10, EW.facets(), S.ResultType.TopkCount, W.sets[j % 6] or None)
        except Exception as e:  # noqa: BLE001
            outcome[j] = e

    _threads(6, mixed)
    assert isinstance(outcome[2], S.SeekStormHipError)
    for j in (0, 1, 3, 4, 5):
        assert not isinstance(outcome[j], Exception), outcome[j]
        assert _same(outcome[j], want[j]), j

    # with the kind off nothing goes through it, and the answers are the same
    sh.set_coalescing_faceted(0)
    stats2 = sh.coalescing_stats_faceted()
    bar, got = threading.Barrier(16), {}
    _threads(16, burst)
    assert not errors, errors[:3]
    assert sh.coalescing_stats_faceted() == stats2
    for j in range(16):
        assert _same(got[j], want[j]), (j, plan[j])


def test_churn_of_mixed_kinds(S, W):
    """8 threads x 25 un-barriered rounds of all four kinds with max_wait_us = 0: no error, every answer its own -- leaders hand over,
    followers sleep and wake, requests of other specs stay queued for the next batch"""
    sh = W.sh
    kinds = ["sorted_facets", "facets", "sorted", "filtered"]
    calls = [(kinds[(t + r) % 4], (3 * t + 5 * r) % len(W.qs), t + r) for t in range(8) for r in range(25)]
    sh.set_coalescing_faceted(0)
    want = {}
    for c in calls:
        if c not in want:
            want[c] = _call(S, W, *c)
    sh.set_coalescing_faceted(64, 0)
    q0 = sh.coalescing_stats_faceted()[1]
    errors = []

    def loop(t):
        try:
            for r in range(25):
                c = calls[t * 25 + r]
                if not _same(_call(S, W, *c), want[c]):
                    errors.append(("differs", c))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    _threads(8, loop)
    assert not errors, errors[:3]
    b, q = sh.coalescing_stats_faceted()
    assert q - q0 == 200 and b >= 1
    sh.set_coalescing_faceted(0)
    # the queue is empty and the kind still serves: a lone caller goes straight through
    sh.set_coalescing_faceted(64, 0)
    assert _same(_call(S, W, *calls[0]), want[calls[0]])
    assert sh.coalescing_stats_faceted()[1] - q == 1
