"""The launch shape of the staged pruned kernel (csrc/bm25_probe.hip: PB_STAGED_WAVES waves per workgroup, one wave per (query, partition),
wave a = blockIdx.x * PB_STAGED_WAVES + w serving query a % nq, partition a / nq; the register budget chosen per instantiation by
pb_staged_min_waves).  Whatever the workgroup size and the number of resident waves, BM25_PRUNED must equal BM25_EXHAUSTIVE bit for bit
(docs, scores, counts, totals):

  * grid tails: nq x P leaves 0, 1 and 7 modulo 8 -- hence 0, 1 (or 0) and W - 1 modulo every workgroup size W of 1, 2, 4, 8 waves --
    through host batches beyond the one-launch limit and through tiny device-resident batches whose only workgroup is partial; the first
    valid wave (query 0, partition 0) and the last (query nq - 1, partition P - 1) each own docs of the expected answer;
  * both register budgets: unions of 2, 3, 4 lists and intersections, with and without tombstones, k = 10 (one key per lane) and
    k = 100 (two), Topk and TopkCount;
  * neighbouring waves of very different length: the 1-posting and the 2048-per-sub-block driver lists in alternation;
  * more than two rounds of 8192 resident waves: 1100 queries x 16 partitions, late waves running on thresholds and histograms that
    finished ones wrote.

The corpus is the 16 x 4096-doc hand corpus of test_gpu_probe_stream_edges."""
import numpy as np
import pytest

from test_gpu_probe_bound import _equal, _ops
from test_gpu_probe_stream_edges import (E_LENS, N_SUB, SUB, T_A, T_B, T_C, T_D, T_H1, T_H2, _batches, partitions, world)  # noqa: F401 (fixtures)
from test_gpu_pruned import _run
from test_gpu_small_batch import _dev_search

pytestmark = pytest.mark.gpu

ONE_LAUNCH_LIMIT = 256  # host batches up to this size may take the one-launch kernel


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _staged(S, sh, lists, qt, k, rt, what):
    """PRUNED == EXHAUSTIVE for a host batch that must take the staged pipeline; returns the (identical) answer"""
    from seekstorm_amd import _native as N
    assert len(lists) > ONE_LAUNCH_LIMIT
    q = sh.make_queries(lists, qt)
    before = sh.one_launch_batches()
    p = _run(S, sh, q, k, rt, N.BM25_PRUNED)
    assert sh.one_launch_batches() == before, "the batch did not take the staged pipeline"
    e = _run(S, sh, q, k, rt, N.BM25_EXHAUSTIVE)
    _equal(p, e, rt, S, what)
    return p


def _fill(base, nq, first=None, last=None):
    out = [base[i % len(base)] for i in range(nq)]
    if first is not None:
        out[0] = first
    if last is not None:
        out[-1] = last
    return out


def _part_range(p, P):
    """doc ids of partition p of P (the kernels' rule: sub-blocks n_sub p / P .. n_sub (p + 1) / P)"""
    return (N_SUB * p) // P * SUB, (N_SUB * (p + 1)) // P * SUB


TAIL_NQ, TAIL_P = (257, 300, 301, 307), (1, 3, 16)


def test_tail_cases_cover_the_remainders():
    """the grid below leaves 0, 1 and 7 waves modulo 8: for every workgroup size W that divides 8, 0, 1 % W and W - 1"""
    rem = {(nq * P) % 8 for nq in TAIL_NQ for P in TAIL_P} | {(nq * 3) % 8 for nq in (1, 3, 5)}
    assert {0, 1, 7} <= rem
    for W in (1, 2, 4, 8):
        assert {0, 1 % W, W - 1} <= {r % W for r in rem}


@pytest.mark.parametrize("partitions", TAIL_P, indirect=True)
def test_grid_tails(S, O, world, partitions):
    from seekstorm_amd import _native as N
    sh, osh, lists = world
    P = partitions
    base = dict((n, tl) for n, _, tl in _batches())["or3"]
    k = 10
    # queries whose top-k needs docs of the FIRST / the LAST partition: found among the base queries on the exhaustive answer
    exh = _run(S, sh, sh.make_queries(base, S.QueryType.Union), k, S.ResultType.Topk, N.BM25_EXHAUSTIVE)
    lo0, hi0 = _part_range(0, P)
    lo1, hi1 = _part_range(P - 1, P)
    in_first = [i for i in range(len(base)) if np.any((exh[0][i][:int(exh[2][i])] >= lo0) & (exh[0][i][:int(exh[2][i])] < hi0))]
    in_last = [i for i in range(len(base)) if np.any((exh[0][i][:int(exh[2][i])] >= lo1) & (exh[0][i][:int(exh[2][i])] < hi1))]
    assert in_first and in_last, (P, in_first, in_last)
    for nq in TAIL_NQ:
        tl = _fill(base, nq, first=base[in_first[0]], last=base[in_last[-1]])
        for rt in (S.ResultType.Topk, S.ResultType.TopkCount):
            got = _staged(S, sh, tl, S.QueryType.Union, k, rt, ("tails", nq, P, rt))
            # the first wave's and the last wave's lists arrived: their docs stand in the answers of query 0 and query nq - 1
            d0, d1 = got[0][0][:int(got[2][0])], got[0][-1][:int(got[2][-1])]
            assert np.any((d0 >= lo0) & (d0 < hi0)) and np.any((d1 >= lo1) & (d1 < hi1)), ("tails", nq, P)
            assert np.array_equal(got[0][0], exh[0][in_first[0]]) and np.array_equal(got[0][-1], exh[0][in_last[-1]])
        # intersections count in the probe kernel itself (one atomic per wave): a wave that left early or ran twice shows in the totals
        tl = _fill(dict((n, t) for n, _, t in _batches())["and2"], nq)
        _staged(S, sh, tl, S.QueryType.Intersection, k, S.ResultType.TopkCount, ("tails, and2", nq, P))


@pytest.mark.parametrize("partitions", [3], indirect=True)
def test_partial_only_workgroup_through_the_device_entry(S, O, world, partitions):
    """1, 3 and 5 device-resident queries x 3 partitions = 3, 9 and 15 waves: the last (or only) workgroup is partial in every shape"""
    from seekstorm_amd import _native as N
    sh, osh, lists = world
    for name, is_and, base in _batches():
        nt = len(base[0])
        qt = S.QueryType.Intersection if is_and else S.QueryType.Union
        for nq in (1, 3, 5):
            q = sh.make_queries(base[-nq:], qt)
            out = {}
            for strategy in (N.BM25_PRUNED, N.BM25_EXHAUSTIVE):
                sh.set_strategy(strategy)
                try:
                    out[strategy] = _dev_search(S, sh, q, 10, S.ResultType.TopkCount, _ops(is_and, nt))
                finally:
                    sh.set_strategy(N.BM25_AUTO)
            _equal(out[N.BM25_PRUNED], out[N.BM25_EXHAUSTIVE], S.ResultType.TopkCount, S, ("device entry", name, nq))


@pytest.mark.parametrize("partitions", [3, N_SUB], indirect=True)
@pytest.mark.parametrize("tombstones", [False, True])
def test_both_register_budgets(S, O, world, partitions, tombstones):
    """every (lists, filter, keys per lane) family of the staged kernel: k = 10 compiles under pb_staged_min_waves' new budget, k = 100
    under the old one"""
    sh, osh, lists = world
    rng = np.random.default_rng(5)
    drivers = list(range(len(E_LENS))) + [T_D]
    gone = np.unique(np.concatenate([rng.integers(0, N_SUB * SUB, N_SUB * SUB // 40)] + [lists[t][0][::4] for t in drivers]))
    try:
        if tombstones:
            sh.set_deleted(gone.astype(np.uint64)); osh.set_deleted([int(x) for x in gone])
        for name, is_and, base in _batches():
            qt = S.QueryType.Intersection if is_and else S.QueryType.Union
            tl = _fill(base, 259)
            for k in (10, 100):
                for rt in (S.ResultType.Topk, S.ResultType.TopkCount):
                    _staged(S, sh, tl, qt, k, rt, ("budgets", name, k, rt, partitions, tombstones))
    finally:
        sh.set_deleted([]); osh.set_deleted([])


@pytest.mark.parametrize("partitions", [N_SUB], indirect=True)
def test_neighbours_of_very_different_length(S, O, world, partitions):
    """E_1 (one posting) and D (up to 2048 postings a sub-block) in alternation: at one partition per sub-block the waves beside a long
    one end at once"""
    sh, osh, lists = world
    assert len(lists[0][0]) == 1 and max(np.bincount(lists[T_D][0] // SUB)) == 2048
    for name, qt, pair in (("or3", S.QueryType.Union, [[0, T_A, T_B], [T_D, T_A, T_B]]), ("or2", S.QueryType.Union, [[0, T_B], [T_D, T_B]]),
                           ("or4", S.QueryType.Union, [[0, T_A, T_B, T_C], [T_D, T_A, T_B, T_C]]),
                           ("and3", S.QueryType.Intersection, [[0, T_A, T_C], [T_D, T_A, T_C]])):
        tl = _fill(pair, 301)
        for k in (10, 100):
            for rt in (S.ResultType.Topk, S.ResultType.TopkCount):
                _staged(S, sh, tl, qt, k, rt, ("neighbours", name, k, rt))


@pytest.mark.parametrize("partitions", [N_SUB], indirect=True)
def test_more_than_two_rounds_of_resident_waves(S, O, world, partitions):
    """1100 queries x 16 partitions = 17 600 waves, more than twice the 8192 a chip of 256 CUs holds at 8 per SIMD"""
    sh, osh, lists = world
    assert 1100 * partitions > 2 * 8192
    base = dict((n, tl) for n, _, tl in _batches())
    base["or3"] = base["or3"] + [[T_H1, T_H2, T_A], [T_A, T_H2, T_H1]]
    for name, qt in (("or3", S.QueryType.Union), ("and3", S.QueryType.Intersection)):
        tl = _fill(base[name], 1100)
        got = _staged(S, sh, tl, qt, 10, S.ResultType.TopkCount, ("rounds", name))
        n = len(base[name])
        for r in range(0, 1100 - n, n):  # every repetition answers like the first
            assert all(np.array_equal(x[r:r + n], x[:n]) for x in got), ("rounds", name, r)
    _staged(S, sh, _fill(base["or3"], 1100), S.QueryType.Union, 100, S.ResultType.Topk, ("rounds", "or3", 100))
