"""The driver stream of the pruned strategy at its edges (csrc/bm25_probe_body.h, the `stream` lambda of pb_wave): a wave reads its driver
list 256 postings a group (512 in the one-launch kernel), keeps the NEXT group's postings in flight while the current one is evaluated, and
relies on the buffer descriptor to turn every read past the partition's end into a null posting.  BM25_PRUNED must equal BM25_EXHAUSTIVE
bit for bit (docs, scores, counts, totals) where that can go wrong:

  * driver streams of 0, 1, 63, 64, 255, 256, 257, 511, 512, 513 and 768 postings inside a partition (and 1023 .. 1536 for the one-launch
    kernel's groups of 512), reached through hand-built lists and SS_BM25_P = 1, 2 and n_sub -- the test counts the postings per
    partition on the host and asserts that every class occurs;
  * a driver list that is the LAST list of the posting array and ends in the middle of a group: the prefetch window reaches past the array;
  * partitions that end in the middle of a group with the next partition's postings directly behind;
  * unions of 2, 3 and 4 lists, intersections, tombstones (the filtered instances), k = 10 and k = 100, Topk and TopkCount;
  * later streams that are non-essential before they begin, and a second stream that must run;
  * the staged kernel (the batch repeated to 300 queries) and the one-launch kernel (the batch as it is)."""
import os

import numpy as np
import pytest

from test_gpu_probe_bound import _both_paths, _hand_corpus, _oracle, _shards

pytestmark = pytest.mark.gpu

N_SUB, SUB = 16, 4096
# postings of the driver list D in sub-block s (its LAST sub-block ends in the middle of a group; D is the last list of the array)
D_COUNTS = [0, 1, 63, 64, 255, 256, 257, 511, 512, 768, 1023, 1024, 1025, 1536, 2048, 513]
# one list E_L per length, all of it inside sub-block 3: the whole stream of partition 0 at P = 1 and P = 2
E_LENS = [1, 63, 64, 255, 256, 257, 511, 512, 513, 768]
CLASSES = [0, 1, 63, 64, 255, 256, 257, 511, 512, 513]  # + a multiple of 256 above 512
T_A, T_B, T_C, T_H, T_H1, T_H2, T_LOW1, T_LOW2, T_D = (len(E_LENS) + i for i in range(9))


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def world(S, O):
    n_docs = N_SUB * SUB
    rng = np.random.default_rng(2024)
    lens = rng.choice([50, 90, 130, 400], n_docs)
    tf = lambda n: rng.geometric(0.5, n).clip(1, 60)
    lists = []
    for L in E_LENS:
        d = np.sort(rng.choice(SUB, L, replace=False)) + 3 * SUB
        lists.append((d, tf(L)))
    for df in (0.30, 0.10, 0.50):  # A, B, C: the probed lists
        d = np.sort(rng.choice(n_docs, int(df * n_docs), replace=False))
        lists.append((d, tf(len(d))))
    # H: rare, large tf -- its docs alone outrank anything LOW1 and LOW2 can add.  H1, H2: rare, disjoint, alike: a top-k holds docs of both
    hd = np.sort(rng.choice(n_docs, 900, replace=False))
    lists.append((hd[:300], rng.integers(8, 40, 300)))
    lists.append((hd[300:600], tf(300)))
    lists.append((hd[600:], tf(300)))
    for df in (0.93, 0.97):  # LOW1, LOW2: in nearly every doc, tf 1 -- tiny upper bounds
        d = np.sort(rng.choice(n_docs, int(df * n_docs), replace=False))
        lists.append((d, np.ones(len(d), np.int64)))
    d = np.concatenate([np.sort(rng.choice(SUB, c, replace=False)) + s * SUB for s, c in enumerate(D_COUNTS)])
    lists.append((d, tf(len(d))))
    assert len(lists) == T_D + 1
    arrays = _hand_corpus(O, n_docs, lens, lists)
    sh, osh = _shards(S, O, n_docs, *arrays)
    yield sh, osh, lists
    sh.close()


def _part_lengths(docs, P):
    """postings of a list inside each of the P partitions of the sub-block range (the kernels' rule: sub-blocks n_sub p / P .. n_sub (p + 1) / P)"""
    edges = np.array([(N_SUB * p) // P for p in range(P + 1)], np.int64) * SUB
    return np.diff(np.searchsorted(docs, edges)).tolist()


def test_every_length_class_occurs(world):
    """the corpus does what it was built for: the drivers of the tests below see every stream length the issue lists, at every P"""
    _, _, lists = world
    drivers = list(range(len(E_LENS))) + [T_D]
    for P in (1, 2, N_SUB):
        seen = set()
        for t in drivers:
            seen.update(_part_lengths(lists[t][0], P))
        if P == N_SUB:
            assert set(CLASSES) <= seen, (P, sorted(set(CLASSES) - seen))
            assert seen >= {768, 1023, 1024, 1025, 1536, 2048}
        else:
            assert set(CLASSES) - {0 if P == 1 else None} <= seen, (P, sorted(set(CLASSES) - seen))  # (P = 1: no list is empty)
        assert any(x > 512 and x % 256 == 0 for x in seen), P
    # partitions that end in the middle of a group with the next partition's postings directly behind; the last list ends in one
    per_sub = _part_lengths(lists[T_D][0], N_SUB)
    assert per_sub == D_COUNTS and per_sub[-1] % 256 != 0
    assert sum(1 for a, b in zip(per_sub, per_sub[1:]) if a % 256 and b) >= 6
    assert len(lists[T_D][0]) < min(len(lists[T_A][0]), len(lists[T_C][0]))  # D drives the intersection [D, A, C]
    assert all(len(lists[t][0]) < len(lists[T_B][0]) for t in range(len(E_LENS)))  # E_L drives [E_L, A, B]


def _batches():
    """(name, query type is an intersection, term lists): <= 64 queries each, one body instantiation (2, 3 or 4 lists) per batch"""
    drivers = list(range(len(E_LENS))) + [T_D]
    return [("or2", False, [[t, T_A] for t in drivers] + [[T_A, T_D], [T_B, T_D]]),
            ("or3", False, [[t, T_A, T_B] for t in drivers] + [[T_B, T_D, T_A], [T_D, T_H1, T_H2]]),
            ("or4", False, [[t, T_A, T_B, T_C] for t in drivers] + [[T_C, T_B, T_D, T_A]]),
            ("and3", True, [[t, T_A, T_B] for t in drivers[:-1]] + [[T_D, T_A, T_C], [T_C, T_D, T_A]]),
            ("and2", True, [[t, T_A] for t in drivers])]


@pytest.fixture()
def partitions(request):
    old = os.environ.get("SS_BM25_P")
    os.environ["SS_BM25_P"] = str(request.param)
    yield request.param
    if old is None:
        os.environ.pop("SS_BM25_P", None)
    else:
        os.environ["SS_BM25_P"] = old


@pytest.mark.parametrize("partitions", [1, 2, N_SUB], indirect=True)
@pytest.mark.parametrize("tombstones", [False, True])
def test_stream_lengths(S, O, world, partitions, tombstones):
    sh, osh, lists = world
    rng = np.random.default_rng(5)
    # tombstones: a fortieth of all docs and every fourth doc of the drivers (postings that die after they were read)
    gone = np.unique(np.concatenate([rng.integers(0, N_SUB * SUB, N_SUB * SUB // 40)] + [lists[t][0][::4] for t in list(range(len(E_LENS))) + [T_D]]))
    try:
        if tombstones:
            sh.set_deleted(gone.astype(np.uint64)); osh.set_deleted([int(x) for x in gone])
        for name, is_and, tl in _batches():
            qt, op = (S.QueryType.Intersection, O.OP_AND) if is_and else (S.QueryType.Union, O.OP_OR)
            for k in (10, 100):
                for rt in (S.ResultType.Topk, S.ResultType.TopkCount):
                    got = _both_paths(S, sh, tl, qt, k, rt, what=(name, partitions, tombstones))
                    _oracle(O, osh, got, tl, op, k, rt, S, (0, 5, len(tl) - 1))
    finally:
        sh.set_deleted([]); osh.set_deleted([])


@pytest.mark.parametrize("partitions", [1, N_SUB], indirect=True)
@pytest.mark.parametrize("tombstones", [False, True])
def test_later_streams_skipped_and_needed(S, O, world, partitions, tombstones):
    """[H, LOW1, LOW2]: once H has been read the k-th best score lies above everything LOW1 and LOW2 can reach together -- their streams end
    before they read anything.  [H1, H2, LOW1] and [H1, H2]: docs that are in H2 alone stand in the top-k -- the second stream must run.
    Under tombstones no threshold seed is known before the first stream begins."""
    sh, osh, lists = world
    gone = np.concatenate([lists[T_H][0][::7], lists[T_H1][0][::5], lists[T_H2][0][::5]])
    try:
        if tombstones:
            sh.set_deleted(gone.astype(np.uint64)); osh.set_deleted([int(x) for x in gone])
        for k in (1, 10):
            tl = [[T_H, T_LOW1, T_LOW2], [T_LOW2, T_H, T_LOW1]]
            got = _both_paths(S, sh, tl, S.QueryType.Union, k, S.ResultType.Topk, what=("skipped", partitions, tombstones))
            _oracle(O, osh, got, tl, O.OP_OR, k, S.ResultType.Topk, S, (0, 1))
            # the scenario holds: the k-th best score exceeds the sum of the two low lists' best scores (their upper bounds)
            low = sum(float(osh.search_exhaustive([t], O.OP_OR, 1)[1][0]) for t in (T_LOW1, T_LOW2))
            assert float(got[1][0][k - 1]) > 1.01 * low
            assert set(got[0][0][:k].tolist()) <= set(lists[T_H][0].tolist())
            for tl in ([[T_H1, T_H2, T_LOW1], [T_H2, T_LOW1, T_H1]], [[T_H1, T_H2], [T_H2, T_H1]]):
                got = _both_paths(S, sh, tl, S.QueryType.Union, 10, S.ResultType.Topk, what=("needed", partitions, tombstones))
                _oracle(O, osh, got, tl, O.OP_OR, 10, S.ResultType.Topk, S, (0, 1))
                top = set(got[0][0][:10].tolist())
                assert top & set(lists[T_H1][0].tolist()) and top & set(lists[T_H2][0].tolist())
            got = _both_paths(S, sh, tl, S.QueryType.Union, k, S.ResultType.TopkCount, what=("needed, counts", partitions, tombstones))
    finally:
        sh.set_deleted([]); osh.set_deleted([])
