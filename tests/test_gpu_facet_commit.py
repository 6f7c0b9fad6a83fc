"""The facet image committed level by level: ss_facet_append_level / ss_facet_reserve / ss_facet_info (-m gpu).

Every output is an integer or a stored bit pattern, so every comparison is ==.  The expectations are numpy, written here as
tests/test_gpu_browse.py writes them: boolean masks for filters, np.lexsort for orders, np.bincount for facet counters -- and after
every step everything also equals a FRESH shard given one ss_facet_upload of the same prefix.

Levels: 65 536 docs, + 5, level 1 re-committed with 4 097 and then with 65 536, + 1 (level 2): the smallest sizes that exercise a full
level, a partial one, its replacement and the next level.  The i32 column falls with the doc id in steps of three docs, so a page
sorted by (i32 descending, doc id) can be placed across the level seam at doc 65 536 (three docs share a value and tie by doc id, the
larger first); the docs around the seam are given a string id and a location that pass the filter."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVEL = 65536
N_ALL = 2 * LEVEL + 1
REC = np.dtype([("i32", "<i4"), ("f32", "<f4"), ("s16", "<u2"), ("s32", "<u4"), ("u16", "<u2"), ("loc", "<u8")])
OFF = {n: REC.fields[n][1] for n in REC.names}
TYPE = {"i32": "i32", "f32": "f32", "s16": "string16", "s32": "string32", "u16": "u16", "loc": "point"}
BASE, UNIT = (38.8951, 30.25), "km"
S16_IDS = 49
DF = [0.6, 0.25, 0.05]
IDS = list(range(0, S16_IDS, 2))  # more than 8 ids: the extern id array
I32_LO, I32_HI = -30_000, 13_000  # the first 2 000 docs or so fail it
# (level, docs of the level) of every step, and the docs held after it
STEPS = [(0, LEVEL), (1, 5), (1, 4097), (1, LEVEL), (2, 1)]
SS_EINVAL = -1


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


@pytest.fixture(scope="module")
def world(O):
    """the corpus, its records and every numpy expectation that does not depend on the step: computed once, never written again"""
    W = World()
    rng = np.random.default_rng(77)
    offs, docs, tfs = [0], [], []
    for df in DF:
        d = np.sort(rng.choice(N_ALL, int(df * N_ALL), replace=False)).astype(np.uint32)
        docs.append(d); tfs.append(np.minimum(rng.geometric(0.6, len(d)), 60).astype(np.uint16)); offs.append(offs[-1] + len(d))
    W.offs, W.docs, W.tfs = np.asarray(offs, np.uint64), np.concatenate(docs), np.concatenate(tfs)
    W.dl = O.lex_doclen(N_ALL)
    v = np.zeros(N_ALL, REC)
    v["i32"] = -30_000 + (N_ALL - 1 - np.arange(N_ALL)) // 3  # falls with the doc id, three docs per value
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf])
    pick = rng.integers(0, 3, N_ALL) == 0
    v["f32"] = np.where(pick, special[rng.integers(0, len(special), N_ALL)], rng.normal(0.0, 50.0, N_ALL)).astype(np.float32)
    v["s16"] = rng.integers(0, S16_IDS, N_ALL)
    v["s32"] = rng.integers(0, 100_000, N_ALL)
    v["u16"] = rng.integers(0, 65536, N_ALL)
    lat, lon = rng.random(N_ALL) * 50.0 + 10.0, rng.random(N_ALL) * 60.0 + 5.0
    near = np.r_[LEVEL - 8:LEVEL + 8, 2 * LEVEL - 8:N_ALL]  # around both seams: pass the filter for sure
    v["s16"][near] = IDS[3]
    lat[near], lon[near] = BASE[0] + 9.0, BASE[1]
    v["loc"] = O.morton_encode(lat, lon)
    W.v = v
    W.raw = np.ascontiguousarray(v.view(np.uint8).reshape(N_ALL, REC.itemsize))
    W.dist = O.geo_distances(v["loc"], BASE, UNIT)
    m0, m1 = O.geo_morton_range(BASE, 2500.0, UNIT)
    W.flt = [(OFF["i32"], "i32", I32_LO, I32_HI), (OFF["s16"], "string16", IDS), (OFF["loc"], "point", BASE, 300.0, 2500.0, UNIT)]
    W.keep = ((v["i32"] >= I32_LO) & (v["i32"] < I32_HI) & np.isin(v["s16"], IDS) & (v["loc"] >= np.uint64(m0)) & (v["loc"] < np.uint64(m1)) &
              (W.dist >= 300.0) & (W.dist < 2500.0))
    assert W.keep[near].all()
    W.in_list = np.zeros(N_ALL, bool)
    W.in_list[W.docs] = True  # the union of the three lists
    return W


def _csr(W, lo, hi):
    """the postings of docs [lo, hi), doc ids as they are"""
    o, d, t = [0], [], []
    for i in range(len(DF)):
        a, b = int(W.offs[i]), int(W.offs[i + 1])
        i0, i1 = a + int(np.searchsorted(W.docs[a:b], lo)), a + int(np.searchsorted(W.docs[a:b], hi))
        d.append(W.docs[i0:i1]); t.append(W.tfs[i0:i1]); o.append(o[-1] + (i1 - i0))
    return np.asarray(o, np.uint64), np.concatenate(d), np.concatenate(t)


def _fresh(S, W, n):
    """a shard given ONE lexical upload and ONE ss_facet_upload of the first n docs"""
    sh = S.Shard(0)
    sh.upload_lexical(n, W.dl[:n], *_csr(W, 0, n))
    sh.upload_facets(W.raw[:n])
    return sh


def _facets():
    r = lambda bounds: [("r%d" % i, b) for i, b in enumerate(bounds)]
    return [
        {"field": "i32", "offset": OFF["i32"], "type": "i32", "ranges": r([-(1 << 31), -20_000, -5, 0, 7, 10_000]), "range_type": "within"},
        {"field": "f32", "offset": OFF["f32"], "type": "f32", "ranges": r([-50.0, -1.0, 0.0, 1.0, 25.0]), "range_type": "within"},
        {"field": "loc", "offset": OFF["loc"], "type": "point", "ranges": r([0.0, 500.0, 1000.0, 2000.0, 3000.0]), "range_type": "within",
         "base": BASE, "unit": UNIT},
        {"field": "s16", "offset": OFF["s16"], "type": "string16", "values": ["a%d" % i for i in range(40)], "prefix": "", "length": 10},
        {"field": "s32", "offset": OFF["s32"], "type": "string32", "values": ["b%d" % i for i in range(1000)], "prefix": "", "length": 10},
        {"field": "u16", "offset": OFF["u16"], "type": "u16", "ranges": r([100, 20_000, 65_535]), "range_type": "within"},
    ]


def _want_counts(W, qf, docs):
    if qf["type"].startswith("string"):
        nb = len(qf["values"])
        ids = W.v[qf["field"]][docs].astype(np.int64)
        return np.bincount(np.where(ids < nb, ids, nb), minlength=nb + 1).astype(np.uint64)
    bounds = [b for _, b in qf["ranges"]]
    nb = len(bounds)
    if qf["type"] == "point":
        x, bs = W.dist[docs], np.asarray(bounds, np.float64)
    elif qf["type"] == "f32":
        x, bs = W.v["f32"][docs], np.asarray(bounds, np.float32)
    else:
        x, bs = W.v[qf["field"]][docs].astype(np.int64), np.asarray(bounds, np.int64)
    b = np.searchsorted(bs, x, side="right").astype(np.int64) - 1
    return np.bincount(np.where(b < 0, nb, b), minlength=nb + 1).astype(np.uint64)


def _bits(W, name, n):
    """the stored bits of a column, zero-extended as ss_facet_values returns them"""
    col = W.v[name][:n]
    return col.view("<u%d" % col.dtype.itemsize).astype(np.uint64)


def _values(sh, n):
    """every column of every doc, as stored bits"""
    docs = np.arange(n, dtype=np.uint32)
    return [sh.facet_values(docs, OFF[name], TYPE[name]) for name in REC.names]


def _check(S, W, sh, n, what):
    """the shard holds exactly the first n records: values, a filtered search, a sorted page across the seam and its counters --
    against numpy and against a fresh shard given one upload of the prefix"""
    ref = _fresh(S, W, n)
    try:
        assert sh.facet_info()[:2] == (n, REC.itemsize), what
        got, ref_vals = _values(sh, n), _values(ref, n)
        for name, g, r in zip(REC.names, got, ref_vals):
            assert np.array_equal(g, _bits(W, name, n)), (what, name)
            assert np.array_equal(g, r), (what, name)
        # a filtered search: the matches are the docs of the three lists that pass the filter
        q = sh.make_queries([[0, 1, 2]], S.QueryType.Union)
        a = sh.search_lexical_batch(q, 50, S.ResultType.TopkCount, facet_filter=W.flt)
        b = ref.search_lexical_batch(ref.make_queries([[0, 1, 2]], S.QueryType.Union), 50, S.ResultType.TopkCount, facet_filter=W.flt)
        hit = W.keep[:n] & W.in_list[:n]
        assert int(a[3][0]) == int(hit.sum()) and int(a[2][0]) == min(50, int(hit.sum())), what
        assert hit[a[0][0][:a[2][0]]].all(), what
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), what
        # the empty query under the filter, sorted by (i32 descending, the larger doc id first): a page across the level seam
        docs = np.nonzero(W.keep[:n])[0]
        order = docs[np.lexsort([-docs, -W.v["i32"][docs].astype(np.int64)])]
        below = int((docs < LEVEL).sum())  # i32 falls with the doc id: the docs of level 0 come first
        skip, k = max(0, below - 5), 12
        page = order[skip:skip + k]
        if n > LEVEL:
            assert (page < LEVEL).any() and (page >= LEVEL).any(), what
        qfs = _facets()
        sorts = [(OFF["i32"], "i32", True)]
        d, cnt, tot, per = sh.search_docs_raw(k, S.ResultType.TopkCount, W.flt, sorts, qfs, skip=skip)
        assert tot == len(docs) and cnt == len(page) and np.array_equal(d, page), what
        for qf, c in zip(qfs, per):
            assert np.array_equal(c, _want_counts(W, qf, docs)), (what, qf["field"])
        d2, cnt2, tot2, per2 = ref.search_docs_raw(k, S.ResultType.TopkCount, W.flt, sorts, qfs, skip=skip)
        assert np.array_equal(d, d2) and (cnt, tot) == (cnt2, tot2) and all(np.array_equal(x, y) for x, y in zip(per, per2)), what
    finally:
        ref.close()


@pytest.mark.parametrize("reserve", [False, True])
def test_levels_appended_and_recommitted_equal_one_upload(S, world, reserve):
    """the five steps on an empty shard: the facets first, the lexical level second, everything checked after each step.  Without
    reserved room the second append must grow the image (by half, as the vector image grows); with the room reserved -- before the
    first level -- the capacity never moves."""
    W = world
    sh = S.Shard(0)
    try:
        assert sh.facet_info() == (0, 0, 0, 0)
        if reserve:
            sh.reserve_facets(N_ALL + 1000)
            assert sh.facet_info() == (0, 0, N_ALL + 1000, 0)
        caps = []
        for level, nl in STEPS:
            lo, n = level * LEVEL, level * LEVEL + nl
            sh.append_facet_level(level, W.raw[lo:n])
            sh.append_level(level, W.dl[lo:n], *_csr(W, lo, n))
            caps.append(sh.facet_info()[2])
            _check(S, W, sh, n, ("reserve", reserve, level, nl))
        if reserve:
            assert caps == [N_ALL + 1000] * len(STEPS)
        else:
            # exactly the first level; the second append grows it by half; the full second level by half again
            assert caps == [LEVEL, 98_304, 98_304, 147_456, 147_456]
        # room taken later: the records stay
        sh.reserve_facets(4 * LEVEL)
        assert sh.facet_info() == (N_ALL, REC.itemsize, 4 * LEVEL, 0)
        assert all(np.array_equal(a, _bits(W, name, N_ALL)) for name, a in zip(REC.names, _values(sh, N_ALL)))
    finally:
        sh.close()


def test_levels_appended_onto_an_upload(S, world):
    """an image that came from ss_facet_upload is continued the same way: 70 000 docs are level 0 and a partial level 1"""
    W = world
    sh = S.Shard(0)
    try:
        n = 70_000
        sh.upload_facets(W.raw[:n])
        assert sh.facet_info() == (n, REC.itemsize, n, 0)
        for level, nl in [(1, 5000), (1, LEVEL), (2, 1)]:
            lo, n = level * LEVEL, level * LEVEL + nl
            sh.append_facet_level(level, W.raw[lo:n])
            sh.upload_lexical(n, W.dl[:n], *_csr(W, 0, n))
            _check(S, W, sh, n, ("onto an upload", level, nl))
        # an upload in turn drops the reserved room with the image it replaces
        sh.reserve_facets(3 * LEVEL)
        sh.upload_facets(W.raw[:100])
        assert sh.facet_info() == (100, REC.itemsize, 100, 0)
    finally:
        sh.close()


def test_facets_may_run_ahead_of_the_lexical_image(S, world):
    """facets appended first, the lexical level second: between the two calls no facet-reading entry answers SS_ESTATE, and the answers
    are those of the lexical image's docs"""
    W = world
    sh = S.Shard(0)
    try:
        n0 = 5000
        sh.append_facet_level(0, W.raw[:n0])
        sh.append_level(0, W.dl[:n0], *_csr(W, 0, n0))
        sh.append_facet_level(0, W.raw[:LEVEL])  # the lexical image still holds n0 docs
        docs = np.nonzero(W.keep[:n0])[0]
        d, cnt, tot, _ = sh.search_docs_raw(10, S.ResultType.TopkCount, W.flt, [(OFF["i32"], "i32", True)])
        assert tot == len(docs) and np.array_equal(d, docs[np.lexsort([-docs, -W.v["i32"][docs].astype(np.int64)])][:10])
        a = sh.search_lexical_batch(sh.make_queries([[0, 1, 2]], S.QueryType.Union), 10, S.ResultType.TopkCount, facet_filter=W.flt)
        assert int(a[3][0]) == int((W.keep[:n0] & W.in_list[:n0]).sum())
    finally:
        sh.close()


def test_refused_levels_change_nothing(S, world):
    """every refusal of ss_facet_append_level: SS_EINVAL, and facet_info and every stored value as before"""
    from seekstorm_amd import _native as N
    W = world
    L = N.lib()
    sh = S.Shard(0)
    try:
        def call(level, n_docs, record_size, rows, null=False):
            r = np.ascontiguousarray(rows)
            return L.ss_facet_append_level(sh._h, level, n_docs, record_size, None if null else N.ptr(r, N.u8p))
        rs = REC.itemsize
        # no image yet: the first level is level 0
        assert call(1, 5, rs, W.raw[LEVEL:LEVEL + 5]) == SS_EINVAL
        assert sh.facet_info() == (0, 0, 0, 0)
        n = LEVEL + 5
        sh.append_facet_level(0, W.raw[:LEVEL])
        sh.append_facet_level(1, W.raw[LEVEL:n])
        info, vals = sh.facet_info(), _values(sh, n)
        other = np.zeros((70_000, rs), np.uint8)  # what a refused call must not leave anywhere
        refusals = [
            ("null records", call(1, 6, rs, other, null=True)),
            ("null shard", L.ss_facet_append_level(None, 1, 6, rs, N.ptr(other, N.u8p))),
            ("no docs", call(1, 0, rs, other)),
            ("more than a level", call(1, LEVEL + 1, rs, other)),
            ("another record size", call(1, 6, rs + 4, other)),
            ("a record size of 0", call(1, 6, 0, other)),
            ("beyond the next level", call(3, 6, rs, other)),
            ("older than the last level", call(0, LEVEL, rs, other)),
            ("a new level while the last is incomplete", call(2, 6, rs, other)),
            ("a shrinking re-commit", call(1, 4, rs, other)),
        ]
        for what, rc in refusals:
            assert rc == SS_EINVAL, what
        assert sh.facet_info() == info
        assert all(np.array_equal(a, b) for a, b in zip(vals, _values(sh, n)))
        # the same size is no shrinking: the level is replaced
        sh.append_facet_level(1, W.raw[LEVEL + 100:LEVEL + 105])
        assert np.array_equal(sh.facet_values(np.arange(LEVEL, n, dtype=np.uint32), OFF["u16"], "u16"), W.v["u16"][LEVEL + 100:LEVEL + 105].astype(np.uint64))
    finally:
        sh.close()
