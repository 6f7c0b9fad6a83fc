"""The empty query: ss_docs_search (csrc/browse.hip), Shard.search_docs and Index.search(enable_empty_query=True), both mirrors (-m gpu).

Every output is an integer, so every comparison is ==.  The expectations are numpy, written here: the match set is "not tombstoned and
passes the filter", the order is np.lexsort by (the sort fields, then the doc id in the tie direction), a facet's counters are
np.bincount over the bucket rule of tests/test_gpu_query_facets.py.  No NaN in a sort field.

Sizes: 5 docs (shorter than one 64-bit word), 4097 (the second 4096-doc sub-block holds ONE doc and 4095 padded bits that must never
be emitted), 20 003 (two 16 384-doc slices of the bitmap, the second partial).  Tombstones at 0, 63, 64, 4095, 4096, n - 1 and a random
30 %."""
import ctypes as C

import numpy as np
import pytest

from test_query_facets_host import _spec, host_lib, parse_facets_text, ref_planner, ref_shard_map, same_facet

pytestmark = pytest.mark.gpu

SIZES = [5, 4097, 20_003]
REC = np.dtype([("grade", "<i4"), ("i32", "<i4"), ("f32", "<f4"), ("s16", "<u2"), ("u16", "<u2"), ("loc", "<u8")])
OFF = {n: REC.fields[n][1] for n in REC.names}
BASE, UNIT = (38.8951, 30.25), "km"
S16_BUCKETS = 40
SENTINEL = 0xABABABAB
DF = [0.6, 0.25, 0.05]


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


def _lists(n_docs, seed):
    rng = np.random.default_rng(seed)
    offs, docs, tfs = [0], [], []
    for df in DF:
        d = np.sort(rng.choice(n_docs, max(1, int(df * n_docs)), replace=False)).astype(np.uint32)
        docs.append(d); tfs.append(np.minimum(rng.geometric(0.6, len(d)), 60).astype(np.uint16)); offs.append(offs[-1] + len(d))
    return np.asarray(offs, np.uint64), np.concatenate(docs), np.concatenate(tfs)


def _records(O, n_docs, seed):
    rng = np.random.default_rng(seed)
    v = np.zeros(n_docs, REC)
    v["grade"] = rng.integers(-1, 3, n_docs)  # 4 distinct values: tie groups far larger than any k
    v["i32"] = rng.integers(-(1 << 31), 1 << 31, n_docs)
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf])
    pick = rng.integers(0, 3, n_docs) == 0
    v["f32"] = np.where(pick, special[rng.integers(0, len(special), n_docs)], rng.normal(0.0, 50.0, n_docs)).astype(np.float32)
    v["s16"] = rng.integers(0, S16_BUCKETS + 9, n_docs)
    v["u16"] = rng.integers(0, 65536, n_docs)
    v["loc"] = O.morton_encode(rng.random(n_docs) * 50.0 + 10.0, rng.random(n_docs) * 60.0 + 5.0)
    return v


def _gone(n_docs, seed):
    rng = np.random.default_rng(seed)
    edges = [d for d in (0, 63, 64, 4095, 4096, n_docs - 1) if 0 <= d < n_docs]
    return sorted(set(edges) | set(np.nonzero(rng.random(n_docs) < 0.3)[0].tolist()))


def _world(S, O, n_docs, seed=5, shard_id=0, image="plain"):
    """image: plain | sparse (a sparse tier appended) | fields3 (three indexed fields) | budget3 (probe rows for three lists only)"""
    W = World()
    W.n_docs = n_docs
    dl = O.lex_doclen(n_docs)
    offs, docs, tfs = _lists(n_docs, seed)
    W.sh = S.Shard(0, shard_id=shard_id)
    if image == "budget3":
        W.sh.set_probe_budget((3 + 1) * ((n_docs + 4095) // 4096) * 64 * 12)
    if image == "fields3":
        W.sh.upload_lexical_fields(n_docs, np.stack([dl, dl, dl]), np.array([1.5, 1.0, 0.5], np.float32), offs, docs, (docs % 3).astype(np.uint8), tfs)
    else:
        W.sh.upload_lexical(n_docs, dl, offs, docs, tfs)
    if image == "sparse":
        rng = np.random.default_rng(seed + 9)
        sd = np.sort(rng.choice(n_docs, 40, replace=False)).astype(np.uint32)
        assert W.sh.append_sparse(np.array([0, 40], np.uint64), sd, np.ones(40, np.uint16)) == len(DF)
    W.v = _records(O, n_docs, seed + 1)
    W.sh.upload_facets(np.ascontiguousarray(W.v.view(np.uint8).reshape(n_docs, REC.itemsize)))
    W.gone = _gone(n_docs, seed + 2)
    W.sh.set_deleted(W.gone)
    W.alive = np.ones(n_docs, bool)
    W.alive[W.gone] = False
    W.dist = O.geo_distances(W.v["loc"], BASE, UNIT)
    W.sortkey = O.geo_distances(W.v["loc"], BASE, "sortkey")
    return W


@pytest.fixture(scope="module")
def worlds(S, O):
    made = {}

    def get(n_docs, image="plain"):
        if (n_docs, image) not in made:
            made[(n_docs, image)] = _world(S, O, n_docs, image=image)
        return made[(n_docs, image)]
    yield get
    for W in made.values():
        W.sh.close()


# ------------------------------------------------------------------------------------------------ the statement, in numpy
def _filters(O, W):
    """every facet-filter kind of the world: (name, the mirror's filter list, the docs that pass)"""
    m0, m1 = O.geo_morton_range(BASE, 2500.0, UNIT)
    ids = [1, 5, 8, 13, 21, 34, 39, 44]
    many = list(range(0, S16_BUCKETS + 9, 2))  # more than 8 ids: the extern id array
    return [
        ("range", [(OFF["u16"], "u16", 10_000, 52_000)], (W.v["u16"] >= 10_000) & (W.v["u16"] < 52_000)),
        ("f32", [(OFF["f32"], "f32", 0.0, 60.0)], (W.v["f32"] >= 0.0) & (W.v["f32"] < 60.0)),
        ("ids", [(OFF["s16"], "string16", ids)], np.isin(W.v["s16"], ids)),
        ("many ids", [(OFF["s16"], "string16", many)], np.isin(W.v["s16"], many)),
        ("point", [(OFF["loc"], "point", BASE, 300.0, 2500.0, UNIT)],
         (W.v["loc"] >= np.uint64(m0)) & (W.v["loc"] < np.uint64(m1)) & (W.dist >= 300.0) & (W.dist < 2500.0)),
        ("two", [(OFF["u16"], "u16", 10_000, 52_000), (OFF["grade"], "i32", 0, 2)],
         (W.v["u16"] >= 10_000) & (W.v["u16"] < 52_000) & (W.v["grade"] >= 0) & (W.v["grade"] < 2)),
    ]


def _ranges(bounds):
    return [("r%d" % i, b) for i, b in enumerate(bounds)]


def _facets():
    return [
        {"field": "i32", "offset": OFF["i32"], "type": "i32", "ranges": _ranges([-(1 << 31), -1_000_000_000, -5, 0, 7, 1_500_000_000]), "range_type": "within"},
        {"field": "f32", "offset": OFF["f32"], "type": "f32", "ranges": _ranges([-50.0, -1.0, 0.0, 1.0, 25.0]), "range_type": "within"},
        {"field": "loc", "offset": OFF["loc"], "type": "point", "ranges": _ranges([0.0, 500.0, 1000.0, 2000.0, 3000.0]), "range_type": "within",
         "base": BASE, "unit": UNIT},
        {"field": "s16", "offset": OFF["s16"], "type": "string16", "values": ["a%d" % i for i in range(S16_BUCKETS)], "prefix": "", "length": 10},
        {"field": "u16", "offset": OFF["u16"], "type": "u16", "ranges": _ranges([100, 20_000, 65_535]), "range_type": "within"},
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


def _sort_column(W, sf):
    """one sort field as a float64 / int64 column where SMALLER = better"""
    off, ty, desc = sf[:3]
    if ty == "point":
        col = O_sortkey(W, sf[3])
    else:
        name = {OFF["grade"]: "grade", OFF["i32"]: "i32", OFF["f32"]: "f32"}[off]
        col = W.v[name].astype(np.float64 if ty == "f32" else np.int64)
    return -col if desc else col  # (-0.0 == +0.0 as numbers: they tie, as the library documents)


def O_sortkey(W, base):
    assert tuple(base) == BASE
    return W.sortkey


def _want_order(W, keep, sorts, ascending, gid=None):
    """all matching docs in answer order"""
    docs = np.nonzero(W.alive & keep)[0]
    ids = docs if gid is None else gid[docs]
    tie = ids if ascending else -ids.astype(np.int64)
    cols = [_sort_column(W, sf)[docs] for sf in sorts]
    return docs[np.lexsort([tie] + cols[::-1])]


SORTS = [
    [(OFF["i32"], "i32", False)], [(OFF["i32"], "i32", True)], [(OFF["f32"], "f32", False)], [(OFF["f32"], "f32", True)],
    [(OFF["loc"], "point", False, BASE)], [(OFF["loc"], "point", True, BASE)], [(OFF["grade"], "i32", False)],
    [(OFF["grade"], "i32", True), (OFF["f32"], "f32", False)], [(OFF["grade"], "i32", False), (OFF["loc"], "point", True, BASE)],
]


def _raw(S, W, k, rt=None, ascending=False, skip=0, sorts=(), flt=None, qfs=None, pad=8):
    """ss_docs_search itself, the doc buffer pre-filled with a sentinel -> (rc, docs, count, total, [counters per facet])"""
    from seekstorm_amd import _native as N
    rt = S.ResultType.TopkCount if rt is None else rt
    n, arr = W.sh._result_sorts(list(sorts))
    farr, nf = W.sh.facet_filters(flt) if flt else (None, 0)
    doc = np.full(int(k) + pad, SENTINEL, np.uint32)
    cnt, tot = C.c_uint32(0xFFFFFFFF), C.c_uint64(0xFFFFFFFFFFFFFFFF)
    off = ty = nb = allb = bases = out = None
    nqf = len(qfs) if qfs else 0
    if nqf:
        off, ty, nb, allb, bases, stride = W.sh._query_facet_args(qfs)
        out = np.full(stride, 0x5555, np.uint64)
    rc = N.lib().ss_docs_search(W.sh._h, int(skip), int(k), int(rt), 1 if ascending else 0, n, C.cast(arr, C.c_void_p) if n else None, nf,
                                None if farr is None else C.cast(farr, C.c_void_p), nqf, N.ptr(off, N.u32p), N.ptr(ty, N.u32p), N.ptr(nb, N.u32p),
                                N.ptr(allb, N.u64p), None if bases is None else C.cast(bases, C.c_void_p), N.ptr(doc, N.u32p), C.byref(cnt),
                                C.byref(tot), N.ptr(out, N.u64p))
    per, at = [], 0
    for b in (nb if nqf else []):
        per.append(out[at:at + int(b) + 1])
        at += int(b) + 1
    if rc == 0:
        assert cnt.value <= k and np.all(doc[cnt.value:] == SENTINEL), ("written beyond out_count", k, skip, cnt.value)
    return rc, doc[:cnt.value].astype(np.int64), int(cnt.value), int(tot.value), per


def _check_page(S, W, want_all, k, skip=0, what=None, **kw):
    rc, d, c, t, per = _raw(S, W, k, skip=skip, **kw)
    want = want_all[skip:skip + k]
    assert rc == 0, (what, rc)
    assert c == len(want) and t == len(want_all), (what, k, skip, c, len(want), t, len(want_all))
    assert np.array_equal(d, want), (what, k, skip, d[:8], want[:8], np.nonzero(d != want)[0][:4])
    return per


# ------------------------------------------------------------------------------------------------ by doc id
@pytest.mark.parametrize("n_docs", SIZES)
def test_doc_id_order_pages_of_any_depth(S, worlds, n_docs):
    W = worlds(n_docs)
    everybody = np.ones(n_docs, bool)
    live = int(W.alive.sum())
    assert 0 < live < n_docs
    for ascending in (False, True):
        want_all = _want_order(W, everybody, [], ascending)
        assert len(want_all) == live and (want_all[0] < want_all[-1]) == ascending
        for k in (1, 10, 1024, 3000, n_docs + 7):
            for skip in (0, 1, 63, 64, 5000, live, live + 1):
                _check_page(S, W, want_all, k, skip, ("by id", n_docs, ascending), ascending=ascending)
    # Topk: the same docs (the total is only promised to be >= the count); Count: no docs, the exact total
    rc, d, c, t, _ = _raw(S, W, 10, rt=S.ResultType.Topk)
    assert rc == 0 and np.array_equal(d, _want_order(W, everybody, [], False)[:10]) and t >= c
    rc, d, c, t, _ = _raw(S, W, 10, rt=S.ResultType.Count)
    assert rc == 0 and c == 0 and t == live
    # the Python mirror returns the same page
    d, c, t, fac = W.sh.search_docs(10, skip=1, doc_ascending=True)
    assert np.array_equal(d, _want_order(W, everybody, [], True)[1:11]) and c == len(d) and t == live and fac == {}


def test_nobody_left(S, O):
    """all docs tombstoned; a filter nobody passes: count 0, total 0, every counter zero"""
    W = _world(S, O, 4097, seed=77)
    try:
        qfs = _facets()
        nobody = [(OFF["u16"], "u16", 70, 70)]
        for sorts in ([], SORTS[0]):
            rc, d, c, t, per = _raw(S, W, 10, sorts=sorts, flt=nobody, qfs=qfs)
            assert rc == 0 and c == 0 and t == 0 and all(int(p.sum()) == 0 for p in per), (sorts, c, t)
        W.sh.set_deleted(list(range(W.n_docs)))
        for sorts in ([], SORTS[0]):
            for ascending in (False, True):
                rc, d, c, t, per = _raw(S, W, 10, sorts=sorts, qfs=qfs, ascending=ascending)
                assert rc == 0 and c == 0 and t == 0 and all(int(p.sum()) == 0 for p in per), (sorts, c, t)
    finally:
        W.sh.close()


# ------------------------------------------------------------------------------------------------ filters, facets, result types
@pytest.mark.parametrize("n_docs", SIZES)
def test_every_filter_kind_with_facets_and_result_types(S, O, worlds, n_docs):
    W = worlds(n_docs)
    qfs = _facets()
    for name, flt, keep in [("none", None, np.ones(n_docs, bool))] + _filters(O, W):
        want_all = _want_order(W, keep, [], False)
        counts = [_want_counts(W, qf, want_all) for qf in qfs]
        for rt in (S.ResultType.Count, S.ResultType.Topk, S.ResultType.TopkCount):
            rc, d, c, t, per = _raw(S, W, 25, rt=rt, flt=flt, qfs=qfs)
            assert rc == 0, (name, rt, rc)
            if rt == S.ResultType.Count:
                assert c == 0 and t == len(want_all), (name, c, t)
            else:
                assert np.array_equal(d, want_all[:25]), (name, rt)
                assert t == len(want_all) if rt == S.ResultType.TopkCount else t >= c
            for qf, got, want in zip(qfs, per, counts):  # (counted whatever the result type: include/seekstorm_hip.h)
                assert np.array_equal(got, want), (name, rt, qf["field"], got, want)
                assert int(got.sum()) == len(want_all)
        # ... and without query_facets, through the mirror
        d, c, t, fac = W.sh.search_docs(25, facet_filter=flt, doc_ascending=True)
        assert np.array_equal(d, want_all[::-1][:25]) and t == len(want_all) and fac == {}
    if n_docs == SIZES[-1]:
        assert all(0 < int((W.alive & keep).sum()) < int(W.alive.sum()) for _, _, keep in _filters(O, W))  # every filter filters


# ------------------------------------------------------------------------------------------------ sorts
@pytest.mark.parametrize("n_docs", SIZES)
@pytest.mark.parametrize("ascending", [False, True])
def test_sorted_pages(S, O, worlds, n_docs, ascending):
    """one and two fields, both directions, i32 / f32 with +-0.0 / Point, a 4-valued first field; k = 2500 runs in passes of SS_MAX_K"""
    W = worlds(n_docs)
    name, flt, keep = _filters(O, W)[0]
    for sorts in SORTS:
        want_all = _want_order(W, np.ones(n_docs, bool), sorts, ascending)
        for k in (10, 300, 1024, 2500):
            _check_page(S, W, want_all, k, 0, ("sorted", n_docs, sorts, ascending), sorts=sorts, ascending=ascending)
        _check_page(S, W, want_all, 10, 7, ("sorted, skip", sorts), sorts=sorts, ascending=ascending)
        _check_page(S, W, want_all, 100, 1500, ("sorted, deep skip", sorts), sorts=sorts, ascending=ascending)
        # under a filter, with facets beside it
        want_f = _want_order(W, keep, sorts, ascending)
        per = _check_page(S, W, want_f, 300, 0, ("sorted, filtered", sorts), sorts=sorts, ascending=ascending, flt=flt, qfs=_facets()[:2])
        for qf, got in zip(_facets()[:2], per):
            assert np.array_equal(got, _want_counts(W, qf, want_f)), (sorts, qf["field"])
    if n_docs == SIZES[-1]:
        grade = W.v["grade"][W.alive]
        assert len(np.unique(grade)) == 4 and np.bincount(grade + 1).min() > 2500  # every tie group of the 4-valued field exceeds every k
        z = W.v["f32"][W.alive]
        assert np.any((z == 0) & np.signbit(z)) and np.any((z == 0) & ~np.signbit(z))  # both zeros are among the keys
    # the mirror's `_id` marker: the last entry sets the tie direction
    d, c, t, _ = W.sh.search_docs(50, result_sort=SORTS[6] + [("_id", not ascending)])
    assert np.array_equal(d, _want_order(W, np.ones(n_docs, bool), SORTS[6], ascending)[:50])
    with pytest.raises(ValueError):
        W.sh.search_docs(50, result_sort=[("_id", True)] + SORTS[6])


# ------------------------------------------------------------------------------------------------ images that must not matter
@pytest.mark.parametrize("image", ["sparse", "fields3", "budget3"])
def test_the_image_makes_no_difference(S, O, worlds, image):
    """a sparse tier, three indexed fields, probe rows for three lists only: no posting list is read, so the answers are the plain image's"""
    n_docs = SIZES[-1]
    W = worlds(n_docs, image)
    if image == "fields3":
        assert W.sh.fields_info()[0] == 3
    if image == "sparse":
        assert W.sh.sparse_info()[0] >= 1
    qfs = _facets()
    name, flt, keep = _filters(O, W)[4]
    for ascending in (False, True):
        want_all = _want_order(W, np.ones(n_docs, bool), [], ascending)
        for k, skip in ((10, 0), (3000, 64), (n_docs + 7, 0)):
            _check_page(S, W, want_all, k, skip, (image, "by id"), ascending=ascending)
        want_f = _want_order(W, keep, [], ascending)
        per = _check_page(S, W, want_f, 10, 0, (image, "filtered"), ascending=ascending, flt=flt, qfs=qfs)
        for qf, got in zip(qfs, per):
            assert np.array_equal(got, _want_counts(W, qf, want_f)), (image, qf["field"])
        for sorts in (SORTS[3], SORTS[7]):
            for k in (10, 2500):
                _check_page(S, W, _want_order(W, keep, sorts, ascending), k, 0, (image, sorts), sorts=sorts, ascending=ascending, flt=flt)


# ------------------------------------------------------------------------------------------------ errors
def test_errors(S, O, worlds):
    from seekstorm_amd import _native as N
    W = worlds(4097)
    qf = _facets()[0]
    assert _raw(S, W, 10, qfs=[dict(qf, offset=REC.itemsize - 3)])[0] == N.SS_EINVAL     # a facet offset outside the record
    assert _raw(S, W, 10, sorts=[(REC.itemsize - 3, "i32", False)])[0] == N.SS_EINVAL    # ... a sort field's
    assert _raw(S, W, 10, flt=[(REC.itemsize - 1, "u16", 0, 5)])[0] == N.SS_EINVAL       # ... a filter's
    assert _raw(S, W, 0)[0] == N.SS_EINVAL and _raw(S, W, 0, rt=S.ResultType.Topk)[0] == N.SS_EINVAL  # k = 0 where docs are wanted
    assert _raw(S, W, 0, rt=S.ResultType.Count)[0] == N.SS_OK
    assert _raw(S, W, 10, rt=3)[0] == N.SS_EINVAL
    assert _raw(S, W, 10, sorts=[(OFF["s16"], "string16", False)])[0] == N.SS_EINVAL     # strings sort by the host's rank column
    assert _raw(S, W, 10, sorts=[(OFF["i32"], "i32", False)] * (N.SS_MAX_SORT_FIELDS + 1))[0] == N.SS_EINVAL
    assert _raw(S, W, 10, qfs=_facets())[0] == N.SS_OK  # (the arguments the cases above vary are valid)
    bare = World()
    bare.sh = S.Shard(0)
    try:
        assert _raw(S, bare, 10)[0] == N.SS_ESTATE  # no lexical image
        offs, docs, tfs = _lists(4097, 3)
        bare.sh.upload_lexical(4097, O.lex_doclen(4097), offs, docs, tfs)
        assert _raw(S, bare, 10)[0] == N.SS_OK      # by doc id no facet records are needed
        assert _raw(S, bare, 10, sorts=SORTS[0])[0] == N.SS_ESTATE
        assert _raw(S, bare, 10, flt=[(OFF["u16"], "u16", 0, 5)])[0] == N.SS_ESTATE
        assert _raw(S, bare, 10, qfs=[qf])[0] == N.SS_ESTATE
        with pytest.raises(N.SeekStormHipError) as e:
            bare.sh.search_docs(10, result_sort=SORTS[0])
        assert e.value.code == N.SS_ESTATE
    finally:
        bare.sh.close()


# ------------------------------------------------------------------------------------------------ non-interference
def test_a_browse_leaves_the_scored_entries_alone(S, O, worlds):
    """the compose kernel's browse instances and the shared facet workspace: a sorted search and a search with query_facets answer after
    a ss_docs_search call what they answered before it"""
    W = worlds(SIZES[-1])
    q = W.sh.make_queries([[0, 1], [1, 2], [2]], [S.QueryType.Union, S.QueryType.Intersection, S.QueryType.Union])
    flt = _filters(O, W)[0][1]
    qfs = _facets()

    def scored():
        a = W.sh.search_lexical_sorted_batch(q, SORTS[7], 50, facet_filter=flt)
        b = W.sh.search_lexical_sorted_batch(q[:1], SORTS[0], 1500)
        c = W.sh.search_lexical_facets(q, 20, qfs, S.ResultType.TopkCount, facet_filter=flt)
        return [np.asarray(x).copy() for x in a] + [np.asarray(x).copy() for x in b] + [np.asarray(x).copy() for x in c[:4]] + [x.copy() for x in c[4]]

    before = scored()
    assert int(before[2].min()) > 0  # (the searches match something)
    for sorts, k in (([], 3000), (SORTS[7], 300), (SORTS[1], 2500)):
        assert _raw(S, W, k, sorts=sorts, flt=flt, qfs=qfs)[0] == 0
        after = scored()
        assert len(after) == len(before) and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(before, after)), (sorts, k)


# ------------------------------------------------------------------------------------------------ two shards, both mirrors
class SortC(C.Structure):  # host_capi.cpp ssh_result_sort
    _fields_ = [("facet_offset", C.c_uint32), ("facet_type", C.c_uint32), ("descending", C.c_uint32), ("reserved", C.c_uint32), ("base", C.c_double * 2)]


def _cpp_search_empty(shards, offset, length, rt, flt_arr, n_flt, sorts, qfs):
    from seekstorm_amd import _native as N
    H = host_lib()
    H.ssh_index_adopt.restype = C.c_void_p
    H.ssh_index_adopt.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    H.ssh_index_destroy.argtypes = [C.c_void_p]
    H.ssh_index_search_empty.restype = C.c_int
    H.ssh_index_search_empty.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                         C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_int)]
    id_sort, fields = 0, list(sorts)
    if fields and isinstance(fields[-1][0], str):
        name, desc = fields.pop()
        id_sort = {"_id": 1, "_score": 3}[name] + (0 if desc else 1)
    arr = (SortC * max(len(fields), 1))()
    for i, sf in enumerate(fields):
        arr[i].facet_offset, arr[i].facet_type, arr[i].descending = int(sf[0]), N.FACET_TYPES[sf[1]], 1 if sf[2] else 0
        if sf[1] == "point":
            arr[i].base[0], arr[i].base[1] = sf[3]
    handles = (C.c_void_p * len(shards))(*[sh._h for sh in shards])
    ix = H.ssh_index_adopt(len(shards), handles, (C.c_int * len(shards))(*([0] * len(shards))))
    try:
        cap = offset + length + 1
        doc, score, meta = np.zeros(cap, np.uint64), np.ones(cap, np.float32), np.zeros(4, np.uint64)
        buf = C.create_string_buffer(1 << 18)
        flen = C.c_int(0)
        n = H.ssh_index_search_empty(ix, offset, length, int(rt), n_flt, None if flt_arr is None else C.cast(flt_arr, C.c_void_p),
                                     C.cast(arr, C.c_void_p), len(fields), id_sort, _spec(qfs or []), cap, doc.ctypes.data, score.ctypes.data,
                                     meta.ctypes.data, buf, len(buf), C.byref(flen))
        assert n >= 0 and flen.value >= 0 and int(meta[3]) == 0, (n, flen.value, meta)
        assert np.all(score[:n] == 0.0)
        return doc[:n].astype(np.int64), int(meta[1]), parse_facets_text(buf.value.decode())
    finally:
        H.ssh_index_destroy(ix)


def test_two_shard_index_both_paths_both_mirrors(S, O, worlds):
    W0 = worlds(SIZES[-1])
    W1 = _world(S, O, 4097, seed=41, shard_id=1)
    try:
        Ws = [W0, W1]
        ix = S.Index([W0.sh, W1.sh])
        n_all = W0.n_docs + W1.n_docs
        live_gid = np.sort(np.concatenate([np.nonzero(W.alive)[0] * 2 + sid for sid, W in enumerate(Ws)]))
        # ---- index path: by global id, tombstoned docs skipped, the total counts them
        for sorts, ascending in ((None, False), ([("_id", True)], False), ([("_id", False)], True), ([("_score", True)], False), ([("_score", False)], True)):
            for offset, length in ((0, 10), (3, 10), (5000, 2000), (len(live_gid) - 4, 10), (len(live_gid) + 1, 5)):
                want = (live_gid if ascending else live_gid[::-1])[offset:offset + length]
                ro = ix.search([], enable_empty_query=True, offset=offset, length=length, result_sort=sorts)
                assert [r.doc_id for r in ro.results] == want.tolist(), (sorts, offset)
                assert all(r.score == 0.0 for r in ro.results) and ro.result_count == len(want) and ro.result_count_total == n_all
                cd, ctot, _ = _cpp_search_empty([W0.sh, W1.sh], offset, length, S.ResultType.TopkCount, None, 0, sorts or [], None)
                assert np.array_equal(cd, want) and ctot == n_all, ("c++", sorts, offset)
        ro = ix.search([], enable_empty_query=True, result_type=S.ResultType.Count)
        assert ro.results == [] and ro.result_count_total == n_all
        assert n_all > len(live_gid)
        # ---- shard path: a filter, facets, sorts
        flt = [(OFF["u16"], "u16", 10_000, 52_000)]
        farr, nflt = W0.sh.facet_filters(flt)
        qfs = [dict(_facets()[0], range_type="above"), dict(_facets()[3], length=7), _facets()[2]]
        keeps = [(W.v["u16"] >= 10_000) & (W.v["u16"] < 52_000) for W in Ws]
        for sorts, ascending in (([], False), ([("_id", False)], True), (SORTS[7], False), (SORTS[4] + [("_id", False)], True), (SORTS[6] + [("_score", True)], False)):
            fields = [sf for sf in sorts if not isinstance(sf[0], str)]
            rows = []
            for sid, (W, keep) in enumerate(zip(Ws, keeps)):
                docs = np.nonzero(W.alive & keep)[0]
                rows.append((docs * 2 + sid, [_sort_column(W, sf)[docs] for sf in fields]))
            gid = np.concatenate([g for g, _ in rows])
            cols = [np.concatenate([c[f] for _, c in rows]) for f in range(len(fields))]
            order = gid[np.lexsort([gid if ascending else -gid] + cols[::-1])]
            with_facets = True  # (the shard path counts every requested facet for every counted doc, sorted or not: add_result.rs:226-230)
            for offset, length in ((0, 10), (7, 300), (1500, 1200)):
                want = order[offset:offset + length]
                ro = ix.search([], enable_empty_query=True, offset=offset, length=length, facet_filter=flt, result_sort=sorts, field_filter=[0],
                               query_facets=qfs if with_facets else None)
                assert [r.doc_id for r in ro.results] == want.tolist(), (sorts, offset)
                assert ro.result_count_total == len(order) and all(r.score == 0.0 for r in ro.results)
                cd, ctot, cfac = _cpp_search_empty([W0.sh, W1.sh], offset, length, S.ResultType.TopkCount, farr, nflt, sorts, qfs if with_facets else None)
                assert np.array_equal(cd, want) and ctot == len(order), ("c++", sorts, offset)
                if with_facets:
                    shard_lists = []
                    for W, keep in zip(Ws, keeps):
                        m = {}
                        for qf in qfs:
                            ref = ref_shard_map(qf, _want_counts(W, qf, np.nonzero(W.alive & keep)[0]), 2)
                            if ref is not None and ref[0]:
                                m[qf["field"]] = ref[0]
                        shard_lists.append(m)
                    wantf = ref_planner(qfs, shard_lists, S.ResultType.TopkCount)
                    for who, facets in (("python", ro.facets), ("c++", cfac)):
                        assert set(facets) == set(wantf), (who, set(facets) ^ set(wantf))
                        for field, (full, cut) in wantf.items():
                            same_facet([(a, int(c)) for a, c in facets[field]], full, cut, (who, field))
        assert len(order) < len(live_gid)  # the shard path's total counts live matches only
    finally:
        W1.sh.close()
