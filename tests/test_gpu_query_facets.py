"""A search's query_facets in the same call as its top-k (ss_bm25_search_facets, csrc/facet.hip "Facet counts of a BATCH"; -m gpu).

The world: 100 003 docs (the last 64-doc word of every bitmap is partial), 12 dense lists from 97 % of the docs down to 50 docs, 7
sparse-tier lists (one confined to a single 64-doc group), tombstones, and a packed facet record with one column of every type --
Point and both string widths included; the f32 / f64 columns hold +-0.0, NaN and infinities; `same` holds one value in every doc.

Every expectation comes from numpy over the oracle's match set (oracle.search_exhaustive with the filtered docs and the tombstones
deleted): counters == a histogram by the bucket rule "the last lower bound <= value, below the first or NaN -> other, a string id >=
n_buckets -> other", totals ==, hits by the rule of tests/test_gpu_shape_sweep.py::_check.  Agreement with the library's other entry
points (search_lexical_batch, Shard.facet_count) is asserted as well, as a second assertion, never as the reference."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_shape_sweep import _check
from test_query_facets_host import TYPE_CODE, _spec, host_lib, parse_facets_text, ref_planner, ref_shard_map, same_facet

pytestmark = pytest.mark.gpu

N_DOCS = 100_003
DENSE_DF = [0.97, 0.5, 0.3, 0.15, 0.08, 0.04, 0.02, 0.01, 0.005, 0.002, 0.001, 0.0005]
SPARSE_N = [3, 40, 300, 1200, 2500, 17]
ND = len(DENSE_DF)
ONE_GROUP = ND + len(SPARSE_N)  # a sparse list whose 5 docs share one 64-doc group
REC = np.dtype([("u8", "u1"), ("u16", "<u2"), ("u32", "<u4"), ("u64", "<u8"), ("i8", "i1"), ("i16", "<i2"), ("i32", "<i4"), ("i64", "<i8"),
                ("f32", "<f4"), ("f64", "<f8"), ("s16", "<u2"), ("s32", "<u4"), ("loc", "<u8"), ("same", "<u4")])
S16_BUCKETS, S32_BUCKETS = 256, 5000  # 5001 counters: more than any LDS budget holds, counted in global memory
BASE, UNIT = (38.8951, 30.25), "km"


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


def _corpus(O, n_docs, seed):
    rng = np.random.default_rng(seed)
    dl = O.lex_doclen(n_docs)
    offs, docs, tfs = [0], [], []
    for df in DENSE_DF:
        d = np.sort(rng.choice(n_docs, int(df * n_docs), replace=False)).astype(np.uint32)
        docs.append(d); tfs.append(np.minimum(rng.geometric(0.6, len(d)), 60).astype(np.uint16)); offs.append(offs[-1] + len(d))
    hot = np.sort(rng.choice(n_docs, 5000, replace=False))
    s_offs, s_docs, s_tfs = [0], [], []
    for n in SPARSE_N:
        d = np.sort(rng.choice(hot, n, replace=False)).astype(np.uint32)
        s_docs.append(d); s_tfs.append(np.minimum(rng.geometric(0.5, n), 30).astype(np.uint16)); s_offs.append(s_offs[-1] + n)
    g0 = (n_docs // 2 // 64) * 64
    d = (g0 + np.array([0, 7, 31, 32, 63])).astype(np.uint32)
    s_docs.append(d); s_tfs.append(np.array([1, 2, 3, 4, 5], np.uint16)); s_offs.append(s_offs[-1] + 5)
    return (dl, np.asarray(offs, np.uint64), np.concatenate(docs), np.concatenate(tfs), np.asarray(s_offs, np.uint64), np.concatenate(s_docs),
            np.concatenate(s_tfs), hot)


def _records(O, n_docs, seed):
    rng = np.random.default_rng(seed)
    v = np.zeros(n_docs, REC)
    v["u8"] = rng.integers(0, 256, n_docs)
    v["u16"] = rng.integers(0, 65536, n_docs)
    v["u32"] = rng.integers(0, 1 << 32, n_docs, dtype=np.uint64)
    v["u64"] = rng.integers(0, 1 << 63, n_docs, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n_docs).astype(np.uint64)
    v["i8"] = rng.integers(-128, 128, n_docs)
    v["i16"] = rng.integers(-32768, 32768, n_docs)
    v["i32"] = rng.integers(-(1 << 31), 1 << 31, n_docs)
    v["i64"] = rng.integers(-(1 << 63), (1 << 63) - 1, n_docs)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0])
    pick = rng.integers(0, 3, n_docs) == 0  # a third of the docs hold a special value
    f = rng.normal(0.0, 50.0, n_docs)
    v["f32"] = np.where(pick, special[rng.integers(0, len(special), n_docs)], f).astype(np.float32)
    f = rng.normal(0.0, 1e6, n_docs)
    v["f64"] = np.where(pick, special[rng.integers(0, len(special), n_docs)], f)
    v["s16"] = rng.integers(0, S16_BUCKETS + 44, n_docs)
    v["s32"] = np.minimum(rng.zipf(1.3, n_docs), S32_BUCKETS + 1000)
    v["s32"][::1000] = 0xFFFFFFF0
    v["loc"] = O.morton_encode(rng.random(n_docs) * 50.0 + 10.0, rng.random(n_docs) * 60.0 + 5.0)
    v["same"] = 77
    return v


def _world(S, O, n_docs=N_DOCS, seed=31, shard_id=0):
    W = World()
    W.n_docs = n_docs
    dl, d_offs, d_docs, d_tfs, s_offs, s_docs, s_tfs, W.hot = _corpus(O, n_docs, seed)
    W.osh = O.Shard(n_docs, dl, np.concatenate([d_offs, d_offs[-1] + s_offs[1:]]), np.concatenate([d_docs, s_docs]), np.concatenate([d_tfs, s_tfs]))
    W.v = _records(O, n_docs, seed + 1)
    W.off = {n: REC.fields[n][1] for n in REC.names}
    W.gone = sorted(set(W.hot[::7].tolist()) | set(range(11, n_docs, 89)))
    W.sh = S.Shard(0, shard_id=shard_id)
    W.sh.upload_lexical(n_docs, dl, d_offs, d_docs, d_tfs)
    assert W.sh.append_sparse(s_offs, s_docs, s_tfs) == ND
    W.sh.upload_facets(np.ascontiguousarray(W.v.view(np.uint8).reshape(n_docs, REC.itemsize)))
    W.sh.set_deleted(W.gone)
    W.dist = O.geo_distances(W.v["loc"], BASE, UNIT)
    return W


@pytest.fixture(scope="module")
def W(S, O):
    assert N_DOCS % 64 != 0
    W = _world(S, O)
    yield W
    W.sh.close()


# ------------------------------------------------------------------------------------------------ queries, filter, facets
OR, AND = "or", "and"


def _query_mix():
    """70 queries: unions and intersections of 1-8 terms over both tiers, NOT terms, rare terms, one without a match, one matching
    nearly everything, one confined to one 64-doc group"""
    rng = np.random.default_rng(9)
    qs = [(OR, [0], []), (AND, [ND + 0, ONE_GROUP], []), (OR, [ONE_GROUP], []), (OR, [11], []), (AND, [0, 1], []), (OR, [0, 1, 2, 3, 4, 5, 6, 7], []),
          (AND, [0, 1, 2, 3], [4]), (OR, [ND + 3, ND + 4], [0]), (AND, [1, ND + 4], []), (OR, [10, 11, ND + 5], [])]
    n_terms_all = ONE_GROUP + 1
    while len(qs) < 70:
        n = int(rng.integers(1, 9))
        op = OR if rng.random() < 0.6 else AND
        pool = rng.permutation(n_terms_all)
        if op == AND:  # intersections of frequent terms (and at most one rarer one), so that most of them match something
            pool = np.concatenate([rng.permutation(5), rng.permutation(np.arange(5, n_terms_all))[:1]]) if n > 1 else pool
            n = min(n, 4)
        terms = [int(t) for t in pool[:n]]
        rest = [int(t) for t in pool[n:]]
        neg = rest[:int(rng.integers(0, 3))] if rng.random() < 0.4 else []
        qs.append((op, terms, neg))
    return qs


QUERIES = _query_mix()
FILTER_LO, FILTER_HI = 10_000, 52_000  # on u16: keeps ~64 % of the docs


def _filter(W):
    keep = (W.v["u16"] >= FILTER_LO) & (W.v["u16"] < FILTER_HI)
    return [(W.off["u16"], "u16", FILTER_LO, FILTER_HI)], keep


def _ranges(bounds):
    return [("r%d" % i, b) for i, b in enumerate(bounds)]


def _facets(W):
    """numeric, f32 with +-0.0 and NaN around a 0.0 bound, Point, String16, String32 beyond the LDS budget, a second numeric"""
    return [
        {"field": "i32", "offset": W.off["i32"], "type": "i32", "ranges": _ranges([-(1 << 31), -1_000_000_000, -5, 0, 7, 1_500_000_000]), "range_type": "within"},
        {"field": "f32", "offset": W.off["f32"], "type": "f32", "ranges": _ranges([-np.inf, -50.0, -1.0, 0.0, 1.0, 25.0, np.inf]), "range_type": "within"},
        {"field": "loc", "offset": W.off["loc"], "type": "point", "ranges": _ranges([0.0, 500.0, 1000.0, 2000.0, 3000.0]), "range_type": "within",
         "base": BASE, "unit": UNIT},
        {"field": "s16", "offset": W.off["s16"], "type": "string16", "values": ["a%d" % i for i in range(S16_BUCKETS)], "prefix": "", "length": 10},
        {"field": "s32", "offset": W.off["s32"], "type": "string32", "values": ["b%d" % i for i in range(S32_BUCKETS)], "prefix": "", "length": 10},
        {"field": "u64", "offset": W.off["u64"], "type": "u64", "ranges": _ranges([1 << 20, 1 << 62, 1 << 63, (1 << 64) - 5]), "range_type": "within"},
    ]


def _other_facets(W):
    """the remaining types, and the column every doc holds one value of"""
    return [
        {"field": "u8", "offset": W.off["u8"], "type": "u8", "ranges": _ranges([1, 50, 200, 255]), "range_type": "within"},
        {"field": "u16", "offset": W.off["u16"], "type": "u16", "ranges": _ranges([0, 20_000, 65_535]), "range_type": "within"},
        {"field": "u32", "offset": W.off["u32"], "type": "u32", "ranges": _ranges([5, 1 << 31, (1 << 32) - 1000]), "range_type": "within"},
        {"field": "i8", "offset": W.off["i8"], "type": "i8", "ranges": _ranges([-128, -1, 0, 100]), "range_type": "within"},
        {"field": "i16", "offset": W.off["i16"], "type": "i16", "ranges": _ranges([-30_000, -1, 1, 32_767]), "range_type": "within"},
        {"field": "i64", "offset": W.off["i64"], "type": "i64", "ranges": _ranges([-(1 << 62), -1, 0, 1 << 62]), "range_type": "within"},
        {"field": "f64", "offset": W.off["f64"], "type": "f64", "ranges": _ranges([-1e6, -0.0, 1e-300, 1e6]), "range_type": "within"},
        {"field": "same", "offset": W.off["same"], "type": "u32", "ranges": _ranges([0, 77, 78]), "range_type": "within"},
    ]


def _buckets(W, qf, docs):
    """the bucket of every doc of `docs` for one facet -- the rule, in numpy; n_buckets = "other" """
    if qf["type"].startswith("string"):
        nb = len(qf["values"])
        ids = W.v[qf["field"]][docs].astype(np.int64)
        return np.where(ids < nb, ids, nb).astype(np.int64), nb
    bounds = [b for _, b in qf["ranges"]]
    nb = len(bounds)
    if qf["type"] == "point":
        x, bs = W.dist[docs], np.asarray(bounds, np.float64)
    elif qf["type"] in ("f32", "f64"):
        dt = np.float32 if qf["type"] == "f32" else np.float64
        x, bs = W.v[qf["field"]][docs].astype(dt), np.asarray(bounds, dt)
    else:  # integers: compared in the column's own type, exactly
        dt = W.v[qf["field"]].dtype
        x, bs = W.v[qf["field"]][docs], np.array(bounds, dtype=dt)
        b = np.searchsorted(bs, x, side="right").astype(np.int64) - 1
        return np.where(b < 0, nb, b), nb
    b = np.searchsorted(bs, x, side="right") - 1  # (-0.0 == +0.0 for searchsorted as for the rule)
    b = np.where(np.isnan(x), -1, b).astype(np.int64)
    return np.where(b < 0, nb, b), nb


def _want_counts(W, qf, docs):
    b, nb = _buckets(W, qf, docs)
    return np.bincount(b, minlength=nb + 1).astype(np.uint64)


def _oracle(W, O, q, keep, k):
    """(docs, scores, total) of the first k and ALL matching docs, under tombstones and the filter"""
    op, terms, neg = q
    dead = set(W.gone) if keep is None else set(W.gone) | set(np.nonzero(~keep)[0].tolist())
    W.osh.set_deleted(sorted(dead))
    md, ms, tot = W.osh.search_exhaustive(terms, O.OP_OR if op == OR else O.OP_AND, W.n_docs, neg)
    assert len(md) == tot
    return md.astype(np.int64), ms, tot


def _make(S, W, qs):
    return W.sh.make_queries([t for _, t, _ in qs], [S.QueryType.Union if op == OR else S.QueryType.Intersection for op, _, _ in qs],
                             [n for _, _, n in qs])


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("k", [10, 1500])
def test_batch_against_brute_force(S, O, W, k):
    """70 queries x 6 facets in ONE call under a facet filter, TopkCount: counters, totals and hits against numpy over the oracle's match
    sets; then the same outputs against the library's own one-query-one-facet entries"""
    flt, keep = _filter(W)
    qfs = _facets(W)
    q = _make(S, W, QUERIES)
    doc, score, cnt, tot, per = W.sh.search_lexical_facets(q, k, qfs, S.ResultType.TopkCount, facet_filter=flt, reference_shortcuts=False)
    sizes = []
    for i, qq in enumerate(QUERIES):
        md, ms, otot = _oracle(W, O, qq, keep, k)
        sizes.append(otot)
        _check(doc[i], score[i], cnt[i], tot[i], md, ms, otot, S.ResultType.TopkCount, k, S, (k, qq))
        for f, qf in enumerate(qfs):
            want = _want_counts(W, qf, md)
            assert np.array_equal(per[f][i], want), (k, qq, qf["field"], np.nonzero(per[f][i] != want)[0][:8])
            assert int(per[f][i].sum()) == int(tot[i]) == otot
    assert sizes[1] == 0 and sizes[0] > 0.55 * N_DOCS and 0 < sizes[2] <= 5 and sum(1 for s in sizes if s > 1500) > 20  # the mix is what it says
    # consistency inside the library (a second assertion, not the reference)
    d2, s2, c2, t2 = W.sh.search_lexical_batch(q, k, S.ResultType.TopkCount, reference_shortcuts=False, facet_filter=flt)
    assert np.array_equal(doc, d2) and np.array_equal(score.view(np.uint32), s2.view(np.uint32)) and np.array_equal(cnt, c2) and np.array_equal(tot, t2)
    if k == 10:
        for i in range(len(QUERIES)):
            for f, qf in enumerate(qfs):
                if qf["type"].startswith("string"):
                    counts, other, total = W.sh.facet_count(q[i:i + 1], qf["offset"], qf["type"], n_buckets=len(qf["values"]), facet_filter=flt)
                else:
                    counts, other, total = W.sh.facet_count(q[i:i + 1], qf["offset"], qf["type"], range_lower_bounds=[b for _, b in qf["ranges"]],
                                                            facet_filter=flt, base=qf.get("base"), unit=qf.get("unit", "km"))
                assert np.array_equal(per[f][i][:-1], counts) and int(per[f][i][-1]) == other and total == int(tot[i]), (i, qf["field"])


def test_every_type_and_one_value_everywhere(S, O, W):
    """the other seven types, and a facet where every matched doc holds the same value (every add of a launch goes to one bucket); no
    facet filter; a near-everything query, the one-group query, the empty one"""
    qfs = _other_facets(W)
    qs = QUERIES[:12]
    q = _make(S, W, qs)
    doc, score, cnt, tot, per = W.sh.search_lexical_facets(q, 10, qfs, S.ResultType.TopkCount, reference_shortcuts=False)
    for i, qq in enumerate(qs):
        md, ms, otot = _oracle(W, O, qq, None, 10)
        _check(doc[i], score[i], cnt[i], tot[i], md, ms, otot, S.ResultType.TopkCount, 10, S, qq)
        for f, qf in enumerate(qfs):
            assert np.array_equal(per[f][i], _want_counts(W, qf, md)), (qq, qf["field"])
        assert per[-1][i].tolist() == [0, otot, 0, 0]  # `same`: all in one bucket
    d2, s2, c2, t2 = W.sh.search_lexical_batch(q, 10, S.ResultType.TopkCount, reference_shortcuts=False)
    assert np.array_equal(doc, d2) and np.array_equal(score.view(np.uint32), s2.view(np.uint32)) and np.array_equal(cnt, c2) and np.array_equal(tot, t2)


def test_a_single_query_with_a_single_facet(S, O, W):
    for qq in (QUERIES[0], QUERIES[2], QUERIES[1], QUERIES[7]):  # nearly everything; one 64-doc group; no match; sparse - dense
        for qf in [_facets(W)[j] for j in (0, 2, 3, 4)]:
            q = _make(S, W, [qq])
            doc, score, cnt, tot, per = W.sh.search_lexical_facets(q, 10, [qf], S.ResultType.TopkCount, reference_shortcuts=False)
            md, ms, otot = _oracle(W, O, qq, None, 10)
            _check(doc[0], score[0], cnt[0], tot[0], md, ms, otot, S.ResultType.TopkCount, 10, S, qq)
            assert np.array_equal(per[0][0], _want_counts(W, qf, md)), (qq, qf["field"])


def _raw_call(S, W, q, k, rt, n_facets, off, ty, nb, bounds, bases, doc_out=True, counts_words=None, flt=None):
    from seekstorm_amd import _native as N
    nq = len(q)
    kk = max(k, 1)
    doc, score = np.full((nq, kk), N.SS_NO_DOC, np.uint32), np.zeros((nq, kk), np.float32)
    cnt, tot = np.zeros(nq, np.uint32), np.zeros(nq, np.uint64)
    words = counts_words if counts_words is not None else int(sum(int(x) + 1 for x in (nb or [])))
    out = np.zeros((nq, max(words, 1)), np.uint64)
    a = lambda x, dt: None if x is None else np.asarray(x, dt)
    off_, ty_, nb_, bounds_ = a(off, np.uint32), a(ty, np.uint32), a(nb, np.uint32), a(bounds, np.uint64)
    farr, nf = W.sh.facet_filters(flt) if flt else (None, 0)
    rc = N.lib().ss_bm25_search_facets(W.sh._h, nq, q.ctypes.data_as(C.c_void_p), k, int(rt), nf, None if farr is None else C.cast(farr, C.c_void_p),
                                       n_facets, N.ptr(off_, N.u32p), N.ptr(ty_, N.u32p), N.ptr(nb_, N.u32p), N.ptr(bounds_, N.u64p),
                                       None if bases is None else C.cast(bases, C.c_void_p), N.ptr(doc, N.u32p) if doc_out else None,
                                       N.ptr(score, N.f32p) if doc_out else None, N.ptr(cnt, N.u32p), N.ptr(tot, N.u64p), N.ptr(out, N.u64p))
    return rc, doc, score, cnt, tot, out


def test_no_facets_is_the_filtered_search(S, O, W):
    flt, keep = _filter(W)
    q = _make(S, W, QUERIES[:20])
    rc, doc, score, cnt, tot, _ = _raw_call(S, W, q, 10, S.ResultType.TopkCount, 0, None, None, None, None, None, flt=flt)
    assert rc == 0
    for i, qq in enumerate(QUERIES[:20]):
        md, ms, otot = _oracle(W, O, qq, keep, 10)
        _check(doc[i], score[i], cnt[i], tot[i], md, ms, otot, S.ResultType.TopkCount, 10, S, qq)
    d2, s2, c2, t2 = W.sh.search_lexical_batch(q, 10, S.ResultType.TopkCount, reference_shortcuts=False, facet_filter=flt)
    assert np.array_equal(doc, d2) and np.array_equal(score.view(np.uint32), s2.view(np.uint32)) and np.array_equal(cnt, c2) and np.array_equal(tot, t2)


def test_count_with_null_doc_outputs(S, O, W):
    qfs = _facets(W)[:2]
    q = _make(S, W, QUERIES[:16])
    bounds = np.concatenate([W.sh._facet_bounds(qf) for qf in qfs])
    rc, _, _, cnt, tot, out = _raw_call(S, W, q, 0, S.ResultType.Count, 2, [qf["offset"] for qf in qfs], [TYPE_CODE[qf["type"]] for qf in qfs],
                                        [len(qf["ranges"]) for qf in qfs], bounds, None, doc_out=False)
    assert rc == 0
    for i, qq in enumerate(QUERIES[:16]):
        md, _, otot = _oracle(W, O, qq, None, 1)
        assert int(tot[i]) == otot
        want = np.concatenate([_want_counts(W, qf, md) for qf in qfs])
        assert np.array_equal(out[i], want), qq


def _err(S, W, **kw):
    from seekstorm_amd import _native as N
    qf = _facets(W)[0]
    args = dict(q=_make(S, W, [QUERIES[4]]), k=10, rt=S.ResultType.TopkCount, n_facets=1, off=[qf["offset"]], ty=[TYPE_CODE["i32"]],
                nb=[len(qf["ranges"])], bounds=W.sh._facet_bounds(qf), bases=None)
    args.update(kw)
    return _raw_call(S, W, **args)[0], N


def test_einval(S, W):
    """a type beyond SS_FACET_POINT, a Point facet without bases, missing bounds, more than SS_MAX_QUERY_FACETS facets, no buckets"""
    rc, N = _err(S, W, ty=[13])
    assert rc == N.SS_EINVAL
    assert _err(S, W, ty=[12], off=[W.off["loc"]])[0] == N.SS_EINVAL
    assert _err(S, W, bounds=None)[0] == N.SS_EINVAL
    n = N.SS_MAX_QUERY_FACETS + 1
    qf = _facets(W)[0]
    assert _err(S, W, n_facets=n, off=[qf["offset"]] * n, ty=[TYPE_CODE["i32"]] * n, nb=[2] * n, bounds=[0, 1] * n)[0] == N.SS_EINVAL
    assert _err(S, W, nb=[0])[0] == N.SS_EINVAL
    assert _err(S, W)[0] == N.SS_OK  # (the arguments the cases above vary are valid)
    # a sparse-tier term id is a valid term id
    assert _err(S, W, q=_make(S, W, [(OR, [ND + 2], [])]))[0] == N.SS_OK


def test_estate(S, O, W):
    """an offset beyond the record; a shard without facet records"""
    rc, N = _err(S, W, off=[REC.itemsize - 3])
    assert rc == N.SS_ESTATE
    bare = S.Shard(0)
    try:
        dl, d_offs, d_docs, d_tfs = _corpus(O, 8192, 3)[:4]  # (the corpus draws 5000 hot docs: more docs than that)
        bare.upload_lexical(8192, dl, d_offs, d_docs, d_tfs)
        W2 = World()
        W2.sh = bare
        qf = _facets(W)[0]
        assert _raw_call(S, W2, bare.make_queries([[1, 2]], S.QueryType.Union), 10, S.ResultType.TopkCount, 1, [qf["offset"]], [TYPE_CODE["i32"]],
                         [len(qf["ranges"])], W.sh._facet_bounds(qf), None)[0] == N.SS_ESTATE
    finally:
        bare.close()


def test_enotsup_for_a_batch_holding_a_phrase(S, W):
    """a phrase among the batch's queries: the whole call is left to the caller, as ss_bm25_facet_count leaves a phrase"""
    from seekstorm_amd import _native as N
    q = _make(S, W, QUERIES[:3])
    ph = W.sh.make_queries([[1, 2]], S.QueryType.Phrase)
    assert (int(ph["op"][0]) & 0xFF) == N.OP_PHRASE
    batch = np.concatenate([q, ph])
    assert _err(S, W, q=batch)[0] == N.SS_ENOTSUP
    with pytest.raises(N.SeekStormHipError) as e:
        W.sh.facet_count(ph, W.off["i32"], "i32", range_lower_bounds=[0])
    assert e.value.code == N.SS_ENOTSUP  # (the single-facet entry's own answer to the same query)


# ------------------------------------------------------------------------------------------------ two shards, both mirrors
def _index_facets(W0):
    sets = [["s%d" % (i % 5), "t%d" % (i % 3)] if i % 4 else ["s0"] for i in range(S16_BUCKETS)]
    return [
        {"field": "i32", "offset": W0.off["i32"], "type": "i32", "ranges": _ranges([-(1 << 31), -5, 0, 7, 1_500_000_000]), "range_type": "above"},
        {"field": "loc", "offset": W0.off["loc"], "type": "point", "ranges": _ranges([0.0, 500.0, 1000.0, 2000.0]), "range_type": "below", "base": BASE,
         "unit": UNIT},
        {"field": "s16", "offset": W0.off["s16"], "type": "string16", "values": ["a%d" % i for i in range(S16_BUCKETS)], "prefix": "a1", "length": 7},
        {"field": "s32", "offset": W0.off["s32"], "type": "string32", "values": ["b%d" % i for i in range(S32_BUCKETS)], "prefix": "", "length": 12},
        {"field": "tags", "offset": W0.off["s16"], "type": "stringset16", "values": sets, "prefix": "", "length": 4},
        {"field": "f32", "offset": W0.off["f32"], "type": "f32", "ranges": _ranges([-50.0, 0.0, 25.0]), "range_type": "within"},
    ]


def _cpp_index_search(shards, terms, qt, offset, length, rt, flt_arr, n_flt, qfs):
    u32p = C.POINTER(C.c_uint32)
    H = host_lib()
    H.ssh_index_adopt.restype = C.c_void_p
    H.ssh_index_adopt.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    H.ssh_index_destroy.argtypes = [C.c_void_p]
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
        n = H.ssh_index_search_facets(ix, t.ctypes.data_as(u32p), len(t), int(qt), offset, length, int(rt), n_flt,
                                      None if flt_arr is None else C.cast(flt_arr, C.c_void_p), _spec(qfs), cap, doc.ctypes.data, score.ctypes.data,
                                      meta.ctypes.data, buf, len(buf), C.byref(flen))
        assert n >= 0 and flen.value >= 0 and int(meta[3]) == 0, (n, flen.value, meta)
        return doc[:n], score[:n], int(meta[1]), parse_facets_text(buf.value.decode())
    finally:
        H.ssh_index_destroy(ix)


def test_two_shard_index_search_with_query_facets(S, O, W):
    """Index.search(query_facets=...) over two shards, Python and C++ mirror: ResultObject.facets against the brute-force maps over the whole
    corpus (every shard's raw histogram from numpy, finished and merged by the restated crate code), with the tie rule; hits and totals too"""
    n1 = 60_007
    W1 = _world(S, O, n_docs=n1, seed=57, shard_id=1)
    W1.dist = O.geo_distances(W1.v["loc"], BASE, UNIT)
    Ws = [W, W1]
    try:
        ix = S.Index([W.sh, W1.sh])
        qfs = _index_facets(W)
        flt, _ = _filter(W)
        farr, nflt = W.sh.facet_filters(flt)
        for op, terms, neg in [(OR, [3, 5, ND + 3], []), (AND, [0, 2], []), (OR, [ONE_GROUP], []), (AND, [ND + 0, ONE_GROUP], [])]:
            qt = S.QueryType.Union if op == OR else S.QueryType.Intersection
            shard_lists, total, merged = [], 0, []
            for sid, Wi in enumerate(Ws):
                keep = (Wi.v["u16"] >= FILTER_LO) & (Wi.v["u16"] < FILTER_HI)
                md, ms, otot = _oracle(Wi, O, (op, terms, neg), keep, 10)
                total += otot
                merged += [(-float(s), int(d) * 2 + sid) for d, s in zip(md[:10], ms[:10])]
                m = {}
                for qf in qfs:
                    col = dict(qf, field="s16") if qf["field"] == "tags" else qf
                    ref = ref_shard_map(qf, _want_counts(Wi, col, md), 2)
                    if ref is not None and ref[0]:
                        m[qf["field"]] = ref[0]
                shard_lists.append(m)
            want = ref_planner(qfs, shard_lists, S.ResultType.TopkCount)
            ro = ix.search(terms, None, qt, S.SearchMode.Lexical, 0, 10, S.ResultType.TopkCount, strict=True, not_terms=neg, facet_filter=flt,
                           query_facets=qfs)
            cd, cs, ctot, cfac = _cpp_index_search([W.sh, W1.sh], terms, qt, 0, 10, S.ResultType.TopkCount, farr, nflt, qfs) if not neg else (None,) * 4
            for who, facets, tot_ in (("python", ro.facets, ro.result_count_total),) + ((("c++", cfac, ctot),) if cfac is not None else ()):
                assert tot_ == total, (who, terms)
                assert set(facets) == set(want), (who, terms, set(facets) ^ set(want))
                for field, (full, cut) in want.items():
                    same_facet([(a, int(c)) for a, c in facets[field]], full, cut, (who, terms, field))
            merged.sort()
            ws = np.array([-s for s, _ in merged[:10]], np.float32)
            assert np.allclose([r.score for r in ro.results], ws, rtol=1e-4, atol=1e-7)
            if cd is not None:
                assert np.allclose(cs, ws, rtol=1e-4, atol=1e-7)
            topk = ix.search(terms, None, qt, S.SearchMode.Lexical, 0, 10, S.ResultType.Topk, strict=True, not_terms=neg, facet_filter=flt, query_facets=qfs)
            assert topk.facets == {}  # search.rs:1748
    finally:
        W1.sh.close()
