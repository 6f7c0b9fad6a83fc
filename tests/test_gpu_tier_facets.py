"""Facet counts, sort pivots and result sorts of queries that name SPARSE-tier terms (csrc/bm25_match.hip; -m gpu).

One world: the tiered shard of test_gpu_sparse_tier.py (5 dense lists + 9 sparse lists of 2 .. 3000 postings that overlap each other and
the dense ones) over 150 003 docs -- the last 64-doc word of every bitmap is partial --, tombstones that hit sparse postings, and the
packed facet record of test_gpu_facet_edges.py with its u8, i8, i16, i32, f32 (+-0), u64 and string16 columns filled from
oracle/naive.py's palettes.  The oracle holds all 14 lists as ordinary lists; every answer is checked against oracle/naive.py's facet
reference over the oracle's match set and scores, by the rules of test_gpu_facet_edges.py (scores within test_gpu_parity.REL)."""
import numpy as np
import pytest

from oracle import naive
from test_gpu_facet_edges import COL_TYPE, REC, World, _filter, _reference_order, _spec, _tie_ks, check_sorted, value_of
from test_gpu_parity import _fields_corpus
from test_gpu_sparse_tier import _tiered_shard

pytestmark = pytest.mark.gpu

N_DOCS = 150_003
COLS = ["u8", "i8", "i16", "i32", "f32", "u64"]
N_BUCKETS = 24  # string ids at or above it are counted as "other"
ND, NS = 5, 9   # dense lists 0..4, sparse lists 5..13 with [2, 50, 400, 1500, 3000, 9, 65, 2200, 700] postings
OR, AND = "or", "and"
# (name, op, terms, NOT terms): unions and intersections of 1-4 terms mixing tiers, all-sparse, dense NOT + sparse NOT, scored terms
# dense with a sparse NOT
TIERED = [
    ("one sparse term, 2 docs", OR, [5], []),
    ("one sparse term, 3000 docs", OR, [9], []),
    ("dense | sparse", OR, [1, 8], []),
    ("4 terms, both tiers", OR, [3, 9, 12, 0], []),
    ("all sparse", OR, [8, 9, 12], []),
    ("dense | sparse - dense - sparse", OR, [2, 7], [1, 12]),
    ("dense | dense - sparse", OR, [3, 2], [9]),
    ("dense - sparse - sparse", OR, [4], [9, 12]),
    ("dense & sparse", AND, [4, 9], []),
    ("sparse & sparse", AND, [9, 12], []),
    ("4 terms &, both tiers", AND, [4, 9, 12, 3], []),
    ("dense & sparse - dense - sparse", AND, [3, 8], [2, 12]),
    ("dense & dense - sparse", AND, [4, 3], [9]),
    ("no match", AND, [5, 10], []),
]
DENSE = [("dense |", OR, [1, 2], []), ("dense &", AND, [3, 4], []), ("dense | - dense", OR, [2, 0], [3]), ("one dense term", OR, [0], [])]
EMPTY, FEW, DEEP = "no match", "one sparse term, 2 docs", "4 terms, both tiers"
SORTS = [[("u8", True)], [("f32", False)], [("i32", True), ("f32", False)], [("u8", False), ("f32", True), ("u64", True), ("i32", False)]]


def _columns(W, n_docs, seed):
    """the facet record of test_gpu_facet_edges.py: every column of COLS from its type's palette (one value, or +-0, holds 30 % of the
    docs: large tie groups), string16 ids beyond N_BUCKETS"""
    rng = np.random.default_rng(seed)
    W.vals, W.idx = {}, {}
    rec = np.zeros(n_docs, REC)
    for col in COLS:
        ty = COL_TYPE[col]
        pal = naive.facet_palette(ty)
        p = np.full(len(pal), 0.7 / (len(pal) - 1))
        if ty[0] == "f":
            z = [i for i, x in enumerate(pal) if x == 0.0]
            p[:] = 0.7 / (len(pal) - 2)
            p[z] = 0.15
        else:
            p[len(pal) // 2] = 0.3
        W.vals[col] = pal
        W.idx[col] = rng.choice(len(pal), n_docs, p=p / p.sum())
        ub = np.array([naive.facet_bits(x, ty) for x in pal], np.uint64)
        rec[col] = ub[W.idx[col]].astype("<u%d" % REC[col].itemsize).view(REC[col])
    W.vals["s16"] = list(range(N_BUCKETS + 8)) + [65535]
    W.idx["s16"] = rng.integers(0, len(W.vals["s16"]), n_docs)
    rec["s16"] = np.array(W.vals["s16"], np.uint64)[W.idx["s16"]].astype(REC["s16"])
    W.rec = rec
    W.off = {n: REC.fields[n][1] for n in REC.names}
    return np.ascontiguousarray(rec.view(np.uint8).reshape(n_docs, REC.itemsize))


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _oracle_world(O):
    """everything of the world that needs no device: the corpus as _tiered_shard draws it with the oracle shard over all 14 lists, the
    facet columns, the tombstones -- and the proof that the cases are not vacuous"""
    W = World()
    W.raw = _columns(W, N_DOCS, 2027)
    W.cases = {c[0]: c for c in TIERED + DENSE}
    dl, d_offs, d_docs, d_tfs, s_offs, s_docs, s_tfs, W.hot = _tiered_corpus(O, N_DOCS, 21)
    W.osh = O.Shard(N_DOCS, dl, np.concatenate([d_offs, d_offs[-1] + s_offs[1:]]), np.concatenate([d_docs, s_docs]), np.concatenate([d_tfs, s_tfs]))
    W.gone = sorted(set(W.hot[::5].tolist()) | set(range(13, N_DOCS, 997)))  # every fifth doc of the sparse lists' pool, and others
    W.cache = {}
    W.dead = None
    _not_vacuous(W, O)
    return W


def _matches(W, O, name, dead):
    key = (name, dead)
    if key not in W.cache:
        _, op, terms, neg = W.cases[name]
        W.osh.set_deleted(W.gone if dead else [])
        md, ms, tot = W.osh.search_exhaustive(terms, O.OP_OR if op == OR else O.OP_AND, N_DOCS, neg)
        assert len(md) == tot
        W.cache[key] = (md.astype(np.int64), ms)
    return W.cache[key]


@pytest.fixture(scope="module")
def W(S, O):
    W = _oracle_world(O)  # on the oracle alone, before any call on the device
    W.sh, osh, nd, ns, hot, n_docs = _tiered_shard(S, O, n_docs=N_DOCS)
    assert (nd, ns, n_docs) == (ND, NS, N_DOCS) and N_DOCS % 64 != 0 and np.array_equal(hot, W.hot)  # the same draw
    W.sh.upload_facets(W.raw)
    yield W
    W.sh.close()


def _not_vacuous(W, O):
    """the world holds what the cases are about: every tiered case (but the empty one) answers differently from the same query without
    its sparse terms, by at least one doc; tombstones hit sparse postings; one case has fewer matches than k = 10, one none; a sort's
    first field has a tie group straddling some k"""
    for dead in (False, True):
        for name, op, terms, neg in TIERED:
            md = _matches(W, O, name, dead)[0]
            if name == EMPTY:
                assert len(md) == 0
                continue
            dterms, dneg = [t for t in terms if t < ND], [t for t in neg if t < ND]
            W.osh.set_deleted(W.gone if dead else [])
            if not dterms:
                only_sparse = set(md.tolist())  # no dense scored term: every match is a sparse list's
            else:
                dd = W.osh.search_exhaustive(dterms, O.OP_OR if op == OR else O.OP_AND, N_DOCS, dneg)[0]
                only_sparse = set(md.tolist()) ^ set(dd.tolist())
            assert only_sparse, name
        assert 0 < len(_matches(W, O, FEW, dead)[0]) < 10
        assert len(_matches(W, O, DEEP, dead)[0]) > 1500
    for name, _, terms, _ in TIERED:
        if name != EMPTY and any(t >= ND for t in terms):  # tombstones take docs of the sparse lists away
            assert len(_matches(W, O, name, True)[0]) < len(_matches(W, O, name, False)[0]) or name == FEW, name
    ref = _reference_order(W, *_matches(W, O, "dense | sparse", True), SORTS[0])
    first = value_of(W, "u8", ref[0][:1100])
    assert any(first[k - 1] == first[k] and first[0] != first[k] for k in _tie_ks(W, ref, SORTS[0]) if k < len(first))


def _state(W, dead):
    if W.dead != dead:
        W.sh.set_deleted(W.gone if dead else [])
        W.dead = dead


def _query(S, W, name):
    _, op, terms, neg = W.cases[name]
    return W.sh.make_queries([terms], S.QueryType.Union if op == OR else S.QueryType.Intersection, [neg])


def _filters(S, W):
    flt = _filter(S, W, "i16", W.vals["i16"][1], W.vals["i16"][-2])
    return ((None, None), ([flt[0]], flt[1]))


@pytest.mark.parametrize("dead", [False, True])
def test_facet_counts_over_tiered_match_sets(S, O, W, dead):
    """ss_bm25_facet_count: numeric bounds (u8, i32, f32 with a 0.0 bound against stored -0.0, u64) and string16 ids -- every bucket,
    "other" and the total equal the reference's, with and without a facet filter"""
    _state(W, dead)
    bounds_of = {}
    for col in ("u8", "i32", "f32", "u64"):
        pal = [x for x in W.vals[col] if not (isinstance(x, float) and x == 0.0 and np.copysign(1.0, x) < 0)]
        bounds_of[col] = [pal[1::3], [pal[len(pal) // 2]]]
    bounds_of["f32"].append([-1.0, 0.0, 1.0])
    for name, _, terms, neg in TIERED:
        q = _query(S, W, name)
        md = _matches(W, O, name, dead)[0]
        for flt, keep in _filters(S, W):
            m = md if keep is None else md[keep[md]]
            for col, bl in bounds_of.items():
                for bounds in bl:
                    counts, other, tot = W.sh.facet_count(q, W.off[col], COL_TYPE[col], range_lower_bounds=bounds, facet_filter=flt)
                    b = [naive.facet_bucket(x, bounds) for x in W.vals[col]]
                    want = np.zeros(len(bounds) + 1, np.int64)
                    np.add.at(want, [len(bounds) if x is None else x for x in np.array(b, object)[W.idx[col][m]]], 1)
                    assert tot == len(m), (name, col, flt is None, tot, len(m))
                    assert np.array_equal(counts, want[:-1]) and other == want[-1], (name, col, bounds, flt is None)
            counts, other, tot = W.sh.facet_count(q, W.off["s16"], "string16", n_buckets=N_BUCKETS, facet_filter=flt)
            ids = np.array(W.vals["s16"], np.int64)[W.idx["s16"][m]]
            want = np.bincount(np.minimum(ids, N_BUCKETS), minlength=N_BUCKETS + 1)
            assert tot == len(m) and np.array_equal(counts, want[:N_BUCKETS]) and other == want[N_BUCKETS], (name, "s16", flt is None)


@pytest.mark.parametrize("dead", [False, True])
def test_sort_pivot_over_tiered_match_sets(S, O, W, dead):
    """ss_bm25_facet_kth, both directions, k in {1, the first tie group's edge and the rank after it, matches, matches + 1}: value,
    n_better, n_equal and the total equal the reference's"""
    _state(W, dead)
    for name, _, terms, neg in TIERED:
        q = _query(S, W, name)
        md = _matches(W, O, name, dead)[0]
        for flt, keep in _filters(S, W):
            m = md if keep is None else md[keep[md]]
            for col in ("u8", "i32", "f32", "u64"):
                ty = COL_TYPE[col]
                vals = value_of(W, col, m)
                for desc in (True, False):
                    edge = naive.kth(vals, 1, desc)[2]
                    for k in sorted({1, max(edge, 1), edge + 1, max(len(m), 1), len(m) + 1}):
                        v, nb, ne = naive.kth(vals, k, desc)
                        bits, gb, ge, tot = W.sh.facet_kth(q, W.off[col], ty, desc, k, facet_filter=flt)
                        assert tot == len(m), (name, col, tot, len(m))
                        assert (gb, ge) == (nb, ne), (name, col, desc, k, flt is None, (gb, ge), (nb, ne))
                        if len(m):
                            assert naive.facet_value(bits, ty) == v, (name, col, desc, k, flt is None)


@pytest.mark.parametrize("dead", [False, True])
def test_result_sort_over_tiered_match_sets(S, O, W, dead):
    """ss_bm25_search_sorted with 1, 2 and 4 sort fields, k in {1, 10, tie-group edges, 1024}, one query at a time and in batches that
    mix all-dense and tiered queries; the composed route gives the same answer"""
    _state(W, dead)
    names = [c[0] for c in TIERED]
    mixed = [names[0], DENSE[0][0], names[3], names[5], DENSE[1][0], names[8], names[13], DENSE[2][0], names[11], names[6]]
    qb = np.concatenate([_query(S, W, n) for n in mixed])
    for flt, keep in _filters(S, W):
        for srt in SORTS:
            refs = {n: _reference_order(W, *_matches(W, O, n, dead), srt, keep) for n in names + [d[0] for d in DENSE]}
            for k in (1, 10, 1024):  # the mixed batch: every row against its own reference
                bd, bs, bc, bt = W.sh.search_lexical_sorted_batch(qb, _spec(W, srt), k, facet_filter=flt)
                for row, n in enumerate(mixed):
                    check_sorted(W, bd[row][:bc[row]], bs[row][:bc[row]], int(bt[row]), refs[n], srt, k, ("mixed", n, srt, k, flt is None))
                    assert np.all(bd[row][bc[row]:] == 0xFFFFFFFF)
            for n in names:  # one query per call: tie edges, and the composed route
                q = _query(S, W, n)
                ks = _tie_ks(W, refs[n], srt) if (flt is None or srt is SORTS[0]) else [10]
                for k in ks:
                    bd, bs, bc, bt = W.sh.search_lexical_sorted_batch(q, _spec(W, srt), k, facet_filter=flt)
                    check_sorted(W, bd[0][:bc[0]], bs[0][:bc[0]], int(bt[0]), refs[n], srt, k, ("batched", n, srt, k, flt is None))
                    if k in (1, 10, 1024) and srt is not SORTS[2]:
                        cd, cs, ct = W.sh.search_lexical_sorted_composed(q, _spec(W, srt), k, facet_filter=flt)
                        check_sorted(W, cd, cs, ct, refs[n], srt, k, ("composed", n, srt, k, flt is None))


def test_result_sort_batch_of_more_than_64_queries(S, O, W):
    """one call for 70 queries: two chunks, both holding tiered and all-dense queries"""
    _state(W, True)
    names = [c[0] for c in TIERED + DENSE]
    idx = [names[(7 * i) % len(names)] for i in range(70)]
    qb = np.concatenate([_query(S, W, n) for n in idx])
    for srt, k in ((SORTS[0], 25), (SORTS[2], 300)):
        bd, bs, bc, bt = W.sh.search_lexical_sorted_batch(qb, _spec(W, srt), k)
        refs = {}
        for row, n in enumerate(idx):
            if n not in refs:
                refs[n] = _reference_order(W, *_matches(W, O, n, True), srt)
            check_sorted(W, bd[row][:bc[row]], bs[row][:bc[row]], int(bt[row]), refs[n], srt, k, ("batch of 70", row, n, srt))


def test_deep_sorted_page_of_a_tiered_query(S, O, W):
    """k = 1500 > SS_MAX_K on a query with more matches than that: passes of the sorted search under the peel bitmap"""
    for dead in (False, True):
        _state(W, dead)
        for srt in (SORTS[1], SORTS[2]):
            ref = _reference_order(W, *_matches(W, O, DEEP, dead), srt)
            doc, score, tot = W.sh.search_lexical_sorted(_query(S, W, DEEP), _spec(W, srt), 1500)
            check_sorted(W, doc, score, tot, ref, srt, 1500, ("deep", srt, dead))


def test_index_of_two_tiered_shards_sorts(S, O, W):
    """Index.search with result_sort over two shards that both have a sparse tier: against the reference's order of the union of the
    shards' matches, each scored with its own shard's statistics"""
    n_each = 60_001
    W2 = World()
    raw = _columns(W2, 2 * n_each, 99)
    shards, oshards = [], []
    try:
        for sid in range(2):
            sh, osh = _tiered_pair(S, O, n_each, 40 + sid, sid)
            sh.upload_facets(np.ascontiguousarray(raw[sid::2]))
            shards.append(sh)
            oshards.append(osh)
        idx = S.Index(shards)
        for name in ("dense | sparse", "dense & sparse", "dense | dense - sparse", "all sparse"):
            _, op, terms, neg = W.cases[name]
            md, ms = [], []
            for sid, osh in enumerate(oshards):
                d, s_, _ = osh.search_exhaustive(terms, O.OP_OR if op == OR else O.OP_AND, n_each, neg)
                md.append(d.astype(np.int64) * 2 + sid)
                ms.append(s_)
            md, ms = np.concatenate(md), np.concatenate(ms)
            assert len(md) > 20
            for srt in (SORTS[0], SORTS[2]):
                ref = _reference_order(W2, md, ms, srt)
                for off_, length in ((0, 10), (5, 300)):
                    ro = idx.search(terms, None, S.QueryType.Union if op == OR else S.QueryType.Intersection, S.SearchMode.Lexical, off_, length,
                                    strict=True, not_terms=neg, result_sort=_spec(W2, srt))
                    sub = (ref[0][off_:], ref[1][off_:], ref[2], ref[3])
                    assert ro.result_count_total == len(md)
                    check_sorted(W2, [r.doc_id for r in ro.results], [r.score for r in ro.results], len(md), sub, srt,
                                 min(length, max(len(md) - off_, 0)), ("index", name, srt, off_, length))
    finally:
        for sh in shards:
            sh.close()


def _tiered_corpus(O, n_docs, seed):
    """the lists _tiered_shard draws, dense and sparse apart"""
    rng = np.random.default_rng(seed)
    dl = O.lex_doclen(n_docs)
    offs, docs, tfs = [0], [], []
    for df in (0.004, 0.02, 0.07, 0.15, 0.33):
        d = np.sort(rng.choice(n_docs, int(df * n_docs), replace=False)).astype(np.uint32)
        docs.append(d); tfs.append(np.minimum(rng.geometric(0.6, len(d)), 60).astype(np.uint16)); offs.append(offs[-1] + len(d))
    hot = np.sort(rng.choice(n_docs, 6000, replace=False))
    s_offs, s_docs, s_tfs = [0], [], []
    for n in [2, 50, 400, 1500, 3000, 9, 65, 2200, 700]:
        d = np.sort(rng.choice(hot, n, replace=False)).astype(np.uint32)
        s_docs.append(d); s_tfs.append(np.minimum(rng.geometric(0.5, n), 30).astype(np.uint16)); s_offs.append(s_offs[-1] + n)
    return (dl, np.asarray(offs, np.uint64), np.concatenate(docs), np.concatenate(tfs),
            np.asarray(s_offs, np.uint64), np.concatenate(s_docs), np.concatenate(s_tfs), hot)


def _tiered_pair(S, O, n_docs, seed, shard_id):
    """a tiered shard under its own shard id, and the oracle holding all of its lists as ordinary lists"""
    dl, d_offs, d_docs, d_tfs, s_offs, s_docs, s_tfs, _ = _tiered_corpus(O, n_docs, seed)
    sh = S.Shard(0, shard_id=shard_id)
    sh.upload_lexical(n_docs, dl, d_offs, d_docs, d_tfs)
    assert sh.append_sparse(s_offs, s_docs, s_tfs) == ND
    osh = O.Shard(n_docs, dl, np.concatenate([d_offs, d_offs[-1] + s_offs[1:]]), np.concatenate([d_docs, s_docs]), np.concatenate([d_tfs, s_tfs]))
    return sh, osh


def test_all_dense_queries_answer_as_on_the_dense_image(S, O, W):
    """the old path is intact: all-dense queries on the tiered shard give exactly what a shard holding only the dense image gives"""
    dl, d_offs, d_docs, d_tfs = _tiered_corpus(O, N_DOCS, 21)[:4]
    plain = S.Shard(0)
    try:
        plain.upload_lexical(N_DOCS, dl, d_offs, d_docs, d_tfs)
        plain.upload_facets(W.raw)
        flt = _filters(S, W)[1][0]
        for dead in (False, True):
            _state(W, dead)
            plain.set_deleted(W.gone if dead else [])
            for name, op, terms, neg in DENSE:
                qa, qb = _query(S, W, name), plain.make_queries([terms], S.QueryType.Union if op == OR else S.QueryType.Intersection, [neg])
                assert qa.tobytes() == qb.tobytes()
                for f in (None, flt):
                    a = W.sh.facet_count(qa, W.off["i32"], "i32", range_lower_bounds=W.vals["i32"][1::3], facet_filter=f)
                    b = plain.facet_count(qb, W.off["i32"], "i32", range_lower_bounds=W.vals["i32"][1::3], facet_filter=f)
                    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], name
                    for desc in (True, False):
                        assert W.sh.facet_kth(qa, W.off["f32"], "f32", desc, 7, facet_filter=f) == plain.facet_kth(qb, W.off["f32"], "f32", desc, 7, facet_filter=f)
                    for srt in SORTS:
                        for k in (10, 300):
                            x = W.sh.search_lexical_sorted_batch(qa, _spec(W, srt), k, facet_filter=f)
                            y = plain.search_lexical_sorted_batch(qb, _spec(W, srt), k, facet_filter=f)
                            for u, v in zip(x, y):
                                assert np.array_equal(u, v), (name, srt, k)
    finally:
        plain.close()


# What these entries leave to the caller's own path on a query naming a sparse term, one query each.  (The
# list's "several indexed fields without merged lists" cannot be built: such an image takes no sparse tier.)
NOT_ANSWERED = {"phrase", "all_terms_frequent", "union of several terms under a field filter", "a dense list without a probe row"}


def _code(call):
    from seekstorm_amd import _native as N
    try:
        call()
    except N.SeekStormHipError as e:
        return e.code
    return N.SS_OK


def _entries(sh, W, q):
    """facet count, sort pivot and result sort of one query (the Point variants share their implementations)"""
    return [lambda: sh.facet_count(q, W.off["i32"], "i32", range_lower_bounds=[0]), lambda: sh.facet_kth(q, W.off["i32"], "i32", True, 3),
            lambda: sh.search_lexical_sorted_batch(q, [(W.off["i32"], "i32", True)], 10)]


def test_what_stays_unanswered_is_not_supported_and_a_bad_term_is_invalid(S, O, W):
    from seekstorm_amd import _native as N
    got = {}
    _state(W, False)
    sh = W.sh
    got["phrase"] = [_code(c) for c in _entries(sh, W, sh.make_queries([[1, 8]], S.QueryType.Phrase))]
    q = sh.make_queries([[4, 9]], S.QueryType.Intersection)
    q["op"][0] |= np.uint32(1 << 31)  # SS_OP_ALL_TERMS_FREQUENT
    got["all_terms_frequent"] = [_code(c) for c in _entries(sh, W, q)]
    # several indexed fields, merged lists: a union of several terms under a field filter, the sparse term scored or excluded
    n_docs, dfs, nd = 20_003, [6_000, 2_000, 3_000, 900, 120, 40, 300], 3
    dl, offs, docs, fields, tfs = _fields_corpus(O, n_docs, 3, dfs, 12)
    e = int(offs[nd])
    W3 = World()
    raw = _columns(W3, n_docs, 5)
    m = S.Shard(0)
    try:
        m.upload_lexical_fields(n_docs, dl, [2.0, 1.0, 0.5], offs[:nd + 1], docs[:e], fields[:e], tfs[:e])
        assert m.fields_info()[1]
        assert m.append_sparse_fields(offs[nd:] - offs[nd], docs[e:], fields[e:], tfs[e:]) == nd
        m.upload_facets(raw)
        got["union of several terms under a field filter"] = (
            [_code(c) for c in _entries(m, W3, m.make_queries([[0, 4]], S.QueryType.Union, field_filter=(0,)))] +
            [_code(c) for c in _entries(m, W3, m.make_queries([[0, 1]], S.QueryType.Union, [[4]], field_filter=(0, 1)))])
    finally:
        m.close()
    # a probe budget of three rows, no pool: the two shortest dense lists have no bit records
    dl1, d_offs, d_docs, d_tfs, s_offs, s_docs, s_tfs, _ = _tiered_corpus(O, N_DOCS, 21)
    r = S.Shard(0)
    try:
        n_sub = (N_DOCS + 4095) // 4096
        r.set_probe_budget(4 * n_sub * 64 * 12)  # (a row: 64 groups per sub-block, 8 + 4 bytes each; one row is the all-zero row)
        r.upload_lexical(N_DOCS, dl1, d_offs, d_docs, d_tfs)
        assert r.append_sparse(s_offs, s_docs, s_tfs) == ND
        r.upload_facets(W.raw)
        got["a dense list without a probe row"] = ([_code(c) for c in _entries(r, W, r.make_queries([[1, 8]], S.QueryType.Union))] +
                                                   [_code(c) for c in _entries(r, W, r.make_queries([[9, 0]], S.QueryType.Intersection))])
        # ... while its lists with rows answer
        want = len(_matches(W, O, "dense & sparse", False)[0])
        assert r.facet_kth(r.make_queries([[4, 9]], S.QueryType.Intersection), W.off["i32"], "i32", True, 3)[3] == want
    finally:
        r.close()
    assert {k for k, v in got.items() if v and all(c == N.SS_ENOTSUP for c in v)} == NOT_ANSWERED, got
    # a term id at or beyond n_dense + sp_n is no term of the index
    for bad in (ND + NS, 0xFFFFFFF0):
        for terms, qt in (([1, 8], S.QueryType.Union), ([1, 2], S.QueryType.Intersection)):
            q = sh.make_queries([terms], qt)
            q["term"][0, 1] = bad
            assert [_code(c) for c in _entries(sh, W, q)] == [N.SS_EINVAL] * 3, (bad, terms)
    # and the valid ids just below it answer: never SS_EINVAL for a term of the index
    assert [_code(c) for c in _entries(sh, W, sh.make_queries([[ND + NS - 1]], S.QueryType.Union))] == [N.SS_OK] * 3


def test_tiered_image_with_several_indexed_fields(S, O):
    """merged lists + a sparse tier: an unfiltered union and field-filtered intersections / single terms (NOT terms of either tier),
    facet-counted, pivoted and sorted against the BM25F oracle over all entries"""
    n_docs, n_fields, boost = 50_003, 3, [2.0, 1.0, 0.5]
    dfs = [15_000, 4_500, 7_000, 2_000, 300, 50, 600, 5, 150, 1_250]
    nd = 4
    dl, offs, docs, fields, tfs = _fields_corpus(O, n_docs, n_fields, dfs, 12)
    e = int(offs[nd])
    W = World()
    raw = _columns(W, n_docs, 31)
    sh = S.Shard(0)
    try:
        sh.upload_lexical_fields(n_docs, dl, boost, offs[:nd + 1], docs[:e], fields[:e], tfs[:e])
        assert sh.fields_info()[1]
        assert sh.append_sparse_fields(offs[nd:] - offs[nd], docs[e:], fields[e:], tfs[e:]) == nd
        sh.upload_facets(raw)
        gone = list(range(3, n_docs, 97))
        cases = [(OR, [0, 4], [], None), (OR, [6, 1, 2], [3], None), (OR, [2, 1], [9], None), (AND, [0, 9], [], None),
                 (AND, [0, 4], [], (0,)), (AND, [6, 9], [], (1, 2)), (AND, [9, 1], [], (1, 2)), (AND, [9, 0, 6], [], (0, 1)), (AND, [6, 0], [9], (2,)),
                 (AND, [2, 1], [6], (0,)), (OR, [9], [0], (1, 2)), (AND, [4], [], (2,))]
        for deleted in ((), gone):
            sh.set_deleted(deleted)
            for op, terms, neg, filt in cases:
                q = sh.make_queries([terms], S.QueryType.Union if op == OR else S.QueryType.Intersection, [neg], field_filter=filt)
                md, ms, tot, _ = O.search_fields_exhaustive(n_docs, dl, boost, offs, docs, fields, tfs, terms, O.OP_OR if op == OR else O.OP_AND,
                                                            n_docs, neg, deleted, **({"field_filter": filt} if filt else {}))
                md = md.astype(np.int64)
                assert len(md) == tot and tot > 0, (terms, filt)
                what = (op, terms, neg, filt, bool(deleted))
                bounds = W.vals["i32"][1::3]
                counts, other, got = sh.facet_count(q, W.off["i32"], "i32", range_lower_bounds=bounds)
                b = [naive.facet_bucket(x, bounds) for x in W.vals["i32"]]
                want = np.zeros(len(bounds) + 1, np.int64)
                np.add.at(want, [len(bounds) if x is None else x for x in np.array(b, object)[W.idx["i32"][md]]], 1)
                assert got == tot and np.array_equal(counts, want[:-1]) and other == want[-1], what
                vals = value_of(W, "f32", md)
                for desc in (True, False):
                    v, nb, ne = naive.kth(vals, 5, desc)
                    bits, gb, ge, got = sh.facet_kth(q, W.off["f32"], "f32", desc, 5)
                    assert (gb, ge, got) == (nb, ne, tot) and naive.facet_value(bits, "f32") == v, what
                for srt in (SORTS[0], SORTS[2]):
                    ref = _reference_order(W, md, ms, srt)
                    for k in (10, 200):
                        bd, bs, bc, bt = sh.search_lexical_sorted_batch(q, _spec(W, srt), k)
                        check_sorted(W, bd[0][:bc[0]], bs[0][:bc[0]], int(bt[0]), ref, srt, k, ("fields",) + what)
    finally:
        sh.close()
