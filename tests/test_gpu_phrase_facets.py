"""Facet counts, sort pivots, result sorts and query_facets of PHRASE queries (csrc/bm25_phrase_bits.hip; -m gpu).

A phrase's match set is built as the match set of the intersection of its unique terms, refined by the position check.  Every world
below is small (20 003 docs: no multiple of 64 or 4096, five sub-blocks) and is first built on the oracle alone, where it has to show
that the refine has something to do: for at least three phrases 0 < |phrase set| < |intersection set|.

Expectations: the oracle's FULL phrase list (search_phrase / search_fields_phrase / search_phrase_items with k = n_docs), NOT lists,
tombstones and the facet filter applied in numpy; counters == numpy histograms by test_gpu_query_facets.py's bucket rule; pivots ==
oracle/naive.py's k-th value; sorted pages by test_gpu_facet_edges.py's check_sorted (keys position by position, scores within
test_gpu_parity.REL); the hits of search_lexical_facets bit-identical to search_lexical_batch under the same filter."""
import ctypes as C

import numpy as np
import pytest

from oracle import naive
from test_gpu_facet_edges import _reference_order, check_sorted
from test_gpu_phrase import _corpus, _corpus_fields
from test_gpu_query_facets import BASE, REC, S16_BUCKETS, UNIT, World, _cpp_index_search, _ranges, _records, _want_counts
from test_query_facets_host import host_lib, ref_planner, ref_shard_map, same_facet

pytestmark = pytest.mark.gpu

N_DOCS = 20_003
EDGE_DOCS = [0, N_DOCS - 1, 4095, 4096]
SORT_COLS = {"u8": "u8", "i8": "i8", "u16": "u16", "i32": "i32"}
SORTS = [[("u8", True)], [("i8", False), ("u16", True)]]
FILTER_LO, FILTER_HI = 10_000, 52_000  # on u16: keeps ~64 % of the docs
S16_IDS = list(range(0, 200))          # on s16 (ids 0 .. 299): keeps two thirds


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# ------------------------------------------------------------------------------------------------ worlds
def _plant_at(arrays, n_terms, plants):
    """the CSR arrays of test_gpu_phrase._corpus with phrases written into CHOSEN docs: plants = [(words, doc, start position)]"""
    dl, offs, docs, tfs, positions = arrays
    pos_of, at = [dict() for _ in range(n_terms)], 0
    for t in range(n_terms):
        for i in range(int(offs[t]), int(offs[t + 1])):
            pos_of[t][int(docs[i])] = set(positions[at:at + int(tfs[i])].tolist())
            at += int(tfs[i])
    for words, d, st in plants:
        for i, t in enumerate(words):
            pos_of[t].setdefault(int(d), set()).add(st + i)
    offs2, docs2, tfs2, pos2 = [0], [], [], []
    for t in range(n_terms):
        for d in sorted(pos_of[t]):
            ps = sorted(pos_of[t][d])
            docs2.append(d); tfs2.append(len(ps)); pos2 += ps
        offs2.append(len(docs2))
    return dl, np.asarray(offs2, np.uint64), np.asarray(docs2, np.uint32), np.asarray(tfs2, np.uint16), np.asarray(pos2, np.uint16)


def _facet_side(W, O, n_docs, seed):
    """the packed record of test_gpu_query_facets.py (one column of every type), and the sort columns in the vals / idx form that
    test_gpu_facet_edges.py's value_of / check_sorted read"""
    W.n_docs = n_docs
    W.v = _records(O, n_docs, seed)
    W.off = {n: REC.fields[n][1] for n in REC.names}
    W.dist = O.geo_distances(W.v["loc"], BASE, UNIT)
    W.sortkey = O.geo_distances(W.v["loc"], BASE, "sortkey")
    W.vals, W.idx = {}, {}
    for col in SORT_COLS:
        u, inv = np.unique(W.v[col], return_inverse=True)
        W.vals[col], W.idx[col] = [int(x) for x in u], inv.reshape(-1)
    W.raw = np.ascontiguousarray(W.v.view(np.uint8).reshape(n_docs, REC.itemsize))
    W.filters = {
        None: (None, None),
        "numeric": ([(W.off["u16"], "u16", FILTER_LO, FILTER_HI)], (W.v["u16"] >= FILTER_LO) & (W.v["u16"] < FILTER_HI)),
        "string": ([(W.off["s16"], "string16", S16_IDS)], np.isin(W.v["s16"], S16_IDS)),
    }
    W.qfs = [
        {"field": "i32", "offset": W.off["i32"], "type": "i32", "ranges": _ranges([-(1 << 31), -1_000_000_000, -5, 0, 7, 1_500_000_000]), "range_type": "within"},
        {"field": "s16", "offset": W.off["s16"], "type": "string16", "values": ["a%d" % i for i in range(S16_BUCKETS)], "prefix": "", "length": 10},
    ]
    W.point_bounds = [0.0, 500.0, 1000.0, 2000.0, 3000.0]


def _spec(W, srt):
    return [(W.off[c], SORT_COLS[c], d) for c, d in srt]


def _seq(ph):
    uniq = list(dict.fromkeys(ph))
    return uniq, [uniq.index(w) for w in ph]


DENSE_DFS = [6000, 4500, 8000, 2000, 3000, 1500, 2500, 150, 200]
LONG = [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 4]  # 12 words, 7 unique terms: beyond the staged phrase kernel's six
DENSE_PLANT = [([0, 1], 1500), ([0, 1, 2], 60), ([2, 0, 2], 50), ([1, 1], 40), ([3, 4], 30), ([0, 1, 2, 3, 4, 5], 20), (LONG, 15), ([7, 8], 25)]
# (phrase, NOT terms)
DENSE_CASES = [([0, 1], []), ([1, 0], []), ([0, 1, 2], []), ([2, 0, 2], []), ([1, 1], []), ([3, 4], []), ([0, 1, 2, 3, 4, 5], []), (LONG, []),
               ([7, 8], []), ([8, 7], []), ([0, 1], [2]), ([0, 1, 2], [3, 4])]
REFINED = [[0, 1], [0, 1, 2], [2, 0, 2], [3, 4]]  # the intersection of their words holds docs without the phrase


def _dense_world(O):
    """one indexed field, everything dense; phrases planted by the corpus builder and, on top, into docs 0, n - 1, 4095, 4096 and into a
    doc whose 64-doc group holds no other candidate of its phrase"""
    W = World()
    arrays = _corpus(O, N_DOCS, DENSE_DFS, 41, DENSE_PLANT)
    edge = [(ph, d, 300 + 20 * j) for d in EDGE_DOCS for j, ph in enumerate(([0, 1], [2, 0, 2], [7, 8], LONG))]
    arrays = _plant_at(arrays, len(DENSE_DFS), edge)
    # the lonely doc: a group without a doc of terms 7 and 8 together
    dl, offs, docs, tfs, positions = arrays
    both = np.intersect1d(docs[int(offs[7]):int(offs[8])], docs[int(offs[8]):int(offs[9])])
    free = sorted(set(range(100, N_DOCS // 64)) - set((both // 64).tolist()))
    W.lonely = free[len(free) // 2] * 64 + 37
    arrays = _plant_at(arrays, len(DENSE_DFS), [([7, 8], W.lonely, 500)])
    W.dl, W.offs, W.docs, W.tfs, W.positions = arrays
    W.lists = [W.docs[int(W.offs[t]):int(W.offs[t + 1])] for t in range(len(DENSE_DFS))]
    W.osh = O.Shard(N_DOCS, W.dl, W.offs, W.docs, W.tfs)
    W.osh.set_positions(W.positions)
    W.gone = sorted(set(range(3, N_DOCS, 61)) | {4096})
    _facet_side(W, O, N_DOCS, 77)
    W.cache = {}
    # ---- not vacuous, on the oracle's own numbers
    for ph in REFINED:
        uniq, seq = _seq(ph)
        n_ph = W.osh.search_phrase(uniq, seq, N_DOCS)[2]
        n_and = W.osh.search_exhaustive(uniq, O.OP_AND, N_DOCS)[2]
        assert 0 < n_ph < n_and, (ph, n_ph, n_and)
    m01 = set(_matches(W, O, [0, 1], [], False)[0].tolist())
    assert set(EDGE_DOCS) <= m01 and len(m01) > 1024  # (a page of 1500 takes two passes)
    m78 = _matches(W, O, [7, 8], [], False)[0]
    assert W.lonely in m78 and set(EDGE_DOCS) <= set(m78.tolist())
    both = np.intersect1d(W.lists[7], W.lists[8])
    assert np.count_nonzero(both // 64 == W.lonely // 64) == 1  # the only candidate of its group
    assert set(EDGE_DOCS) <= set(_matches(W, O, LONG, [], False)[0].tolist())
    assert 4096 not in _matches(W, O, [0, 1], [], True)[0] and len(_matches(W, O, [0, 1], [2], False)[0]) < len(m01)
    return W


def _matches(W, O, ph, neg, dead):
    """every match of the phrase with its score, by (score desc, doc asc): the oracle's full list less the docs of the NOT lists"""
    key = (tuple(ph), tuple(neg), dead)
    if key not in W.cache:
        uniq, seq = _seq(ph)
        W.osh.set_deleted(W.gone if dead else [])
        md, ms, tot = W.osh.search_phrase(uniq, seq, W.n_docs)
        assert len(md) == tot
        drop = np.concatenate([W.lists[t] for t in neg]) if neg else np.zeros(0, np.uint32)
        keep = ~np.isin(md, drop)
        W.cache[key] = (md[keep].astype(np.int64), ms[keep])
    return W.cache[key]


@pytest.fixture(scope="module")
def D(S, O):
    W = _dense_world(O)  # on the oracle alone, before any call on the device
    W.sh = S.Shard(0)
    W.sh.upload_lexical(N_DOCS, W.dl, W.offs, W.docs, W.tfs, W.positions)
    W.sh.upload_facets(W.raw)
    yield W
    W.sh.close()


# ------------------------------------------------------------------------------------------------ the checks of one query
def _hist(W, qf, docs):
    return _want_counts(W, qf, docs)


def _check_single_entries(S, W, sh, q, md, ms, flt, what, ks=(10,)):
    """ss_bm25_facet_count[_point], ss_bm25_facet_kth[_point] and ss_bm25_search_sorted of ONE query against its expected match set"""
    n = len(md)
    for qf in W.qfs:  # count: numeric ranges and string ids
        if qf["type"].startswith("string"):
            counts, other, tot = sh.facet_count(q, qf["offset"], qf["type"], n_buckets=len(qf["values"]), facet_filter=flt)
        else:
            counts, other, tot = sh.facet_count(q, qf["offset"], qf["type"], range_lower_bounds=[b for _, b in qf["ranges"]], facet_filter=flt)
        want = _hist(W, qf, md)
        assert tot == n, (what, qf["field"], tot, n)
        assert np.array_equal(counts, want[:-1]) and other == int(want[-1]), (what, qf["field"])
    qp = {"field": "loc", "offset": W.off["loc"], "type": "point", "ranges": _ranges(W.point_bounds)}
    counts, other, tot = sh.facet_count(q, W.off["loc"], "point", range_lower_bounds=W.point_bounds, facet_filter=flt, base=BASE, unit=UNIT)
    want = _hist(W, qp, md)
    assert tot == n and np.array_equal(counts, want[:-1]) and other == int(want[-1]), (what, "count_point")
    for col, desc, k in (("u16", True, 3), ("i32", False, max(n // 2, 1)), ("u8", True, n + 1)):  # kth
        vals = [int(x) for x in W.v[col][md]]
        v, nb, ne = naive.kth(vals, k, desc)
        bits, gb, ge, tot = sh.facet_kth(q, W.off[col], col, desc, k, facet_filter=flt)
        assert (gb, ge, tot) == (nb, ne, n), (what, col, desc, k, (gb, ge, tot), (nb, ne, n))
        if n:
            assert naive.facet_value(bits, col) == v, (what, col, desc, k)
    for desc, k in ((False, 2), (True, 5)):  # kth_point: by simplified_distance to the base
        v, nb, ne = naive.kth([float(x) for x in W.sortkey[md]], k, desc)
        bits, gb, ge, tot = sh.facet_kth(q, W.off["loc"], "point", desc, k, facet_filter=flt, base=BASE)
        assert (gb, ge, tot) == (nb, ne, n), (what, "kth_point", desc, k)
        if n:
            got = float(np.array([bits], np.uint64).view(np.float64)[0])
            assert np.isclose(got, v, rtol=1e-12, atol=0.0), (what, "kth_point", got, v)
    for srt in SORTS:  # sorted pages
        ref = _reference_order(W, md, ms, srt)
        for k in ks:
            doc, score, tot = sh.search_lexical_sorted(q, _spec(W, srt), k, facet_filter=flt)
            check_sorted(W, doc, score, tot, ref, srt, k, (what, "sorted", srt, k))


def _check_search_facets(S, W, sh, q, expected, flt, what, k=10):
    """ss_bm25_search_facets for each result type: counters == the histograms of every query's expected set, totals ==, the hits
    bit-identical to the filtered search's"""
    for rt in (S.ResultType.Topk, S.ResultType.TopkCount, S.ResultType.Count):
        doc, score, cnt, tot, per = sh.search_lexical_facets(q, k, W.qfs, rt, facet_filter=flt, reference_shortcuts=False)
        d2, s2, c2, t2 = sh.search_lexical_batch(q, k, rt, reference_shortcuts=False, facet_filter=flt)
        assert np.array_equal(doc, d2) and np.array_equal(score.view(np.uint32), s2.view(np.uint32)) and np.array_equal(cnt, c2), (what, rt)
        assert np.array_equal(tot, t2), (what, rt)
        for i, md in enumerate(expected):
            for f, qf in enumerate(W.qfs):
                assert np.array_equal(per[f][i], _hist(W, qf, md)), (what, rt, i, qf["field"])
            if rt != S.ResultType.Topk:
                assert int(tot[i]) == len(md), (what, rt, i, int(tot[i]), len(md))


# ------------------------------------------------------------------------------------------------ one indexed field, dense
@pytest.mark.parametrize("dead", [False, True])
@pytest.mark.parametrize("flt_name", [None, "numeric", "string"])
def test_dense_phrases_through_every_entry(S, O, D, dead, flt_name):
    """2 words, repeated words, 6 and 7 unique terms, a 12-word phrase, one and two NOT terms; tombstones on / off; no filter, a
    numeric and a string facet filter; count, count_point, kth, kth_point, sorted (k = 10; k = 1500 on the phrase with more matches
    than SS_MAX_K), search_facets for Topk / TopkCount / Count"""
    W, sh = D, D.sh
    sh.set_deleted(W.gone if dead else [])
    flt, keep = W.filters[flt_name]
    expected = []
    for ph, neg in DENSE_CASES:
        md, ms = _matches(W, O, ph, neg, dead)
        if keep is not None:
            md, ms = md[keep[md]], ms[keep[md]]
        expected.append(md)
        q = sh.make_queries([ph], S.QueryType.Phrase, [neg])
        deep = ph == [0, 1] and not neg and flt_name is None
        if deep:
            assert len(md) > 1024
        _check_single_entries(S, W, sh, q, md, ms, flt, (ph, neg, dead, flt_name), ks=(10, 1500) if deep else (10,))
    qb = sh.make_queries([c[0] for c in DENSE_CASES], S.QueryType.Phrase, [c[1] for c in DENSE_CASES])
    _check_search_facets(S, W, sh, qb, expected, flt, ("dense batch", dead, flt_name))
    sh.set_deleted([])


def test_batch_of_65_mixing_phrases_unions_and_intersections(S, O, D):
    """the chunk seam at 64, and queries that are no phrases left untouched by the refine: every row against its own oracle set"""
    W, sh = D, D.sh
    sh.set_deleted(W.gone)
    W.osh.set_deleted(W.gone)
    flt, keep = W.filters["numeric"]
    phrases = [c for c in DENSE_CASES]
    sets = [([0, 1], "and"), ([0, 1], "or"), ([2, 0], "and"), ([3, 4, 5], "or"), ([7, 8], "and"), ([7], "or"), ([0, 1, 2], "and")]
    rows, expected = [], []
    for i in range(65):
        if i % 3 != 1:  # rows 63, 64 and 65's neighbours: phrases on both sides of the seam
            ph, neg = phrases[(i // 3 + i) % len(phrases)]
            rows.append((ph, S.QueryType.Phrase, neg))
            md = _matches(W, O, ph, neg, True)[0]
        else:
            terms, op = sets[(i // 3) % len(sets)]
            rows.append((terms, S.QueryType.Union if op == "or" else S.QueryType.Intersection, []))
            W.osh.set_deleted(W.gone)
            md = W.osh.search_exhaustive(terms, O.OP_OR if op == "or" else O.OP_AND, N_DOCS)[0].astype(np.int64)
        expected.append(md[keep[md]])
    assert rows[63][1] == S.QueryType.Phrase and rows[64][1] == S.QueryType.Intersection or rows[64][1] in (S.QueryType.Phrase, S.QueryType.Union)
    assert {r[1] for r in rows[:64]} == {S.QueryType.Phrase, S.QueryType.Union, S.QueryType.Intersection}
    qb = sh.make_queries([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    _check_search_facets(S, W, sh, qb, expected, flt, "batch of 65")
    # the sorted entry over the same batch: two chunks, phrases and set queries side by side
    srt = SORTS[1]
    bd, bs, bc, bt = sh.search_lexical_sorted_batch(qb, _spec(W, srt), 10, facet_filter=flt)
    for i, (terms, qt, neg) in enumerate(rows):
        assert int(bt[i]) == len(expected[i]), (i, terms, qt)
        vals = [[W.vals[c][j] for j in W.idx[c][expected[i]]] for c, _ in srt]
        got = [[W.vals[c][j] for j in W.idx[c][bd[i][:bc[i]].astype(np.int64)]] for c, _ in srt]
        order = sorted(range(len(expected[i])), key=lambda j: (vals[0][j], -vals[1][j]))[:10]
        assert bc[i] == min(10, len(expected[i])) and set(bd[i][:bc[i]].tolist()) <= set(expected[i].tolist()), (i, terms)
        assert got == [[v[j] for j in order] for v in vals], (i, terms, qt)
    sh.set_deleted([])


# ------------------------------------------------------------------------------------------------ three indexed fields, merged lists
F_DFS = [5000, 3800, 6500, 1600, 2400, 80]
F_PLANT = [([0, 1], 0, 120), ([0, 1], 2, 90), ([0, 1, 2], 1, 60), ([2, 0, 2], 0, 40), ([3, 4], 2, 40), ([1, 1], 2, 30)]
F_CROSS = [(0, 1, 150), (3, 4, 120)]
F_BOOST = np.array([2.0, 1.0, 0.5], np.float32)
# (phrase, field filter): none; one that lists the phrase's field; one under which [3, 4] stands only in an unlisted field
F_CASES = [([0, 1], ()), ([0, 1, 2], ()), ([2, 0, 2], ()), ([3, 4], ()), ([1, 1], ()), ([0, 1], (2,)), ([0, 1], (0, 1)), ([3, 4], (2,)),
           ([3, 4], (0,)), ([3, 4], (0, 1)), ([0, 1, 2], (1,))]


def _fields_world(O):
    W = World()
    W.arrays = _corpus_fields(O, N_DOCS, 3, F_DFS, 19, F_PLANT, F_CROSS)
    W.gone = list(range(5, N_DOCS, 89))
    _facet_side(W, O, N_DOCS, 91)
    W.cache = {}
    dl, offs, docs, fields, tfs, positions = W.arrays
    n_ref = 0
    for ph in ([0, 1], [0, 1, 2], [2, 0, 2], [3, 4]):
        uniq, seq = _seq(ph)
        n_ph = len(_fields_matches(W, O, ph, (), False)[0])
        n_and = O.search_fields_exhaustive(N_DOCS, dl, F_BOOST, offs, docs, fields, tfs, uniq, O.OP_AND, N_DOCS)[2]
        assert 0 < n_ph < n_and, (ph, n_ph, n_and)
        n_ref += 1
    assert n_ref >= 3
    # the cross docs: 3 and 4 adjacent across a field boundary in 120 docs that the phrase does not match
    n34 = len(_fields_matches(W, O, [3, 4], (), False)[0])
    n34_and = O.search_fields_exhaustive(N_DOCS, dl, F_BOOST, offs, docs, fields, tfs, [3, 4], O.OP_AND, N_DOCS)[2]
    assert 40 <= n34 <= n34_and - 100
    # [3, 4] was planted in field 2: under a filter that lists only field 0 the intersection of the words still holds docs
    assert len(_fields_matches(W, O, [3, 4], (0,), False)[0]) < len(_fields_matches(W, O, [3, 4], (2,), False)[0]) and n34_and > 0
    return W


def _fields_matches(W, O, ph, filt, dead):
    key = (tuple(ph), tuple(filt), dead)
    if key not in W.cache:
        dl, offs, docs, fields, tfs, positions = W.arrays
        uniq, seq = _seq(ph)
        md, ms, tot = O.search_fields_phrase(N_DOCS, dl, F_BOOST, offs, docs, fields, tfs, positions, uniq, seq, N_DOCS,
                                             deleted=W.gone if dead else (), field_filter=filt, reference_loop=False)
        assert len(md) == tot
        W.cache[key] = (md.astype(np.int64), ms)
    return W.cache[key]


@pytest.mark.parametrize("dead", [False, True])
def test_phrases_over_three_indexed_fields(S, O, dead):
    """merged lists and field-tagged positions: no field filter, a filter that lists the phrase's field, one under which the phrase
    stands only in an unlisted field; words adjacent across a field boundary are no phrase"""
    W = _fields_world(O)
    dl, offs, docs, fields, tfs, positions = W.arrays
    sh = S.Shard(0)
    try:
        sh.upload_lexical_fields(N_DOCS, dl, F_BOOST, offs, docs, fields, tfs, positions)
        assert sh.fields_info()[1]
        sh.upload_facets(W.raw)
        sh.set_deleted(W.gone if dead else [])
        for flt_name in (None, "numeric"):
            flt, keep = W.filters[flt_name]
            for filt in sorted({c[1] for c in F_CASES}):
                cases = [c for c in F_CASES if c[1] == filt]
                expected = []
                for ph, _ in cases:
                    md, ms = _fields_matches(W, O, ph, filt, dead)
                    if keep is not None:
                        md, ms = md[keep[md]], ms[keep[md]]
                    expected.append(md)
                    q = sh.make_queries([ph], S.QueryType.Phrase, field_filter=filt)
                    _check_single_entries(S, W, sh, q, md, ms, flt, ("fields", ph, filt, dead, flt_name))
                qb = sh.make_queries([c[0] for c in cases], S.QueryType.Phrase, field_filter=filt)
                _check_search_facets(S, W, sh, qb, expected, flt, ("fields batch", filt, dead, flt_name))
    finally:
        sh.close()


# ------------------------------------------------------------------------------------------------ n-gram keys
def test_phrases_with_ngram_keys(S, O):
    """the reference's default index: a phrase naming an n-gram key carries SS_PHRASE_SKIP places, and the key's other component terms
    are unique terms no place names"""
    import ngram_corpus as NG
    from oracle import ref_format as RF
    from seekstorm_amd.search import idf_f32
    Cn = NG.build(O, _corpus, N_DOCS, [4300, 1700, 2900, 430],
                  [([0, 1], 60), ([0, 1, 2], 50), ([3, 0, 1], 30), ([0, 1, 3], 30), ([0, 1, 2, 3], 20), ([2, 0, 1], 30), ([0, 1, 0, 1], 15), ([3, 0, 1, 2], 15)], 12)
    osh = Cn.oracle_shard(O)
    W = World()
    _facet_side(W, O, N_DOCS, 5)
    data = RF.write_index_bin(N_DOCS, Cn.dl, Cn.terms, np.random.default_rng(3), key_head_size=23, ngram_terms=Cn.ngram_terms)
    ix = S.IndexBin(data, key_head_size=23)
    sh = S.Shard(0)
    try:
        sh.upload_index_bin(ix, positions=True)
        sh.upload_facets(W.raw)
        tid = {t: ix.term_of_key(NG.KEY(t)) for t in range(4)}
        ent, idf_of = {}, {}
        for words, key in NG.KEYS.items():
            comp = ix.terms_of_key(key)
            ent[words] = tuple(t for t, _ in comp)
            idf_of.update({t: i for t, i in comp})
        gone = list(range(7, N_DOCS, 53))
        sh.set_deleted(gone)
        osh.set_deleted(gone)
        flt, keep = W.filters["numeric"]
        refined, expected = 0, []
        gq = sh.make_queries([[ent[e] if isinstance(e, tuple) else tid[e] for e in ph] for ph in NG.PHRASES], S.QueryType.Phrase, idf_of=idf_of)
        assert (gq["phrase_seq"] == 0xFF).any()  # SS_PHRASE_SKIP places are in the batch
        for i, ph in enumerate(NG.PHRASES):
            uniq, seq, places, idf = Cn.oracle_query(ph, lambda e, c: idf_of[ent[e][c]], lambda l: float(idf_f32(N_DOCS, osh.df(l))))
            md, ms, tot = osh.search_phrase_items(uniq, seq, places, N_DOCS, idf=idf, reference_loop=True)
            assert len(md) == tot > 0, ph
            refined += tot < osh.search_exhaustive(uniq, O.OP_AND, N_DOCS)[2]
            md = md.astype(np.int64)
            md, ms = md[keep[md]], ms[keep[md]]
            expected.append(md)
            _check_single_entries(S, W, sh, gq[i:i + 1], md, ms, flt, ("ngram", ph))
        assert refined >= 3
        _check_search_facets(S, W, sh, gq, expected, flt, "ngram batch")
    finally:
        sh.close()


# ------------------------------------------------------------------------------------------------ sparse tier with positions
SP_DFS = [5000, 3700, 1500, 90, 60, 250, 12]
SP_ND = 3
SP_PLANT = [([0, 3], 40), ([3, 4], 25), ([1, 3, 2], 30), ([5, 0, 5], 25), ([4, 4], 15), ([0, 1], 100), ([6, 5, 3, 0, 1], 8), ([2, 5], 30), ([3, 5], 20)]
# sparse first / last / all sparse / mixed with dense / repeated; NOT terms of either tier
SP_CASES = [([3, 0], []), ([0, 3], []), ([3, 4], []), ([1, 3, 2], []), ([5, 0, 5], []), ([4, 4], []), ([6, 5, 3, 0, 1], []), ([2, 5], []), ([3, 5], []),
            ([0, 3], [1]), ([2, 5], [3, 0]), ([3, 4], [5]), ([0, 1], [3]), ([0, 1], [])]


def _sparse_world(O):
    W = World()
    arrays = _corpus(O, N_DOCS, SP_DFS, 23, SP_PLANT)
    edge = [(ph, d, 300 + 20 * j) for d in EDGE_DOCS for j, ph in enumerate(([0, 3], [3, 4], [0, 1]))]
    arrays = _plant_at(arrays, len(SP_DFS), edge)  # (doc 0 of list 3: the tier's very first posting, positions from 0 on)
    W.dl, W.offs, W.docs, W.tfs, W.positions = arrays
    W.lists = [W.docs[int(W.offs[t]):int(W.offs[t + 1])] for t in range(len(SP_DFS))]
    assert int(W.lists[SP_ND][0]) == 0
    W.osh = O.Shard(N_DOCS, W.dl, W.offs, W.docs, W.tfs)
    W.osh.set_positions(W.positions)
    W.gone = sorted(set(range(3, N_DOCS, 61)) | {4095})
    _facet_side(W, O, N_DOCS, 13)
    W.cache = {}
    n_ref = 0
    for ph in ([0, 3], [1, 3, 2], [2, 5], [0, 1], [3, 5]):
        uniq, seq = _seq(ph)
        n_ph = W.osh.search_phrase(uniq, seq, N_DOCS)[2]
        n_and = W.osh.search_exhaustive(uniq, O.OP_AND, N_DOCS)[2]
        n_ref += 0 < n_ph < n_and
    assert n_ref >= 3
    assert set(EDGE_DOCS) <= set(_matches(W, O, [3, 4], [], False)[0].tolist()) and set(EDGE_DOCS) <= set(_matches(W, O, [0, 3], [], False)[0].tolist())
    return W


def _upload_sparse_world(S, W, sparse_positions=True, dense_positions=True):
    e = int(W.offs[SP_ND])
    pe = int(W.tfs[:e].astype(np.int64).sum())
    sh = S.Shard(0)
    sh.upload_lexical(N_DOCS, W.dl, W.offs[:SP_ND + 1], W.docs[:e], W.tfs[:e], W.positions[:pe] if dense_positions else None)
    mid = SP_ND + 2  # two appends: the second one's postings follow the first one's in the tier
    m = int(W.offs[mid]); pm = int(W.tfs[:m].astype(np.int64).sum())
    if sparse_positions:
        assert sh.append_sparse(W.offs[SP_ND:mid + 1] - W.offs[SP_ND], W.docs[e:m], W.tfs[e:m], positions=W.positions[pe:pm]) == SP_ND
        assert sh.append_sparse(W.offs[mid:] - W.offs[mid], W.docs[m:], W.tfs[m:], positions=W.positions[pm:]) == mid
    else:
        assert sh.append_sparse(W.offs[SP_ND:] - W.offs[SP_ND], W.docs[e:], W.tfs[e:]) == SP_ND
    sh.upload_facets(W.raw)
    return sh


@pytest.mark.parametrize("dead", [False, True])
def test_phrases_naming_sparse_terms(S, O, dead):
    """append_sparse with positions: the sparse term first, last, alone, mixed with dense words, repeated; NOT terms of either tier; the
    tier's very first posting (doc 0 of the first sparse list) carries a match"""
    W = _sparse_world(O)
    sh = _upload_sparse_world(S, W)
    try:
        sh.set_deleted(W.gone if dead else [])
        for flt_name in (None, "string"):
            flt, keep = W.filters[flt_name]
            expected = []
            for ph, neg in SP_CASES:
                md, ms = _matches(W, O, ph, neg, dead)
                if keep is not None:
                    md, ms = md[keep[md]], ms[keep[md]]
                expected.append(md)
                q = sh.make_queries([ph], S.QueryType.Phrase, [neg])
                _check_single_entries(S, W, sh, q, md, ms, flt, ("sparse", ph, neg, dead, flt_name))
            if not dead and flt_name is None:
                assert 0 in expected[1] and 0 in expected[2]  # [0, 3] and [3, 4] on doc 0
            qb = sh.make_queries([c[0] for c in SP_CASES], S.QueryType.Phrase, [c[1] for c in SP_CASES])
            _check_search_facets(S, W, sh, qb, expected, flt, ("sparse batch", dead, flt_name))
    finally:
        sh.close()


def test_phrases_naming_sparse_terms_over_three_indexed_fields(S, O):
    """the sparse tier of a multi-field image (append_sparse_fields with positions): merged weights, field-tagged positions, with and
    without a field filter"""
    dfs, nd = [5000, 3800, 1600, 90, 200, 40], 3
    plant = [([0, 3], 0, 40), ([0, 3], 2, 30), ([3, 4], 1, 25), ([1, 4, 2], 2, 25), ([5, 0, 5], 0, 15), ([3, 3], 1, 12), ([0, 1], 0, 80)]
    arrays = _corpus_fields(O, N_DOCS, 3, dfs, 29, plant, [(0, 3, 60), (3, 4, 40)])
    dl, offs, docs, fields, tfs, positions = arrays
    W = World()
    _facet_side(W, O, N_DOCS, 17)
    gone = list(range(5, N_DOCS, 89))
    e = int(offs[nd]); pe = int(tfs[:e].astype(np.int64).sum())
    want = {}
    n_ref = 0
    cases = [([0, 3], ()), ([3, 0], ()), ([3, 4], ()), ([1, 4, 2], ()), ([5, 0, 5], ()), ([3, 3], ()), ([0, 1], ()), ([0, 3], (0,)), ([0, 3], (1, 2)), ([3, 4], (0,))]
    for ph, filt in cases:
        uniq, seq = _seq(ph)
        md, ms, tot = O.search_fields_phrase(N_DOCS, dl, F_BOOST, offs, docs, fields, tfs, positions, uniq, seq, N_DOCS, deleted=gone, field_filter=filt,
                                             reference_loop=False)
        assert len(md) == tot
        want[(tuple(ph), filt)] = (md.astype(np.int64), ms)
        if not filt:
            n_ref += 0 < tot < O.search_fields_exhaustive(N_DOCS, dl, F_BOOST, offs, docs, fields, tfs, uniq, O.OP_AND, N_DOCS, (), gone)[2]
    assert n_ref >= 3
    sh = S.Shard(0)
    try:
        sh.upload_lexical_fields(N_DOCS, dl, F_BOOST, offs[:nd + 1], docs[:e], fields[:e], tfs[:e], positions[:pe])
        assert sh.append_sparse_fields(offs[nd:] - offs[nd], docs[e:], fields[e:], tfs[e:], positions=positions[pe:]) == nd
        sh.upload_facets(W.raw)
        sh.set_deleted(gone)
        flt, keep = W.filters["numeric"]
        for filt in ((), (0,), (1, 2)):
            sub = [c for c in cases if c[1] == filt]
            expected = []
            for ph, _ in sub:
                md, ms = want[(tuple(ph), filt)]
                md, ms = md[keep[md]], ms[keep[md]]
                expected.append(md)
                q = sh.make_queries([ph], S.QueryType.Phrase, field_filter=filt)
                _check_single_entries(S, W, sh, q, md, ms, flt, ("sparse fields", ph, filt))
            qb = sh.make_queries([c[0] for c in sub], S.QueryType.Phrase, field_filter=filt)
            _check_search_facets(S, W, sh, qb, expected, flt, ("sparse fields batch", filt))
    finally:
        sh.close()


# ------------------------------------------------------------------------------------------------ what stays SS_ENOTSUP
def _code(call):
    from seekstorm_amd import _native as N
    try:
        call()
    except N.SeekStormHipError as e:
        return e.code
    return N.SS_OK


def _entries(S, W, sh, q):
    """the three single-query entries and ss_bm25_search_facets, one query each"""
    return [_code(lambda: sh.facet_count(q, W.off["i32"], "i32", range_lower_bounds=[0])),
            _code(lambda: sh.facet_kth(q, W.off["i32"], "i32", True, 3)),
            _code(lambda: sh.search_lexical_sorted_batch(q, [(W.off["i32"], "i32", True)], 10)),
            _code(lambda: sh.search_lexical_facets(q, 10, W.qfs, S.ResultType.TopkCount, reference_shortcuts=False))]


def test_what_stays_not_supported(S, O, D):
    """the residual list: no positions in the image, none in the sparse tier for a phrase naming a sparse term,
    several indexed fields without merged lists, a dense list with neither a probe row nor a pool row, a place naming unique term 12 or
    later -- each SS_ENOTSUP from every entry, and the same phrase answered where the image holds what it needs"""
    from seekstorm_amd import _native as N
    W = D
    ENOTSUP, OK = [N.SS_ENOTSUP] * 4, [N.SS_OK] * 4
    # no positions in the image
    bare = S.Shard(0)
    try:
        bare.upload_lexical(N_DOCS, W.dl, W.offs, W.docs, W.tfs)
        bare.upload_facets(W.raw)
        assert _entries(S, W, bare, bare.make_queries([[0, 1]], S.QueryType.Phrase)) == ENOTSUP
        assert _code(lambda: bare.search_lexical_batch(bare.make_queries([[0, 1]], S.QueryType.Phrase), 10)) == N.SS_ESTATE  # (the search's own answer)
    finally:
        bare.close()
    assert _entries(S, W, W.sh, W.sh.make_queries([[0, 1]], S.QueryType.Phrase)) == OK
    # a sparse tier without positions: the phrase naming a sparse term is refused, the all-dense phrase answers
    Wsp = _sparse_world(O)
    for sparse_positions, want in ((False, ENOTSUP), (True, OK)):
        sh = _upload_sparse_world(S, Wsp, sparse_positions=sparse_positions)
        try:
            assert _entries(S, Wsp, sh, sh.make_queries([[0, 3]], S.QueryType.Phrase)) == want, sparse_positions
            assert _entries(S, Wsp, sh, sh.make_queries([[0, 1]], S.QueryType.Phrase)) == OK
        finally:
            sh.close()
    # several indexed fields without merged lists (boosts that keep them from being built), against the same corpus with them
    arrays = _corpus_fields(O, N_DOCS, 3, F_DFS, 19, F_PLANT, F_CROSS)
    dl, offs, docs, fields, tfs, positions = arrays
    for merged, want in ((False, ENOTSUP), (True, OK)):
        sh = S.Shard(0)
        try:
            if merged:
                sh.upload_lexical_fields(N_DOCS, dl, F_BOOST, offs, docs, fields, tfs, positions)
            else:  # (field-tagged positions belong to the merged lists: the upload takes none without them)
                sh.upload_lexical_fields(N_DOCS, dl, [4096.0, 1.0, 1.0 / 4096.0], offs, docs, fields, tfs)
            assert bool(sh.fields_info()[1]) == merged
            sh.upload_facets(W.raw)
            assert _entries(S, W, sh, sh.make_queries([[0, 1]], S.QueryType.Phrase)) == want, merged
        finally:
            sh.close()
    # a dense list with neither a probe row nor a pool row
    n_sub = (N_DOCS + 4095) // 4096
    for budget, want in ((4 * n_sub * 64 * 12, ENOTSUP), (None, OK)):
        sh = S.Shard(0)
        try:
            if budget:
                sh.set_probe_budget(budget)  # three rows and the all-zero row, no pool: the short lists 7 and 8 have no bit records
            sh.upload_lexical(N_DOCS, W.dl, W.offs, W.docs, W.tfs, W.positions)
            sh.upload_facets(W.raw)
            assert _entries(S, W, sh, sh.make_queries([[7, 8]], S.QueryType.Phrase)) == want, budget
        finally:
            sh.close()
    # a place that names unique term 12: the search refuses it, and so do these entries.  Thirteen unique terms need thirteen lists: a
    # world of its own, tiny
    dfs13 = [400] * 13
    a13 = _corpus(O, 4099, dfs13, 3, [(list(range(13))[:12], 30)])
    sh = S.Shard(0)
    try:
        sh.upload_lexical(4099, *a13)
        W13 = World()
        _facet_side(W13, O, 4099, 3)
        sh.upload_facets(W13.raw)
        q = sh.make_queries([list(range(12))], S.QueryType.Phrase)
        assert _entries(S, W13, sh, q) == OK  # twelve unique terms, twelve places: answered
        q["n_terms"][0] = 13
        q["term"][0, 12] = 12
        q["idf"][0, 12] = q["idf"][0, 0]
        q["phrase_seq"][0, 11] = 12
        assert _entries(S, W13, sh, q) == ENOTSUP
        assert _code(lambda: sh.search_lexical_batch(q, 10)) == N.SS_ENOTSUP
    finally:
        sh.close()


# ------------------------------------------------------------------------------------------------ two shards, both mirrors
class _SortC(C.Structure):  # ssh_result_sort
    _fields_ = [("facet_offset", C.c_uint32), ("facet_type", C.c_uint32), ("descending", C.c_uint32), ("reserved", C.c_uint32), ("base", C.c_double * 2)]


def _cpp_index_sorted(shards, terms, qt, offset, length, sorts):
    from seekstorm_amd import _native as N
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    H = host_lib()
    H.ssh_index_adopt.restype = C.c_void_p
    H.ssh_index_adopt.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    H.ssh_index_destroy.argtypes = [C.c_void_p]
    H.ssh_index_search_sorted.restype = C.c_int
    H.ssh_index_search_sorted.argtypes = [C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.c_uint32, u64p, f32p, u64p]
    handles = (C.c_void_p * len(shards))(*[sh._h for sh in shards])
    ix = H.ssh_index_adopt(len(shards), handles, (C.c_int * len(shards))(*([0] * len(shards))))
    try:
        sarr = (_SortC * len(sorts))()
        for i, so in enumerate(sorts):
            sarr[i].facet_offset, sarr[i].facet_type, sarr[i].descending = so[0], N.FACET_TYPES[so[1]], 1 if so[2] else 0
        t = np.ascontiguousarray(terms, np.uint32)
        cap = length + 1
        doc, sc, meta = np.zeros(cap, np.uint64), np.zeros(cap, np.float32), np.zeros(4, np.uint64)
        n = H.ssh_index_search_sorted(ix, t.ctypes.data_as(u32p), len(t), int(qt), offset, length, 0, None, C.cast(sarr, C.c_void_p), len(sorts), cap,
                                      doc.ctypes.data_as(u64p), sc.ctypes.data_as(f32p), meta.ctypes.data_as(u64p))
        assert n >= 0 and int(meta[3]) == 0, (n, meta)
        return doc[:n].astype(np.int64), sc[:n], int(meta[1])
    finally:
        H.ssh_index_destroy(ix)


def test_two_shards_through_both_mirrors(S, O, D):
    """Index.search(query_type_default = Phrase) with query_facets, and with result_sort, over two shards, Python and C++: against the
    oracle's per-shard phrase sets -- the facet maps finished and merged by the restated crate code, the sorted page by the reference's
    order over the union of the shards' matches"""
    W0 = D
    W0.sh.set_deleted([])
    n1 = 12_007
    W1 = World()
    W1.dl, W1.offs, W1.docs, W1.tfs, W1.positions = _corpus(O, n1, [3600, 2700, 4800, 1200, 1800], 57, [([0, 1], 300), ([0, 1, 2], 40), ([2, 0, 2], 30), ([3, 4], 20)])
    W1.lists = [W1.docs[int(W1.offs[t]):int(W1.offs[t + 1])] for t in range(5)]
    W1.osh = O.Shard(n1, W1.dl, W1.offs, W1.docs, W1.tfs)
    W1.osh.set_positions(W1.positions)
    W1.gone, W1.cache = [], {}
    _facet_side(W1, O, n1, 58)
    W1.sh = S.Shard(0, shard_id=1)
    try:
        W1.sh.upload_lexical(n1, W1.dl, W1.offs, W1.docs, W1.tfs, W1.positions)
        W1.sh.upload_facets(W1.raw)
        Ws = [W0, W1]
        ix = S.Index([W0.sh, W1.sh])
        qfs = [
            {"field": "i32", "offset": W0.off["i32"], "type": "i32", "ranges": _ranges([-(1 << 31), -5, 0, 7, 1_500_000_000]), "range_type": "above"},
            {"field": "s16", "offset": W0.off["s16"], "type": "string16", "values": ["a%d" % i for i in range(S16_BUCKETS)], "prefix": "a1", "length": 7},
        ]
        for ph in ([0, 1], [0, 1, 2], [2, 0, 2], [3, 4]):
            per_shard = [_matches(Wi, O, ph, [], False) for Wi in Ws]
            total = sum(len(m[0]) for m in per_shard)
            assert total > 0
            # ---- query_facets
            shard_lists, merged = [], []
            for sid, (Wi, (md, ms)) in enumerate(zip(Ws, per_shard)):
                merged += [(-float(s), int(d) * 2 + sid) for d, s in zip(md[:10], ms[:10])]
                m = {}
                for qf in qfs:
                    ref = ref_shard_map(qf, _want_counts(Wi, qf, md), 2)
                    if ref is not None and ref[0]:
                        m[qf["field"]] = ref[0]
                shard_lists.append(m)
            want = ref_planner(qfs, shard_lists, S.ResultType.TopkCount)
            ro = ix.search(ph, None, S.QueryType.Phrase, S.SearchMode.Lexical, 0, 10, S.ResultType.TopkCount, strict=True, query_facets=qfs)
            cd, cs, ctot, cfac = _cpp_index_search([W0.sh, W1.sh], ph, S.QueryType.Phrase, 0, 10, S.ResultType.TopkCount, None, 0, qfs)
            merged.sort()
            ws = np.array([-s for s, _ in merged[:10]], np.float32)
            for who, facets, tot_, scores in (("python", ro.facets, ro.result_count_total, [r.score for r in ro.results]), ("c++", cfac, ctot, cs)):
                assert tot_ == total, (who, ph, tot_, total)
                assert set(facets) == set(want), (who, ph, set(facets) ^ set(want))
                for field, (full, cut) in want.items():
                    same_facet([(a, int(c)) for a, c in facets[field]], full, cut, (who, ph, field))
                assert np.allclose(scores, ws, rtol=1e-4, atol=1e-7), (who, ph)
            # ---- result_sort: global ids = local * 2 + shard, every doc's keys from its own shard
            srt = SORTS[1]
            gd = np.concatenate([m[0] * 2 + sid for sid, m in enumerate(per_shard)])
            gs = np.concatenate([m[1] for m in per_shard])
            cols = [np.concatenate([Wi.v[c][m[0]] for Wi, m in zip(Ws, per_shard)]).astype(np.int64).tolist() for c, _ in srt]
            order = naive.sorted_order(gd, gs, cols, [d for _, d in srt])
            for off_, length in ((0, 10), (5, 40)):
                n = min(length, max(total - off_, 0))
                pick = order[off_:off_ + n]
                ro = ix.search(ph, None, S.QueryType.Phrase, S.SearchMode.Lexical, off_, length, strict=True, result_sort=_spec(W0, srt))
                cd, cs, ctot = _cpp_index_sorted([W0.sh, W1.sh], ph, S.QueryType.Phrase, off_, length, _spec(W0, srt))
                for who, docs_, scores, tot_ in (("python", [r.doc_id for r in ro.results], [r.score for r in ro.results], ro.result_count_total),
                                                 ("c++", cd.tolist(), cs, ctot)):
                    assert tot_ == total and len(docs_) == n and len(set(docs_)) == n, (who, ph, off_, length)
                    key_of = dict(zip(gd.tolist(), zip(*cols)))
                    assert [key_of[d] for d in docs_] == [tuple(c[i] for c in cols) for i in pick], (who, ph, off_, length)
                    assert np.allclose(scores, gs[pick], rtol=1e-4), (who, ph, off_, length)
    finally:
        W1.sh.close()
