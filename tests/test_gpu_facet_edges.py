"""Facet filters, counts, pivots and result sorts (facet.hip) at every type's extreme values (-m gpu).

One world: 100 003 docs (the last 64-doc group of every bitmap is partial), five terms from ~20 docs to most of the corpus, a few
tombstones, and a packed facet record of odd size holding every numeric type at an unaligned offset, string16 / string32 ids and two
float columns with NaNs.  Column values come from oracle/naive.py's per-type palettes (min / max and their neighbours, +-0, +-inf,
subnormals, pairs that differ in one byte), skewed so that large tie groups straddle k.  40 records beyond the lexical image hold values
that would change any answer if a kernel read them.  Every answer is checked against oracle/naive.py's facet reference (plain values,
no key transform) over the CPU oracle's match set and scores."""
import numpy as np
import pytest

from oracle import naive
from test_gpu_parity import REL, _check_topk

pytestmark = pytest.mark.gpu

N_DOCS = 100_003
N_EXTRA = 40
DFS = [0.0002, 0.004, 0.04, 0.3, 0.85]  # df / N of terms 0..4
NUMERIC = ["u8", "u16", "u32", "u64", "i8", "i16", "i32", "i64", "f32", "f64"]
# packed, odd size, every multi-byte field at an offset that is not a multiple of its width; the last field ends on the last byte
REC = np.dtype([("u8", "u1"), ("i64", "<i8"), ("u16", "<u2"), ("f32", "<f4"), ("i8", "i1"), ("pad", "u1"), ("u64", "<u8"),
                ("i16", "<i2"), ("f64", "<f8"), ("u32", "<u4"), ("i32", "<i4"), ("s16", "<u2"), ("nf32", "<f4"), ("nf64", "<f8"),
                ("s32", "<u4")])
COL_TYPE = dict({t: t for t in NUMERIC}, s16="string16", s32="string32", nf32="f32", nf64="f64")
N_BUCKETS = 48  # string ids at or above it are counted as "other"
HI, LO = naive.FACET_HI_INCLUSIVE, naive.FACET_LO_EXCLUSIVE


class World:
    pass


def facet_world(S, O):
    """the shard, its oracle, and per column: the palette values (vals[col]) and every doc's index into them (idx[col])"""
    W = World()
    th = O.term_thresholds().copy()
    for t, f in enumerate(DFS):
        th[t] = int(f * 2.0 ** 32)
    W.offs, W.docs, W.tfs = O.lex_corpus(N_DOCS, list(range(len(DFS))), thresholds=th)
    W.dl = O.lex_doclen(N_DOCS)
    W.osh = O.Shard(N_DOCS, W.dl, W.offs, W.docs, W.tfs)
    rng = np.random.default_rng(2026)
    W.vals, W.idx = {}, {}
    rec = np.zeros(N_DOCS + N_EXTRA, REC)
    for col in NUMERIC + ["nf32", "nf64"]:
        ty = COL_TYPE[col]
        pal = naive.facet_palette(ty)
        p = np.full(len(pal), 1.0)
        if ty[0] == "f":  # +-0 hold 30 % of the docs, split evenly by sign
            z = [i for i, x in enumerate(pal) if x == 0.0]
            p[:] = 0.7 / (len(pal) - 2)
            p[z] = 0.15
        else:  # one value holds 30 %
            p[:] = 0.7 / (len(pal) - 1)
            p[len(pal) // 2] = 0.3
        bits = [naive.facet_bits(x, ty) for x in pal]
        if col.startswith("nf"):  # NaN in 20 % of the docs (quiet, negative with a payload, signalling): a column no sort uses
            nan_bits = naive.facet_nan_palette(ty)
            pal, bits = pal + [float("nan")] * len(nan_bits), bits + nan_bits
            p = np.concatenate([p * 0.8, np.full(len(nan_bits), 0.2 / len(nan_bits))])
        W.vals[col] = pal
        W.idx[col] = rng.choice(len(pal), N_DOCS, p=p / p.sum())
        ub = np.array(bits, np.uint64)
        rec[col][:N_DOCS] = ub[W.idx[col]].astype("<u%d" % REC[col].itemsize).view(REC[col])
        # beyond the lexical image: alternately the type's least and greatest value (the best under one direction or the other)
        extra = np.where(np.arange(N_EXTRA) % 2 == 0, 0, len(naive.facet_palette(ty)) - 1)
        rec[col][N_DOCS:] = ub[extra].astype("<u%d" % REC[col].itemsize).view(REC[col])
    W.vals["s16"] = list(range(N_BUCKETS + 16)) + [65535]
    W.vals["s32"] = list(range(N_BUCKETS + 16)) + [1 << 20, 0xFFFFFFFF]
    for col in ("s16", "s32"):
        W.idx[col] = rng.integers(0, len(W.vals[col]), N_DOCS)
        rec[col][:N_DOCS] = np.array(W.vals[col], np.uint64)[W.idx[col]].astype(REC[col])
        rec[col][N_DOCS:] = 3
    W.rec = rec
    W.off = {n: REC.fields[n][1] for n in REC.names}
    W.sh = S.Shard(0)
    W.sh.upload_lexical(N_DOCS, W.dl, W.offs, W.docs, W.tfs)
    W.sh.upload_facets(rec.view(np.uint8).reshape(N_DOCS + N_EXTRA, REC.itemsize))
    W.gone = list(range(13, N_DOCS, 997))
    W.sh.set_deleted(W.gone)
    W.osh.set_deleted(W.gone)
    U, I = S.QueryType.Union, S.QueryType.Intersection
    # (terms, query type, oracle op, NOT terms): ~20 matches (fewer than k), hundreds, thousands, tens of thousands, most of the corpus,
    # a NOT term, none, one
    W.queries = [([0], U, O.OP_OR, []), ([1], U, O.OP_OR, []), ([2, 1], U, O.OP_OR, []), ([3, 4], I, O.OP_AND, []),
                 ([4, 3, 2], U, O.OP_OR, []), ([4], U, O.OP_OR, [3]), ([0, 1], I, O.OP_AND, []), ([0, 3], I, O.OP_AND, [4])]
    W.matches = []
    for terms, _, op, neg in W.queries:  # every match with its score, by (score desc, doc asc)
        md, ms, tot = W.osh.search_exhaustive(terms, op, N_DOCS, neg)
        assert len(md) == tot
        W.matches.append((md.astype(np.int64), ms))
    assert [len(m[0]) for m in W.matches][-2:] == [0, 1] and len(W.matches[0][0]) < 30 and len(W.matches[4][0]) > 80_000
    return W


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


@pytest.fixture(scope="module")
def W(S):
    from oracle import oracle as O
    W = facet_world(S, O)
    yield W
    W.sh.close()


def value_of(W, col, docs):
    """the palette values of docs (Python ints / floats)"""
    v = W.vals[col]
    return [v[i] for i in W.idx[col][np.asarray(docs, np.int64)]]


def _filter(S, W, col, lo, hi, flags=0):
    """(the ss_facet_filter tuple, the reference's keep mask over the docs): flags == 0 in the value form, else in the "bits" form"""
    ty = COL_TYPE[col]
    if flags:
        fb = lambda x: S.Shard._facet_filter_bits(naive.facet_bits(x, ty), ty)
        t = (W.off[col], ty, fb(lo), fb(hi), "bits", flags)
    else:
        t = (W.off[col], ty, lo, hi)
    keep = np.array([naive.facet_pass(x, ty, lo, hi, flags) for x in W.vals[col]])[W.idx[col]]
    return t, keep


def _set(S, W, col, ids):
    keep = np.isin(np.array(W.vals[col], np.int64)[W.idx[col]], ids)
    return (W.off[col], COL_TYPE[col], list(ids)), keep


def test_facet_filters_at_the_edges(S, W):
    """every type: lo == hi, lo > hi, the full range (which excludes the maximum), the four flag combinations on palette values
    through the "bits" form; float ends at +-0, +-inf and NaN; NaN values; string ids beyond the width; two and eight filters at once
    on top of tombstones.  Unions, intersections, NOT terms; both strategies; TopkCount and Count; all queries in one call (the
    one-launch path).  Totals exact, top-k by the parity rule, every returned doc passes."""
    sets = []
    for col in NUMERIC:
        pal = W.vals[col]
        sets += [[_filter(S, W, col, pal[1], pal[1])], [_filter(S, W, col, pal[-2], pal[1])], [_filter(S, W, col, pal[0], pal[-1])]]
        sets += [[_filter(S, W, col, pal[2], pal[-3], fl)] for fl in (HI, LO, LO | HI)]
        sets += [[_filter(S, W, col, pal[0], pal[-1], HI)], [_filter(S, W, col, pal[1], pal[1], HI)]]
    for col in ("f32", "f64"):
        nan = float("nan")
        sets += [[_filter(S, W, col, -0.0, 1.0)], [_filter(S, W, col, -1.0, -0.0)], [_filter(S, W, col, -1.0, 0.0, HI)],
                 [_filter(S, W, col, 0.0, 0.0, HI)], [_filter(S, W, col, -0.0, np.inf, LO | HI)], [_filter(S, W, col, -np.inf, 0.0)],
                 [_filter(S, W, col, -np.inf, np.inf)], [_filter(S, W, col, nan, 1.0)], [_filter(S, W, col, -1.0, nan, HI)]]
    for col in ("nf32", "nf64"):  # NaN values pass nothing
        sets += [[_filter(S, W, col, -np.inf, np.inf, HI)], [_filter(S, W, col, -0.0, 0.0, HI)]]
    sets += [[_set(S, W, "s16", [0, 5, N_BUCKETS + 3, 65535, 70000])], [_set(S, W, "s32", [1, 0xFFFFFFFF, 1 << 20])],
             [_set(S, W, "s16", list(range(3, 60, 2)) + [65535])]]
    sets += [[_filter(S, W, "i64", -1, (1 << 63) - 1, HI), _filter(S, W, "u64", 1 << 63, (1 << 64) - 1, HI)]]
    sets += [[_filter(S, W, c, W.vals[c][1], W.vals[c][-1], HI) for c in ("u8", "u16", "u32", "u64", "i8", "i16", "i32", "i64")]]
    qs = W.queries
    qb = np.concatenate([W.sh.make_queries([t], qt, [neg]) for t, qt, _, neg in qs])
    try:
        for strat in (0, 1):
            W.sh.set_strategy(strat)
            for fs in sets:
                filt = [f for f, _ in fs]
                keep = np.logical_and.reduce([k for _, k in fs])
                for rt in (S.ResultType.TopkCount, S.ResultType.Count):
                    doc, score, cnt, tot = W.sh.search_lexical_batch(qb, 10, rt, reference_shortcuts=False, facet_filter=filt)
                    for i, (md, ms) in enumerate(W.matches):
                        kept = keep[md]
                        assert int(tot[i]) == int(kept.sum()), (filt, qs[i][0], strat, rt)
                        if rt != S.ResultType.Count:
                            _check_topk(doc[i], score[i], cnt[i], md[kept][:10], ms[kept][:10])
                            assert all(keep[int(d)] for d in doc[i][:cnt[i]]), (filt, qs[i][0])
    finally:
        W.sh.set_strategy(0)


def test_facet_counts_at_the_edges(S, W):
    """every numeric type: bounds that start at the type's minimum (nothing in "other"), a bound above every value, values exactly on
    bounds, one bound (all below it "other"), a 0.0 bound against stored -0.0; NaN counted as "other"; string ids at or above
    n_buckets as "other".  Every bucket, "other" and the total exact."""
    cases = []
    for col in NUMERIC:
        pal = [x for x in W.vals[col] if not (isinstance(x, float) and x == 0.0 and np.copysign(1.0, x) < 0)]  # strictly ascending
        nb = 8 * REC[col].itemsize
        above = [pal[-1] + 1] if col[0] != "f" and nb < 64 else []
        cases += [(col, [pal[0]] + pal[3::3] + above), (col, [pal[len(pal) // 2]]), (col, pal)]
    cases += [("f32", [-1.0, 0.0, 1.0]), ("f64", [-np.inf, 0.0]), ("nf32", [-np.inf, -0.0, 1.0]), ("nf64", [-1.0, 0.0, np.inf])]
    filt = _filter(S, W, "u16", W.vals["u16"][1], W.vals["u16"][-2])
    for qi in (1, 3, 4, 5):
        terms, qt, _, neg = W.queries[qi]
        q = W.sh.make_queries([terms], qt, [neg])
        md = W.matches[qi][0]
        for flt, keep in ((None, np.ones(N_DOCS, bool)), ([filt[0]], filt[1])):
            m = md[keep[md]]
            for col, bounds in cases:
                ty = COL_TYPE[col]
                counts, other, tot = W.sh.facet_count(q, W.off[col], ty, range_lower_bounds=bounds, facet_filter=flt)
                b = [naive.facet_bucket(x, bounds) for x in W.vals[col]]
                want = np.zeros(len(bounds) + 1, np.int64)
                np.add.at(want, [len(bounds) if x is None else x for x in np.array(b, object)[W.idx[col][m]]], 1)
                assert tot == len(m) and np.array_equal(counts, want[:-1]) and other == want[-1], (col, bounds, terms, flt is None)
            for col in ("s16", "s32"):
                counts, other, tot = W.sh.facet_count(q, W.off[col], COL_TYPE[col], n_buckets=N_BUCKETS, facet_filter=flt)
                ids = np.array(W.vals[col], np.int64)[W.idx[col][m]]
                want = np.bincount(np.minimum(ids, N_BUCKETS), minlength=N_BUCKETS + 1)
                assert tot == len(m) and np.array_equal(counts, want[:N_BUCKETS]) and other == want[N_BUCKETS], (col, terms)


def test_facet_pivot_at_the_edges(S, W):
    """Shard.facet_kth (ss_bm25_facet_kth: radix select of the k-th best value over the match set), every type, both directions, k
    = 1, at and after a group boundary, inside the +-0 group, matches, matches + 1: n_better and n_equal exact, the value equal to the
    reference's k-th, its bits the stored ones (+0.0 for the zeros' shared key)"""
    for qi in (1, 3, 4, 0):
        terms, qt, _, neg = W.queries[qi]
        q = W.sh.make_queries([terms], qt, [neg])
        md = W.matches[qi][0]
        for col in NUMERIC:
            ty = COL_TYPE[col]
            vals = value_of(W, col, md)
            for desc in (True, False):
                first = naive.kth(vals, 1, desc)
                ks = {1, first[2], first[2] + 1, len(md), len(md) + 1}
                if ty[0] == "f":
                    z = naive.kth([0.0], 1, desc)[0]
                    zk = [i for i in range(1, len(md) + 1, max(1, len(md) // 64)) if naive.kth(vals, i, desc)[0] == z]
                    ks |= set(zk[:1] + zk[len(zk) // 2:len(zk) // 2 + 1])
                for k in sorted(x for x in ks if x >= 1):
                    v, nb, ne = naive.kth(vals, k, desc)
                    bits, gb, ge, tot = W.sh.facet_kth(q, W.off[col], ty, desc, k)
                    assert tot == len(md), (col, terms)
                    assert (gb, ge) == (nb, ne), (col, terms, desc, k, (gb, ge), (nb, ne))
                    got = naive.facet_value(bits, ty)
                    assert got == v, (col, terms, desc, k, got, v)
                    assert bits == naive.facet_bits(0.0 if v == 0 and ty[0] == "f" else v, ty), (col, desc, k, hex(bits))


def test_facet_values_return_the_stored_bits(S, W):
    """ss_facet_values: the stored bits of every palette value unchanged -- sign of zero, NaN payloads, both 64-bit halves"""
    for col in NUMERIC + ["nf32", "nf64", "s16", "s32"]:
        docs = [int(np.nonzero(W.idx[col] == i)[0][0]) for i in range(len(W.vals[col])) if np.any(W.idx[col] == i)]
        docs += [N_DOCS, N_DOCS + 1, N_DOCS + N_EXTRA - 1]
        got = W.sh.facet_values(docs, W.off[col], COL_TYPE[col])
        want = W.rec[col][docs].view("<u%d" % REC[col].itemsize).astype(np.uint64)
        assert np.array_equal(got, want), col


# ------------------------------------------------------------------ result sorts
SORTS = [[("f32", True)], [("f32", False)], [("f64", True)], [("f64", False)], [("i8", False)], [("i64", True)], [("u32", False)],
         [("u64", True)], [("f64", False), ("i8", True)], [("u64", False), ("f32", True)],
         [("i8", True), ("f32", False), ("u64", True), ("i64", False)]]
SORT5 = [("f32", True), ("i8", False), ("f64", True), ("u32", True), ("i64", False)]  # more fields than the batched call takes


def _spec(W, srt):
    return [(W.off[c], COL_TYPE[c], d) for c, d in srt]


def _reference_order(W, md, ms, srt, keep=None):
    if keep is not None:
        md, ms = md[keep[md]], ms[keep[md]]
    order = naive.sorted_order(md, ms, [value_of(W, c, md) for c, _ in srt], [d for _, d in srt])
    return md[order], ms[order], md, ms


def check_sorted(W, doc, score, total, ref, srt, k, what):
    """count exactly min(k, matches), no duplicates, the sort fields position by position (+-0 equal), scores within REL of the
    reference's at every position and of the doc's own -- docs swap only inside groups where fields and scores tie"""
    od, os_, md, ms = ref
    n = min(k, len(od))
    doc = np.asarray(doc, np.int64)
    assert total == len(md), (what, total, len(md))
    assert len(doc) == n, (what, len(doc), n)
    assert len(set(doc.tolist())) == n, what
    for c, _ in srt:
        assert value_of(W, c, doc) == value_of(W, c, od[:n]), (what, c)
    assert np.allclose(score, os_[:n], rtol=REL), (what, np.nonzero(~np.isclose(score, os_[:n], rtol=REL))[0][:5])
    own = dict(zip(md.tolist(), ms.tolist()))
    assert all(d in own for d in doc.tolist()), what
    assert np.allclose(score, [own[d] for d in doc.tolist()], rtol=REL), what


def _tie_ks(W, ref, srt):
    """k at the edges of the first field's groups that straddle the middle of the answer: group size - 1, + 1 (and 1, 10, 1024)"""
    od = ref[0]
    vals = value_of(W, srt[0][0], od[:1100])
    ks = {1, 10, 1024}
    edges = [i for i in range(1, len(vals)) if vals[i] != vals[i - 1]]
    for e in edges[:3]:
        ks |= {e - 1, e + 1}
    return sorted(k for k in ks if k >= 1)


def test_result_sort_batched_and_composed_at_the_edges(S, W):
    """ss_bm25_search_sorted (the batched route) and the composed route (pivot + filtered searches) against the reference's order:
    1, 2 and 4 fields of i8 / i64 / u32 / u64 (above 2^63) / f32 / f64 (+-0, +-inf, subnormals), ascending and descending, 5 fields
    (composed), k at the edges of tie groups, 1 and 1024, with and without a facet filter"""
    flt = _filter(S, W, "i16", W.vals["i16"][1], W.vals["i16"][-2])
    for qi in (0, 1, 2, 3, 5):
        terms, qt, _, neg = W.queries[qi]
        q = W.sh.make_queries([terms], qt, [neg])
        md, ms = W.matches[qi]
        for srt in SORTS + [SORT5]:
            for f, keep in ((None, None), ([flt[0]], flt[1])):
                if f is not None and srt not in (SORTS[0], SORTS[-1], SORT5):
                    continue
                ref = _reference_order(W, md, ms, srt, keep)
                for k in _tie_ks(W, ref, srt):
                    what = (terms, srt, k, f is not None)
                    if len(srt) <= 4:
                        bd, bs, bc, bt = W.sh.search_lexical_sorted_batch(q, _spec(W, srt), k, facet_filter=f)
                        check_sorted(W, bd[0][:bc[0]], bs[0][:bc[0]], int(bt[0]), ref, srt, k, ("batched",) + what)
                        assert np.all(bd[0][bc[0]:] == 0xFFFFFFFF)
                    if k in (1, 10, 1024) or len(srt) == 5 or srt[0][0][0] == "f":
                        cd, cs, ct = W.sh.search_lexical_sorted_composed(q, _spec(W, srt), k, facet_filter=f)
                        check_sorted(W, cd, cs, ct, ref, srt, k, ("composed",) + what)


def test_result_sort_deep_pages_inside_a_zero_group(S, W):
    """deep pages sorted by facets (k = 1030, 2600: passes of SS_MAX_K) whose pass boundary falls inside the +-0 group of the first field"""
    inside = set()
    nonneg = _filter(S, W, "f32", -0.0, np.inf, HI)  # the zeros first under an ascending sort
    for qi, srt, f in ((2, [("f32", False)], None), (2, [("f64", True), ("i8", False)], None), (2, [("f32", False)], nonneg),
                       (3, [("f32", True), ("u32", False)], None)):
        terms, qt, _, neg = W.queries[qi]
        q = W.sh.make_queries([terms], qt, [neg])
        md, ms = W.matches[qi]
        ref = _reference_order(W, md, ms, srt, None if f is None else f[1])
        first = value_of(W, srt[0][0], ref[0][:2600])
        for k in (1030, 2600):
            inside |= {b for b in (1024, 2048) if b < min(k, len(first)) and first[b - 1] == 0.0 and first[b] == 0.0}
            doc, score, tot = W.sh.search_lexical_sorted(q, _spec(W, srt), k, facet_filter=None if f is None else [f[0]])
            check_sorted(W, doc, score, tot, ref, srt, k, ("deep", terms, srt, k, f is not None))
    assert inside == {1024, 2048}  # the world puts both pass boundaries inside a zero group


def test_result_sort_batch_of_70_queries(S, W):
    """one call for 70 queries (more than one 64-query chunk) that include queries with no match, one match and fewer than k"""
    idx = [i % len(W.queries) for i in range(70)]
    qb = np.concatenate([W.sh.make_queries([W.queries[i][0]], W.queries[i][1], [W.queries[i][3]]) for i in idx])
    for srt, k in (([("f32", True)], 25), ([("u64", False), ("f64", True)], 300)):
        bd, bs, bc, bt = W.sh.search_lexical_sorted_batch(qb, _spec(W, srt), k)
        refs = {}
        for row, i in enumerate(idx):
            if i not in refs:
                refs[i] = _reference_order(W, *W.matches[i], srt)
            check_sorted(W, bd[row][:bc[row]], bs[row][:bc[row]], int(bt[row]), refs[i], srt, k, ("batch", row, srt))


def test_index_two_shards_result_sort_at_the_edges(S, W):
    """Index.search with result_sort over two shards (the cross-shard merge by Shard._facet_order_key): against the reference's order of
    the union of the shards' matches, each scored with its own shard's statistics"""
    from oracle import oracle as O
    n_sh = 2
    parts = O.split_corpus(N_DOCS, W.dl, W.offs, W.docs, W.tfs, n_sh)
    raw = W.rec[:N_DOCS].view(np.uint8).reshape(N_DOCS, REC.itemsize)
    shards, oshards = [], []
    try:
        for sid, (nd, dl, o, d, t) in enumerate(parts):
            sh = S.Shard(0, shard_id=sid)
            sh.upload_lexical(nd, dl, o, d, t)
            sh.upload_facets(np.ascontiguousarray(raw[sid::n_sh]))
            shards.append(sh)
            oshards.append(O.Shard(nd, dl, o, d, t))
        idx = S.Index(shards)
        for qi in (1, 2, 5):
            terms, qt, op, neg = W.queries[qi]
            md, ms = [], []
            for sid, osh in enumerate(oshards):
                d, s_, _ = osh.search_exhaustive(terms, op, N_DOCS, neg)
                md.append(d.astype(np.int64) * n_sh + sid)
                ms.append(s_)
            md, ms = np.concatenate(md), np.concatenate(ms)
            for srt in ([("f32", True)], [("f64", False), ("i8", True)], [("i64", False), ("u64", True)]):
                ref = _reference_order(W, md, ms, srt)
                for off_, length in ((0, 10), (0, 1024), (5, 300)):
                    ro = idx.search(terms, None, qt, S.SearchMode.Lexical, off_, length, strict=True, not_terms=neg, result_sort=_spec(W, srt))
                    sub = (ref[0][off_:], ref[1][off_:], ref[2], ref[3])
                    doc = [r.doc_id for r in ro.results]
                    assert ro.result_count_total == len(md)
                    check_sorted(W, doc, [r.score for r in ro.results], len(md), sub, srt, min(length, max(len(md) - off_, 0)),
                                 ("index", terms, srt, off_, length))
    finally:
        for sh in shards:
            sh.close()
