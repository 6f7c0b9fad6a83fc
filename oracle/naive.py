"""Second, deliberately naive restatement (numpy float32) of the scoring rules.

TEST INFRASTRUCTURE ONLY.  It shares no code with ss_oracle.c: two independent restatements
agreeing is our substitute for the Rust binary that cannot be built here.
Citations are file:line under /root/reference/seekstorm/src.
"""
import numpy as np

K = np.float32(1.2)  # add_result.rs:20
B = np.float32(0.75)  # add_result.rs:21


def int_to_byte4(i):  # index.rs:4237-4251
    if i < 24:
        return i
    ii = i - 24
    nb = ii.bit_length()
    if nb < 4:
        return 24 + ii
    sh = nb - 4
    return 24 + (((ii >> sh) & 7) | ((sh + 1) << 3))


def byte4_to_int(b):  # index.rs:4255-4268
    if b < 24:
        return b
    i = b - 24
    bits, sh = i & 7, i >> 3
    return 24 + bits if sh == 0 else 24 + ((bits | 8) << (sh - 1))


DLC = np.array([byte4_to_int(b) for b in range(256)], np.uint32)  # index.rs:4271-4279


def component_cache(avgdl):  # commit.rs:321-325
    q = DLC.astype(np.float32) / np.float32(avgdl)
    return (K * (np.float32(1.0) - B + B * q)).astype(np.float32)


def avgdl(doclen_bytes):  # commit.rs:318-319
    s = int(DLC[doclen_bytes].astype(np.uint64).sum())
    return np.float32(s) / np.float32(len(doclen_bytes))


def idf(N, n):  # search.rs:3225-3230
    Nf, nf = np.float32(N), np.float32(n)
    return np.log(((Nf - nf + np.float32(0.5)) / (nf + np.float32(0.5))) + np.float32(1.0), dtype=np.float32)


def bm25_scores(n_docs, doclen_bytes, postings, op_and):
    """postings: list of (docs u32, tfs) per query term.  Returns (doc ids, scores) of all matches,
    scores summed in query-term order in float32 (add_result.rs:1435-1449)."""
    comp = component_cache(avgdl(doclen_bytes))
    sc = np.zeros(n_docs, np.float32)
    cnt = np.zeros(n_docs, np.int32)
    for docs, tfs in postings:
        i = idf(n_docs, len(docs))
        tf = tfs.astype(np.float32)
        c = comp[doclen_bytes[docs]]
        w = (i * ((tf * (K + np.float32(1.0))) / (tf + c))).astype(np.float32)
        sc[docs] = sc[docs] + w
        cnt[docs] += 1
    m = (cnt == len(postings)) if op_and else (cnt > 0)
    ids = np.nonzero(m)[0].astype(np.uint32)
    return ids, sc[ids]


def topk(ids, scores, k):
    """exact top-k by (score desc, id asc)"""
    order = np.lexsort((ids, -scores.astype(np.float64)))[:k]
    return ids[order], scores[order]


def cosine_topk(rows, q, k):
    s = (rows.astype(np.float32) @ q.astype(np.float32)).astype(np.float32)
    ids = np.arange(len(s), dtype=np.uint32)
    return topk(ids, s, k)


def rrf(lex_ids, vec_ids, length):  # search.rs:1962-2035 (k = 0.6, 0-based ranks)
    sc = {}
    for i, d in enumerate(lex_ids):
        sc[int(d)] = np.float32(1.0) / (np.float32(0.6) + np.float32(i))
    for i, d in enumerate(vec_ids):
        r = np.float32(1.0) / (np.float32(0.6) + np.float32(i))
        sc[int(d)] = np.float32(sc[int(d)] + r) if int(d) in sc else r
    items = sorted(sc.items(), key=lambda kv: (-float(kv[1]), kv[0]))[:length]
    return [d for d, _ in items], [s for _, s in items]


# ---- the cross-shard merge (search.rs:1875-2119), restated over the lists each shard returned
MODE_LEXICAL, MODE_VECTOR, MODE_HYBRID = 0, 1, 2  # SearchMode
SRC_LEXICAL, SRC_VECTOR, SRC_HYBRID = 0, 1, 2  # ResultSource
# scores at a merge's edges: -inf, negatives, the smallest normal and subnormal of either sign, both zeros (f32)
MERGE_PALETTE = np.array([-np.inf, -3.5, -1.0, -2.0 ** -126, -2.0 ** -149, -0.0, 0.0, 2.0 ** -149, 2.0 ** -126, 0.5, 1.0, 2.0],
                         np.float32)


def reference_sorted(scores):
    """f32 scores in the order the reference's stable sort leaves them: descending, -0.0 and +0.0 tied (either may come first)"""
    return np.array(sorted(np.asarray(scores, np.float32).tolist(), key=lambda x: -x), np.float32)


def merge_exact(mode, shard_lists, S, offset, length):
    """The last stage of every multi-shard and every hybrid search.  shard_lists[s] = (lex, vec) of shard s, each None or
    (local ids, f32 scores) or (local ids, f32 scores, result_count_total), a list as the shard returned it.
      global id = local * S + s (search.rs:1671); the lists of a mode are concatenated in shard order and stable-sorted by score
      descending (sorted() on Python floats: -0.0 and +0.0 tie, as partial_cmp has them; equal scores keep concatenation order);
      Lexical / Vector: that order is the answer.  Hybrid: RRF over the two sorted concatenations -- rank i (0-based, over the
      whole concatenation) weighs f32 1 / (0.6 + i); a lexical entry inserts (or overwrites) its doc, a vector entry adds to a
      doc already there (f32 lex + vec, source Hybrid) or inserts it (search.rs:1962-2035); then score descending, equal fused
      scores by doc ascending (the project's choice: the reference leaves them in hash order).
    Then offset and length (2098-2119).  -> (doc uint64, score float32, source uint8, total): total = the sum over the shards of
    the mode's totals, max(lexical, vector) per shard for Hybrid (1884-1921); None when a needed total was not given."""
    def concat(which):
        out = []
        for s, lists in enumerate(shard_lists):
            lst = lists[which]
            if lst is not None:
                out += [(int(d) * S + s, np.float32(x)) for d, x in zip(lst[0], lst[1])]
        return sorted(out, key=lambda e: -float(e[1]))

    def total(lst):
        return 0 if lst is None else (lst[2] if len(lst) > 2 else None)

    if mode == MODE_HYBRID:
        fused = {}
        for i, (d, _) in enumerate(concat(0)):
            fused[d] = (np.float32(1) / (np.float32(0.6) + np.float32(i)), SRC_LEXICAL)
        for i, (d, _) in enumerate(concat(1)):
            r = np.float32(1) / (np.float32(0.6) + np.float32(i))
            fused[d] = (np.float32(fused[d][0] + r), SRC_HYBRID) if d in fused else (r, SRC_VECTOR)
        res = sorted(((d, x, so) for d, (x, so) in fused.items()), key=lambda e: (-float(e[1]), e[0]))
        tots = [(total(lex), total(vec)) for lex, vec in shard_lists]
        tot = None if any(None in t for t in tots) else sum(max(t) for t in tots)
    else:
        which = 0 if mode == MODE_LEXICAL else 1
        src = SRC_LEXICAL if mode == MODE_LEXICAL else SRC_VECTOR
        res = [(d, x, src) for d, x in concat(which)]
        tots = [total(lists[which]) for lists in shard_lists]
        tot = None if None in tots else sum(tots)
    page = res[offset:offset + length]
    return (np.array([e[0] for e in page], np.uint64), np.array([e[1] for e in page], np.float32),
            np.array([e[2] for e in page], np.uint8), tot)


def bm25_exact(n_docs, doclen_bytes, postings, op_and, not_docs=(), deleted=(), n_idf=None):
    """Every match of a lexical query, scored as the crate rounds each term's factors -- f32 idf (search.rs:3225-3230), f32
    component cache (commit.rs:318-325), f32 tf (K + 1) / (tf + comp) (add_result.rs:1445-1447) -- and summed over the doc's
    terms in float64: the yardstick for kernels whose own rounding of the sum (or of the weight) differs from the crate's.
    postings: (docs, tfs) per query term; not_docs: doc arrays of the NOT terms (add_result.rs:3440-3497); deleted: tombstones;
    n_idf: the doc count of idf (default n_docs).  -> (doc ids ascending, float64 scores); len(ids) = result_count_total."""
    comp = component_cache(avgdl(doclen_bytes))
    N = n_docs if n_idf is None else n_idf
    sc = np.zeros(n_docs, np.float64)
    cnt = np.zeros(n_docs, np.int32)
    for docs, tfs in postings:
        docs = np.asarray(docs, np.int64)
        w_idf = np.float64(idf(N, len(docs)))
        tf = np.asarray(tfs).astype(np.float32)
        w = ((tf * (K + np.float32(1.0))) / (tf + comp[doclen_bytes[docs]])).astype(np.float32)
        sc[docs] += w_idf * w.astype(np.float64)
        cnt[docs] += 1
    m = (cnt == len(postings)) if op_and else (cnt > 0)
    for d in not_docs:
        m[np.asarray(d, np.int64)] = False
    if len(deleted):
        m[np.asarray(deleted, np.int64)] = False
    ids = np.nonzero(m)[0].astype(np.uint32)
    return ids, sc[ids]


def _bm25f_core(n_docs, doclen_fields, boost, entries, op_and, not_docs, deleted, field_filter):
    dlf = np.asarray(doclen_fields, np.uint8).reshape(-1, n_docs)
    n_fields = dlf.shape[0]
    b = np.ones(n_fields, np.float32) if boost is None else np.asarray(boost, np.float32)
    psum = int(DLC[dlf].astype(np.uint64).sum())  # positions_sum over ALL fields: one avgdl, one component cache
    comp = component_cache(np.float32(psum) / np.float32(n_docs))
    listed = np.zeros(n_fields, bool)
    listed[[int(f) for f in field_filter]] = True
    assert not listed.any() or op_and or len(entries) == 1, "field filter: intersections and single-term queries"
    sc = np.zeros(n_docs, np.float64)
    cnt = np.zeros(n_docs, np.int32)
    low = np.zeros(n_docs, bool)  # some term's tf in the LOWEST field that holds the doc is < 10
    for docs, fields, tfs in entries:
        docs, fields = np.asarray(docs, np.int64), np.asarray(fields, np.int64)
        assert np.all((docs[1:] > docs[:-1]) | ((docs[1:] == docs[:-1]) & (fields[1:] > fields[:-1]))), "entries sorted by (doc, field)"
        first = np.ones(len(docs), bool)
        first[1:] = docs[1:] != docs[:-1]
        w_idf = np.float64(idf(n_docs, int(first.sum())))  # the docs that hold the term in ANY field
        tf = np.asarray(tfs).astype(np.float32)
        w = ((tf * (K + np.float32(1.0))) / (tf + comp[dlf[fields, docs]])).astype(np.float32)
        np.add.at(sc, docs, b[fields].astype(np.float64) * w_idf * w.astype(np.float64))
        low[docs[first & (tf < np.float32(10.0))]] = True
        cnt[np.unique(docs[listed[fields]]) if listed.any() else docs[first]] += 1
    m = (cnt == len(entries)) if op_and else (cnt > 0)
    for d in not_docs:
        m[np.asarray(d, np.int64)] = False
    if len(deleted):
        m[np.asarray(deleted, np.int64)] = False
    return m, sc, low


def bm25f_exact(n_docs, doclen_fields, boost, entries, op_and, not_docs=(), deleted=(), field_filter=()):
    """bm25_exact over several indexed fields (BM25F, add_result.rs:1171-1426; ss_oracle.c fields_core restated): every match,
    score = sum over the query's (term, field) entries of the doc of  boost[f] * idf * tf (K + 1) / (tf + comp[len byte(doc, f)])
    -- f32 boost, f32 idf from the docs that hold the term in ANY field, f32 weight under the ONE component cache of the avgdl over
    all fields (commit.rs:318-325), their product and the sum in float64.  An intersection asks for every term in some field.
    doclen_fields: [n_fields][n_docs] length bytes; boost: [n_fields] or None (all 1); entries: (docs, fields, tfs) per query term,
    sorted by (doc, field); not_docs: doc arrays of the NOT terms (any field); deleted: tombstones; field_filter: field ids -- a doc
    is dropped unless EVERY term it is matched on stands in a listed field, the score still sums all fields (add_result.rs:3124-3136;
    intersections and single terms).  -> (doc ids ascending, float64 scores); len(ids) = result_count_total."""
    m, sc, _ = _bm25f_core(n_docs, doclen_fields, boost, entries, op_and, not_docs, deleted, field_filter)
    ids = np.nonzero(m)[0].astype(np.uint32)
    return ids, sc[ids]


def bm25f_shortcut_exact(n_docs, doclen_fields, boost, entries, deleted=()):
    """An intersection under all_terms_frequent over several indexed fields (add_result.rs:1595-1607, 3111-3122; ss_oracle.c
    so_search_fields_shortcut): every match is counted, a doc is RANKED only if for every term the tf in the lowest field that holds
    the doc is >= 10.  No NOT terms, no field filter (3116).  -> (ranked doc ids ascending, their float64 scores, result_count_total)"""
    m, sc, low = _bm25f_core(n_docs, doclen_fields, boost, entries, True, (), deleted, ())
    ids = np.nonzero(m & ~low)[0].astype(np.uint32)
    return ids, sc[ids], int(m.sum())


def topk_exact(ids, scores, k):
    """top-k of bm25_exact's answer by (score desc, doc asc)"""
    order = np.lexsort((ids, -np.asarray(scores, np.float64)))[:k]
    return ids[order], np.asarray(scores, np.float64)[order]


# ---- facets: filter (add_result.rs:341-482), counts (add_result.rs:484-640) and result sort (min_heap.rs:574-1050), read as
# plain values -- Python ints for the integer types, Python floats for F32 / F64 -- with no key transform of any kind
FACET_HI_INCLUSIVE, FACET_LO_EXCLUSIVE = 1, 2  # ss_facet_filter.reserved (seekstorm_hip.h)
FACET_NP = {"u8": "<u1", "u16": "<u2", "u32": "<u4", "u64": "<u8", "i8": "<i1", "i16": "<i2", "i32": "<i4", "i64": "<i8",
            "f32": "<f4", "f64": "<f8"}


def facet_value(bits, ty):
    """stored bits (zero-extended) -> the value they hold"""
    dt = np.dtype(FACET_NP[ty])
    x = np.array([int(bits) & ((1 << (8 * dt.itemsize)) - 1)], "<u%d" % dt.itemsize).view(dt)[0]
    return float(x) if ty[0] == "f" else int(x)


def facet_bits(value, ty):
    """a value of the type -> its stored bits (zero-extended)"""
    dt = np.dtype(FACET_NP[ty])
    return int(np.array([value], dt).view("<u%d" % dt.itemsize)[0])


def facet_pass(value, ty, lo, hi, flags=0):
    """Rust's Range::contains, lo <= value < hi; FACET_LO_EXCLUSIVE / FACET_HI_INCLUSIVE turn the ends around.  NaN (a value or
    an end) passes nothing; -0.0 == +0.0."""
    if ty[0] == "f" and (np.isnan(value) or np.isnan(lo) or np.isnan(hi)):
        return False
    above = value > lo if flags & FACET_LO_EXCLUSIVE else value >= lo
    below = value <= hi if flags & FACET_HI_INCLUSIVE else value < hi
    return bool(above and below)


def facet_bucket(value, bounds):
    """the range a numeric facet value is counted in: index of the last lower bound <= value (binary_search_by_key, add_result.rs:484-640);
    None ("other") below the first bound and for NaN.  bounds strictly ascending."""
    assert all(a < b for a, b in zip(bounds, bounds[1:])), "bounds must be strictly ascending"
    if isinstance(value, float) and np.isnan(value):
        return None
    b = None
    for i, x in enumerate(bounds):
        if x <= value:
            b = i
    return b


def _sort_key(value, descending):
    assert not (isinstance(value, float) and np.isnan(value)), "NaN has no order under a result sort"
    if isinstance(value, float) and value == 0.0:
        value = 0.0  # partial_cmp: -0.0 == +0.0
    return -value if descending else value


def sorted_order(docs, scores, columns, directions):
    """indices of docs in result-sort order: the fields (columns[f][i] the value of doc i, directions[f] True = descending), then
    score descending, then doc ascending -- the total order the header promises for deep pages"""
    return sorted(range(len(docs)), key=lambda i: tuple(_sort_key(c[i], d) for c, d in zip(columns, directions))
                  + (-float(scores[i]), int(docs[i])))


def kth(values, k, descending):
    """the pivot of a result sort: (k-th best value, number strictly better, number equal to it); k beyond the values: the worst.
    Equality as the reference's partial_cmp (-0.0 == +0.0).  No values: (None, 0, 0)."""
    if not values:
        return None, 0, 0
    keys = sorted(_sort_key(x, descending) for x in values)
    p = keys[min(k, len(keys)) - 1]
    v = next(x for x in values if _sort_key(x, descending) == p)
    return v, sum(1 for x in keys if x < p), sum(1 for x in keys if x == p)


def facet_palette(ty):
    """every type's edge values: min / max and their neighbours, -1 / 0 / 1, the middle of an unsigned type, pairs that differ only
    in the lowest or only in the top byte (each radix pass of the pivot select decides something); for floats +-inf, +-max, +-1,
    the smallest normals and subnormals and both zeros.  NaN is left to facet_nan_palette."""
    if ty[0] == "f":
        fi = np.finfo(np.float32 if ty == "f32" else np.float64)
        dt = fi.dtype.type
        sub = float(np.nextafter(dt(0), dt(1)))
        one_ulp = float(np.nextafter(dt(1), dt(2)))
        return [-np.inf, -float(fi.max), -1.0, -float(fi.tiny), -sub, -0.0, 0.0, sub, float(fi.tiny), 1.0, one_ulp, float(fi.max), np.inf]
    nb = 8 * np.dtype(FACET_NP[ty]).itemsize
    if ty[0] == "u":
        lo, hi = 0, (1 << nb) - 1
        vals = [lo, lo + 1, hi - 1, hi, (1 << (nb - 1)) - 1, 1 << (nb - 1), (1 << (nb - 1)) + 1]
    else:
        lo, hi = -(1 << (nb - 1)), (1 << (nb - 1)) - 1
        vals = [lo, lo + 1, -1, 0, 1, hi - 1, hi]
    if nb > 8:
        base = int.from_bytes(bytes([0x35]) + bytes([0xA5] * (nb // 8 - 1)), "big")  # positive in every width
        vals += [base, base + 1, base + (1 << (nb - 8))]  # lowest byte; top byte
        if ty[0] == "i":
            vals += [-base, -base - 1, -base - (1 << (nb - 8))]
        else:
            vals += [base | (1 << (nb - 1)), (base | (1 << (nb - 1))) + 1]  # above 2^(b-1)
    return sorted(set(vals))


def facet_nan_palette(ty):
    """NaN bit patterns of a float type: quiet, negative with a payload, signalling"""
    return [0x7FC00000, 0xFFC00001, 0x7F800001] if ty == "f32" else [0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001]


# ---- dense vectors: exact values (float64 from the f32 inputs) and the rounding band of any f32 summation order
U_F32 = 2.0 ** -24  # unit roundoff of f32


def gamma(n):
    """gamma(n) = n u / (1 - n u), u = 2^-24: the relative error bound of n rounded f32 operations in a row (Higham, Accuracy and
    Stability of Numerical Algorithms, 3.1) -- any summation order, fma included"""
    return n * U_F32 / (1.0 - n * U_F32)


def vec_exact_dot(rows, q):
    """x . q of every row in float64: the products of two f32 values are exact, the f64 sum is ~2^-29 of the f32 band below"""
    r = np.asarray(rows, np.float32).astype(np.float64).reshape(-1, np.asarray(q).size)
    return r @ np.asarray(q, np.float32).astype(np.float64).ravel()


def vec_exact_l2(rows, q):
    """|q - x|^2 of every row in float64 (the difference of two f32 values of like magnitude is exact in f64)"""
    r = np.asarray(rows, np.float32).astype(np.float64).reshape(-1, np.asarray(q).size)
    d = np.asarray(q, np.float32).astype(np.float64).ravel()[None, :] - r
    return np.einsum("ij,ij->i", d, d)


def bound_dot(rows, q):
    """how far an f32 dot product of any order may fall from vec_exact_dot: gamma(dim + 1) sum |x_i q_i|"""
    r = np.abs(np.asarray(rows, np.float32).astype(np.float64).reshape(-1, np.asarray(q).size))
    return gamma(r.shape[1] + 1) * (r @ np.abs(np.asarray(q, np.float32).astype(np.float64).ravel()))


def bound_l2(rows, q, d2=None):
    """how far the reference's squared distance (sub, mul, add each rounded: euclidean_f32[_avx2]) may fall from vec_exact_l2:
    gamma(dim + 2) d^2 -- relative to the distance itself, since every term is >= 0"""
    dim = np.asarray(q).size
    return gamma(dim + 2) * (vec_exact_l2(rows, q) if d2 is None else np.asarray(d2, np.float64))


def check_vector_topk(doc, score, cnt, exact, bound, k, row_doc=None, tie_order=True):
    """A vector top-k (doc ids, f32 scores, count) against the exact similarity of every row (-inf: the row may not be returned --
    tombstoned, filtered, below the threshold, in a cluster the mode skips) and each row's rounding band `bound`.  With row_doc
    (several records per doc) a doc's exact value is the best of its rows', its band the widest.  Asserts:
      1. every returned score is within its doc's band of the exact value;
      2. the scores are non-increasing;
      3. every doc whose exact value beats the exact k-th by more than band(doc) + band(k-th) is returned;
      4. no returned doc falls below the exact k-th by more than that band;
      5. among equal scores the docs come in ascending order (tie_order; the reference's own lists keep its TopK slots' order,
         vector.rs:1472);
      6. the count is min(k, live docs), every doc at most once."""
    exact = np.asarray(exact, np.float64).ravel()
    bound = np.broadcast_to(np.asarray(bound, np.float64), exact.shape)
    if row_doc is not None:
        ids, inv = np.unique(np.asarray(row_doc, np.int64), return_inverse=True)
        ex = np.full(len(ids), -np.inf)
        np.maximum.at(ex, inv, exact)
        bd = np.zeros(len(ids))
        np.maximum.at(bd, inv, np.where(np.isfinite(exact), bound, 0.0))
    else:
        ids, ex, bd = np.arange(len(exact), dtype=np.int64), exact, np.asarray(bound)
    live = np.isfinite(ex)
    n = int(cnt)
    want = min(int(k), int(live.sum()))
    assert n == want, "count %d, want min(k=%d, live=%d) = %d" % (n, k, int(live.sum()), want)
    if n == 0:
        return
    d = np.asarray(doc[:n], np.int64)
    s = np.asarray(score[:n], np.float32).astype(np.float64)
    assert len(np.unique(d)) == n, "a doc returned twice"
    pos = np.searchsorted(ids, d)
    assert np.all(pos < len(ids)) and np.all(ids[np.minimum(pos, len(ids) - 1)] == d), "unknown doc returned"
    for j in np.nonzero(~live[pos])[0]:
        raise AssertionError("position %d: doc %d may not be returned" % (j, d[j]))
    tiny = 1e-300  # (bands are 0 for exact scores)
    err = np.abs(s - ex[pos])
    for j in np.nonzero(err > bd[pos] + tiny)[0][:3]:
        raise AssertionError("position %d: doc %d scored %.9g, exact %.17g, off by %.3g > band %.3g" % (j, d[j], s[j], ex[pos[j]], err[j], bd[pos[j]]))
    for j in np.nonzero(np.diff(s) > 0)[0][:3]:
        raise AssertionError("scores rise at position %d: %.9g -> %.9g" % (j, s[j], s[j + 1]))
    for j in np.nonzero((np.diff(s) == 0) & (np.diff(d) < 0) & tie_order)[0][:3]:
        raise AssertionError("equal scores %.9g at positions %d, %d: docs %d before %d" % (s[j], j, j + 1, d[j], d[j + 1]))
    li = np.nonzero(live)[0]
    o = li[np.lexsort((ids[li], -ex[li]))]
    kth, kb = ex[o[want - 1]], bd[o[want - 1]]
    got = set(d.tolist())
    must = np.nonzero(live & (ex > kth + bd + kb))[0]
    miss = [int(i) for i in must if int(ids[i]) not in got]
    if miss:
        i = miss[0]
        worst = int(np.argmin(ex[pos]))
        raise AssertionError("%d docs missing: doc %d with exact %.17g (k-th %.17g, band %.3g) not returned; worst returned doc %d at %.17g"
                             % (len(miss), ids[i], ex[i], kth, bd[i] + kb, d[worst], ex[pos[worst]]))
    low = np.nonzero(ex[pos] < kth - bd[pos] - kb)[0]
    for j in low[:1]:
        raise AssertionError("%d returned docs beyond the band: doc %d at exact %.17g, k-th %.17g" % (len(low), d[j], ex[pos[j]], kth))


def vec_offcentre(seed, n, dim, c, sigma):
    """f32 rows c * u + sigma * N(0, 1) around one centre of norm c (u: a unit vector of positive components, the same for every
    seed of a dim): all-positive embeddings, a shared mean component -- the data on which 2 q.x - |x|^2 - |q|^2 cancels"""
    u = np.random.default_rng(dim).random(dim) + 0.5
    u /= np.linalg.norm(u)
    rng = np.random.default_rng(seed)
    return (c * u[None, :] + sigma * rng.standard_normal((n, dim))).astype(np.float32)


# ---- Point (geo) facets: geo_search.rs, in numpy float64, every operation in the reference's order.  numpy's add, subtract, multiply,
# divide and sqrt are correctly rounded IEEE operations; cos is the one routine that may differ from another libm in the last place.
GEO_EARTH_KM = 6371.0087714  # geo_search.rs:109
GEO_EARTH_MI = 3_958.761_315_801_475  # geo_search.rs:110
GEO_DEG2RAD = 0.017_453_292_519_943_295  # geo_search.rs:111
_GEO_SCALE = 10_000_000.0


def _geo_as_i32(v):
    """Rust's `f64 as i32`: toward zero, saturating at the type's ends, NaN -> 0 (int64 holding the i32 values)"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return np.trunc(np.where(v != v, 0.0, np.clip(v, -2147483648.0, 2147483647.0))).astype(np.int64)


def _geo_spread(x):  # encode_morton_64_bit, geo_search.rs:12-21
    x = x.astype(np.uint64)
    for sh, mask in ((16, 0x0000FFFF0000FFFF), (8, 0x00FF00FF00FF00FF), (4, 0x0F0F0F0F0F0F0F0F), (2, 0x3333333333333333),
                     (1, 0x5555555555555555)):  # (the first line, x | x << 32 under the low mask, leaves a u32 as it is)
        x = (x | (x << np.uint64(sh))) & np.uint64(mask)
    return x


def geo_encode(lat, lon):
    """encode_morton_2_d (geo_search.rs:27-41): lat x 1e7 as i32 as u32 in the even bits, lon in the odd ones -> uint64 codes"""
    with np.errstate(all="ignore"):
        x = _geo_as_i32(np.asarray(lat, np.float64) * _GEO_SCALE) & 0xFFFFFFFF
        y = _geo_as_i32(np.asarray(lon, np.float64) * _GEO_SCALE) & 0xFFFFFFFF
    return (_geo_spread(np.atleast_1d(y)) << np.uint64(1)) | _geo_spread(np.atleast_1d(x))


def _geo_squeeze(x):  # decode_morton_64_bit, geo_search.rs:45-53
    x = x & np.uint64(0x5555555555555555)
    for sh, mask in ((1, 0x3333333333333333), (2, 0x0F0F0F0F0F0F0F0F), (4, 0x00FF00FF00FF00FF), (8, 0x0000FFFF0000FFFF),
                     (16, 0x00000000FFFFFFFF)):
        x = (x ^ (x >> np.uint64(sh))) & np.uint64(mask)
    return x.astype(np.uint32)


def geo_decode(codes):
    """decode_morton_2_d (geo_search.rs:58-79): codes -> (lat, lon), each (u32 as i32) as f64 / 1e7"""
    c = np.atleast_1d(np.asarray(codes, np.uint64))
    lat = _geo_squeeze(c).view(np.int32).astype(np.float64) / _GEO_SCALE
    lon = _geo_squeeze(c >> np.uint64(1)).view(np.int32).astype(np.float64) / _GEO_SCALE
    return lat, lon


def geo_distance(codes, base, unit):
    """unit "km" | "miles": euclidian_distance(point1 = base, point2 = doc) (geo_search.rs:115-124, called so at add_result.rs:462-478
    and 605-618); "sortkey": simplified_distance(point1 = doc, point2 = base) (geo_search.rs:82-87 under morton_ordering, 96-100)"""
    lat, lon = geo_decode(codes)
    b0, b1 = np.float64(base[0]), np.float64(base[1])
    with np.errstate(all="ignore"):
        if unit == "sortkey":
            x = (b1 - lon) * np.cos(GEO_DEG2RAD * (lat + b0) / 2.0)
            y = b0 - lat
            return x * x + y * y
        r = {"km": GEO_EARTH_KM, "miles": GEO_EARTH_MI}[unit]
        x = GEO_DEG2RAD * (lon - b1) * np.cos(GEO_DEG2RAD * (b0 + lat) / 2.0)
        y = GEO_DEG2RAD * (lat - b0)
        return r * np.sqrt(x * x + y * y)


def geo_morton_range(base, distance, unit):
    """point_distance_to_morton_range (geo_search.rs:128-144) -> (morton_min, morton_max), the ends of a Range<u64>"""
    r = np.float64({"km": GEO_EARTH_KM, "miles": GEO_EARTH_MI}[unit])
    b0, b1, d = np.float64(base[0]), np.float64(base[1]), np.float64(distance)
    with np.errstate(all="ignore"):
        lat_delta = d / (GEO_DEG2RAD * r)
        lon_delta = d / (GEO_DEG2RAD * r * np.cos(GEO_DEG2RAD * b0))
        return int(geo_encode(b0 - lat_delta, b1 - lon_delta)[0]), int(geo_encode(b0 + lat_delta, b1 + lon_delta)[0])


def geo_pass(codes, base, lo, hi, unit, flags=0):
    """FilterSparse::Point (add_result.rs:462-478): the code inside the Z-order range of (base, hi) -- an unsigned Range<u64>, empty when
    its ends are out of order -- AND the distance inside [lo, hi).  Under "sortkey" (the pivots of a sort by distance: no reference
    filter has that unit) there is no Z range, and the flags turn the ends around as in facet_pass.  -> bool per code"""
    c = np.atleast_1d(np.asarray(codes, np.uint64))
    d = geo_distance(c, base, unit)
    above = d > lo if flags & FACET_LO_EXCLUSIVE else d >= lo
    below = d <= hi if flags & FACET_HI_INCLUSIVE else d < hi
    keep = above & below
    if unit != "sortkey":
        m0, m1 = geo_morton_range(base, hi, unit)
        keep &= (c >= np.uint64(m0)) & (c < np.uint64(m1))
    return keep
