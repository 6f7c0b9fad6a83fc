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
