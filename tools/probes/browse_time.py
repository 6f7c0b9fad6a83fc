"""The empty query at the C2 size (10 M docs, synthetic facet records): ss_docs_search, host clock around the whole call (Python caller
included), warm-up first, then CALLS calls one by one: the median and p10 .. p90 of the single calls.
  top-10 by doc id | the same under one numeric filter | top-10 sorted by one f32 field | top-10 with three query_facets
and, for orientation only, the same filter and the same sort on a one-term query (ss_bm25_search_filtered / ss_bm25_search_sorted).
Usage: python tools/probes/browse_time.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import seekstorm_amd as S
from oracle import oracle as O

N_DOCS, CALLS, WARM = 10_000_000, 200, 20
sh = S.Shard(0)
sh.synth_lexical(O.LEX_SEED, N_DOCS, O.term_thresholds(), O.len_table())
rng = np.random.default_rng(3)
rec = np.dtype([("date", "<u4"), ("cat", "u1"), ("price", "<f4"), ("brand", "<u2")])
v = np.zeros(N_DOCS, rec)
v["date"] = rng.integers(0, 1 << 31, N_DOCS); v["cat"] = rng.integers(0, 20, N_DOCS); v["price"] = rng.random(N_DOCS) * 1000
v["brand"] = np.minimum(rng.zipf(1.2, N_DOCS), 999)
sh.upload_facets(v.view(np.uint8).reshape(N_DOCS, rec.itemsize))
off = {n: rec.fields[n][1] for n in rec.names}
FILTER = [(off["price"], "f32", 10.0, 20.0)]  # 1 % of the docs
SORT = [(off["price"], "f32", False)]
FACETS = [
    {"field": "price", "offset": off["price"], "type": "f32", "ranges": [("r%d" % i, float(b)) for i, b in enumerate(range(0, 1000, 125))], "range_type": "within"},
    {"field": "cat", "offset": off["cat"], "type": "u8", "ranges": [("c%d" % i, i) for i in range(20)], "range_type": "within"},
    {"field": "brand", "offset": off["brand"], "type": "string16", "values": ["b%d" % i for i in range(1000)], "prefix": "", "length": 10},
]
one_term = sh.make_queries([[0]], S.QueryType.Union)


def timed(call):
    for _ in range(WARM):
        call()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


d, c, tot, _ = sh.search_docs(10)
assert c == 10 and tot == N_DOCS and d.tolist() == list(range(N_DOCS - 1, N_DOCS - 11, -1))
d, c, tot, _ = sh.search_docs(10, facet_filter=FILTER)
keep = np.nonzero((v["price"] >= np.float32(10.0)) & (v["price"] < np.float32(20.0)))[0]
assert tot == len(keep) and d.tolist() == keep[::-1][:10].tolist()
d, c, tot, _ = sh.search_docs(10, result_sort=SORT)
order = np.lexsort((-np.arange(N_DOCS), v["price"]))[:10]
assert d.tolist() == order.tolist(), (d, order)
print(f"image: {N_DOCS} docs, record {rec.itemsize} B, bitmap {N_DOCS // 8} B; us per call, median (p10 .. p90) of {CALLS} calls after {WARM}", flush=True)
legs = [
    ("docs top-10 by id", lambda: sh.search_docs(10)),
    ("docs top-10 by id, one f32 filter (1 %)", lambda: sh.search_docs(10, facet_filter=FILTER)),
    ("docs top-10 sorted by one f32 field", lambda: sh.search_docs(10, result_sort=SORT)),
    ("docs top-10 by id + three query_facets", lambda: sh.search_docs_raw(10, query_facets=FACETS)),
    ("docs page 10 000 deep by id (k = 10, skip = 10 000)", lambda: sh.search_docs(10, skip=10_000)),
    ("one-term query top-10, the same filter (orientation)", lambda: sh.search_lexical_batch(one_term, 10, facet_filter=FILTER, reference_shortcuts=False)),
    ("one-term query top-10, the same sort (orientation)", lambda: sh.search_lexical_sorted_batch(one_term, SORT, 10)),
]
for name, call in legs:
    m, lo, hi = timed(call)
    print(f"{name:58s} {m:9.1f} ({lo:.1f} .. {hi:.1f})", flush=True)
sh.close()
