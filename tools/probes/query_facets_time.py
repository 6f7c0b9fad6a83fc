"""A search page with its query_facets at the C2 size (10 M docs, synthetic facet records, 3-term OR queries, TopkCount, k = 10):
  route a: per query one ss_bm25_search_filtered + F calls of ss_bm25_facet_count -- the only route before ss_bm25_search_facets existed;
           this part uses only entries of that time, so the script runs on an older build as well (it then stops after route a);
  route b: ONE ss_bm25_search_facets call for the batch and all its facets.
(nq, F) in {(1, 1), (1, 4), (64, 4)}; host clock around the whole route, warm-up first, REPS repeats of CALLS rounds each: the median
and the min .. max spread of the repeats.  Answers of the two routes are compared once per shape.
Usage: python tools/probes/query_facets_time.py [a|b|ab]   (rocprofv3 --kernel-trace --stats -- python ... b for the kernel's own time)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import seekstorm_amd as S
from oracle import oracle as O
import bench

MODE = sys.argv[1] if len(sys.argv) > 1 else "ab"
N_DOCS, REPS = 10_000_000, 5
sh = S.Shard(0)
sh.synth_lexical(O.LEX_SEED, N_DOCS, O.term_thresholds(), O.len_table())
rng = np.random.default_rng(3)
rec = np.dtype([("date", "<u4"), ("cat", "u1"), ("price", "<f4"), ("brand", "<u2")])
v = np.zeros(N_DOCS, rec)
v["date"] = rng.integers(0, 1 << 31, N_DOCS); v["cat"] = rng.integers(0, 20, N_DOCS); v["price"] = rng.random(N_DOCS) * 1000
v["brand"] = np.minimum(rng.zipf(1.2, N_DOCS), 999)
sh.upload_facets(v.view(np.uint8).reshape(N_DOCS, rec.itemsize))
off = {n: rec.fields[n][1] for n in rec.names}
FACETS = [
    {"field": "price", "offset": off["price"], "type": "f32", "ranges": [("r%d" % i, float(b)) for i, b in enumerate(range(0, 1000, 125))], "range_type": "within"},
    {"field": "cat", "offset": off["cat"], "type": "u8", "ranges": [("c%d" % i, i) for i in range(20)], "range_type": "within"},
    {"field": "date", "offset": off["date"], "type": "u32", "ranges": [("d%d" % i, i << 27) for i in range(16)], "range_type": "within"},
    {"field": "brand", "offset": off["brand"], "type": "string16", "values": ["b%d" % i for i in range(1000)], "prefix": "", "length": 10},
]
queries = sh.make_queries(bench.make_c2_queries(O, 64)[0], S.QueryType.Union)
have_b = hasattr(sh, "search_lexical_facets")


def route_a(q, facets):
    out = []
    for i in range(len(q)):
        hits = sh.search_lexical_batch(q[i:i + 1], 10, S.ResultType.TopkCount, reference_shortcuts=False)
        cs = []
        for qf in facets:
            if qf["type"].startswith("string"):
                c, other, _ = sh.facet_count(q[i:i + 1], qf["offset"], qf["type"], n_buckets=len(qf["values"]))
            else:
                c, other, _ = sh.facet_count(q[i:i + 1], qf["offset"], qf["type"], range_lower_bounds=[b for _, b in qf["ranges"]])
            cs.append(np.append(c, other))
        out.append((hits, cs))
    return out


def route_b(q, facets):
    return sh.search_lexical_facets(q, 10, facets, S.ResultType.TopkCount, reference_shortcuts=False)


def timed(call, rounds):
    for _ in range(3):
        call()
    reps = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(rounds):
            call()
        reps.append((time.perf_counter() - t0) / rounds * 1e6)
    return float(np.median(reps)), min(reps), max(reps)


rec_bytes = rec.itemsize
print(f"image: {N_DOCS} docs, record {rec_bytes} B, bitmap {N_DOCS // 8} B per query; us per route, median (min .. max) of {REPS} repeats", flush=True)
for nq, F in ((1, 1), (1, 4), (64, 4)):
    q, facets = queries[:nq], FACETS[:F]
    rounds = 50 if nq == 1 else 5
    line = f"nq {nq:2d} F {F}: "
    a = b = None
    if "a" in MODE:
        a = timed(lambda: route_a(q, facets), rounds)
        line += f"a {a[0]:9.1f} ({a[1]:.1f} .. {a[2]:.1f})  "
    if "b" in MODE and have_b:
        b = timed(lambda: route_b(q, facets), rounds)
        line += f"b {b[0]:9.1f} ({b[1]:.1f} .. {b[2]:.1f})  "
        ra, rb = route_a(q, facets), route_b(q, facets)
        same = all(np.array_equal(ra[i][0][0][0], rb[0][i]) and int(ra[i][0][3][0]) == int(rb[3][i]) and
                   all(np.array_equal(ra[i][1][f], rb[4][f][i]) for f in range(F)) for i in range(nq))
        matches = float(rb[3].mean())
        line += f"same answers {same}; mean matches {matches:.0f}: bitmap + record bytes {nq * (N_DOCS // 8) + nq * matches * rec_bytes:.3g} B  "
    if a and b:
        line += f"a / b = {a[0] / b[0]:.2f}"
    print(line, flush=True)
sh.close()
