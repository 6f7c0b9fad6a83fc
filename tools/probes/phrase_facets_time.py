"""What a phrase costs the entries that walk match sets (csrc/bm25_phrase_bits.hip), on the 150 000-doc corpus of
tests/test_gpu_phrase.py::test_phrase_queries_match_oracle, 64 queries per call, k = 10, TopkCount, one String16 facet of 256 buckets:
  phrases:        ONE ss_bm25_search_facets call of 64 two-word phrases (every ordered pair of the six terms, cycled);
  intersections:  the same call for the 64 intersections of the same words -- what the phrase call does before it refines;
  count search:   ss_bm25_search, ResultType Count, of the 64 phrases -- the ranking kernels' own position check over the same docs.
The last two run on a build without the refine kernel as well: they are the yardsticks.  Host clock around the whole call through the
Python mirror, WARM calls first, then CALLS calls: the median and the p10 .. p90 spread.
Usage: python tools/probes/phrase_facets_time.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seekstorm_amd as S
from oracle import oracle as O
from test_gpu_phrase import _corpus

WARM, CALLS = 20, 200
n_docs = 150_000
dfs = [30_000, 22_000, 40_000, 9_000, 15_000, 500]
plant = [([0, 1], 400), ([0, 1, 2], 150), ([2, 0, 2], 120), ([3, 4], 60), ([0, 1, 2, 3, 4, 5], 30), ([1, 1], 80), ([4, 0, 1], 70)]
dl, offs, docs, tfs, positions = _corpus(O, n_docs, dfs, 5, plant)
sh = S.Shard(0)
sh.upload_lexical(n_docs, dl, offs, docs, tfs, positions)
rng = np.random.default_rng(3)
brand = rng.integers(0, 300, n_docs).astype("<u2")
sh.upload_facets(np.ascontiguousarray(brand.view(np.uint8).reshape(n_docs, 2)))
facets = [{"field": "brand", "offset": 0, "type": "string16", "values": ["b%d" % i for i in range(256)], "prefix": "", "length": 10}]
pairs = [[a, b] for a in range(6) for b in range(6) if a != b]
words = [pairs[i % len(pairs)] for i in range(64)]
qp = sh.make_queries(words, S.QueryType.Phrase)
qi = sh.make_queries(words, S.QueryType.Intersection)


def timed(call):
    for _ in range(WARM):
        call()
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


legs = [("intersections, search_facets", lambda: sh.search_lexical_facets(qi, 10, facets, S.ResultType.TopkCount, reference_shortcuts=False)),
        ("phrases, Count search", lambda: sh.search_lexical_batch(qp, 10, S.ResultType.Count))]
try:
    sh.search_lexical_facets(qp, 10, facets, S.ResultType.TopkCount, reference_shortcuts=False)
    legs.insert(0, ("phrases, search_facets", lambda: sh.search_lexical_facets(qp, 10, facets, S.ResultType.TopkCount, reference_shortcuts=False)))
except S.SeekStormHipError as e:
    print("phrases, search_facets: refused by this build (code %d)" % e.code)
ti = sh.search_lexical_facets(qi, 10, facets, S.ResultType.TopkCount, reference_shortcuts=False)[3]
tp = sh.search_lexical_batch(qp, 10, S.ResultType.Count)[3]
print(f"{n_docs} docs, 64 queries per call, k = 10; candidates (intersection matches) per query: mean {float(ti.mean()):.0f}, max {int(ti.max())}; "
      f"phrase matches: mean {float(tp.mean()):.0f}, max {int(tp.max())}")
print(f"us per call, median (p10 .. p90) of {CALLS} calls after {WARM}")
res = {}
for name, call in legs:
    res[name] = timed(call)
    print(f"{name:32s} {res[name][0]:9.1f} ({res[name][1]:.1f} .. {res[name][2]:.1f})", flush=True)
if "phrases, search_facets" in res:
    both = res["intersections, search_facets"][0] + res["phrases, Count search"][0]
    print(f"phrases / (intersections + Count search) = {res['phrases, search_facets'][0] / both:.2f}")
sh.close()
