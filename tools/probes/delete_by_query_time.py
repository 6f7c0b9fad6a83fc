"""delete_documents_by_query at the benchmark size (10 M docs, ss_bm25_synth): the new call against the route a host had before it.
Two shapes of one benchmark query (bench.make_c2_queries): the 2-term AND of its two longer lists (tens of thousands of matches) and
its 3-term OR (about 1.3 M).  Sides, alternated inside every round, host clock around calls that end synchronised, set_deleted([])
between them outside the timed window:
  a   Shard.delete_by_query, the whole match set, without the ids / with the ids
  b   the earlier route: search_lexical_batch with k = the matches (deep pages of 1024), then add_deleted of the returned ids; for the
      OR shape ONE round under a stated time limit ("over the limit" is recorded, nothing is extrapolated)
  c   a floor: a facet count of the same query (the same match-set build) plus add_deleted of one doc
Writes the medians with min and max (ms) as JSON.  Usage: python tools/probes/delete_by_query_time.py [--out FILE] [--rounds N]"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import seekstorm_amd as S
from oracle import oracle as O
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delete_by_query_time.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--limit", type=float, default=120.0, help="seconds the one round of side b on the OR shape may take")
args = ap.parse_args()

N_DOCS = 10_000_000
sh = S.Shard(0)
sh.synth_lexical(O.LEX_SEED, N_DOCS, O.term_thresholds(), O.len_table())
cat = np.random.default_rng(3).integers(0, 20, N_DOCS).astype(np.uint8)
sh.upload_facets(cat.reshape(N_DOCS, 1))
# of the benchmark's first 64 queries the one whose union is expected closest to 1.31 M docs, the batch's mean (README.md)
cands, th = bench.make_c2_queries(O, 64)
union_of = lambda tl: 1.0 - float(np.prod([1.0 - th[t] / 2.0 ** 32 for t in tl]))
terms = min(cands, key=lambda tl: abs(union_of(tl) - 0.131))
shapes = {"and2": sh.make_queries([terms[1:]], S.QueryType.Intersection), "or3": sh.make_queries([terms], S.QueryType.Union)}


def clock(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def route_b(q, k):
    doc, _, cnt, _ = sh.search_lexical_batch(q, k, S.ResultType.Topk, reference_shortcuts=False)
    sh.add_deleted(doc[0][:int(cnt[0])])
    return int(cnt[0])


def floor_c(q):
    sh.facet_count(q, 0, "u8", range_lower_bounds=[0, 5, 10, 15])
    sh.add_deleted([7])


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "rounds": len(ms)}


result = {"n_docs": N_DOCS, "terms": [int(t) for t in terms], "protocol": "host clock, sides alternated inside each round, set_deleted([]) between them untimed",
          "shapes": {}}
for name, q in shapes.items():
    sh.set_deleted([])
    matched = int(sh.delete_by_query(q, dry_run=True)[0][0])
    b_rounds = args.rounds if name == "and2" else 1
    for _ in range(2):  # warm-up: workspaces grown, probe rows placed
        sh.set_deleted([]); sh.delete_by_query(q, return_docs=True)
        sh.set_deleted([]); floor_c(q)
    t = {"a_without_ids": [], "a_with_ids": [], "b_search_then_add_deleted": [], "c_facet_count_plus_one_doc": []}
    b_note = None
    for r in range(args.rounds):
        sh.set_deleted([])
        ms, out = clock(lambda: sh.delete_by_query(q))
        assert out[2] == matched
        t["a_without_ids"].append(ms)
        sh.set_deleted([])
        ms, out = clock(lambda: sh.delete_by_query(q, return_docs=True))
        assert out[2] == matched and len(out[3]) == matched
        t["a_with_ids"].append(ms)
        if r < b_rounds:
            sh.set_deleted([])
            box = {}
            th = threading.Thread(target=lambda: box.update(zip(("ms", "n"), clock(lambda: route_b(q, matched)))))
            th.start()
            th.join(args.limit)
            if th.is_alive():
                b_note = "over the limit of %.0f s" % args.limit
                th.join()
            else:
                assert box["n"] == matched
                t["b_search_then_add_deleted"].append(box["ms"])
        sh.set_deleted([])
        ms, _ = clock(lambda: floor_c(q))
        t["c_facet_count_plus_one_doc"].append(ms)
    entry = {"matched": matched, "search_passes_of_1024": -(-matched // 1024)}
    for side, ms in t.items():
        entry[side] = summary(ms) if ms else {"note": b_note}
    if b_note and t["b_search_then_add_deleted"]:
        entry["b_search_then_add_deleted"]["note"] = b_note
    entry["a_with_ids_over_c"] = entry["a_with_ids"]["median_ms"] / entry["c_facet_count_plus_one_doc"]["median_ms"]
    entry["a_without_ids_over_c"] = entry["a_without_ids"]["median_ms"] / entry["c_facet_count_plus_one_doc"]["median_ms"]
    result["shapes"][name] = entry
    print(name, json.dumps(entry), flush=True)
sh.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
