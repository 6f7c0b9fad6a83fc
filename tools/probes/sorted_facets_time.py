"""A sorted search page with its query_facets at the C2 size: 10 M docs (ss_bm25_synth), 16-byte synthetic facet records, C2's 3-term
ORs and 2-term ANDs, nq 1 and 64, k = 10, ONE u32 sort field, three facets (string16 with 64 ids, i32 with 10 ranges, u8).
  a: the two calls there were before -- ss_bm25_search_sorted + ss_bm25_search_facets(SS_RT_COUNT);
  b: ss_bm25_search_sorted_facets with SS_SORT_FUSED=0 (one match-set build; facet count, then the whole radix select);
  c: ss_bm25_search_sorted_facets at its default (facet_sort_first_kernel: the facets and the select's first byte in one launch).
SS_SORT_FUSED is read once per process, so the script runs itself twice, one leg per setting; inside a leg `a` and the new entry
ALTERNATE round by round (host clock around each call, warm-up first, ROUNDS rounds: median and min .. max), and `a` -- the same code
in both legs -- shows how far two processes drift apart.  Answers of the two routes are compared once per shape.
Usage: python tools/probes/sorted_facets_time.py   -> profiles/sorted_facets_time.json (OUT_DIR in the environment: written there instead)"""
import gc
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
N_DOCS, ROUNDS, WARM = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("ROUNDS", 24)), 10


def leg():
    import seekstorm_amd as S
    from oracle import oracle as O
    import bench
    tl, th = bench.make_c2_queries(O, 64)
    sh = S.Shard(0)
    sh.synth_lexical(O.LEX_SEED, N_DOCS, th, O.len_table())
    rng = np.random.default_rng(3)
    rec = np.dtype([("price", "<u4"), ("date", "<i4"), ("brand", "<u2"), ("cat", "u1"), ("pad", "u1", 5)])
    assert rec.itemsize == 16
    v = np.zeros(N_DOCS, rec)
    v["price"] = rng.integers(0, 1 << 32, N_DOCS, dtype=np.uint64)
    v["date"] = rng.integers(0, 1 << 31, N_DOCS)
    v["brand"] = np.minimum(rng.zipf(1.2, N_DOCS), 80) - 1
    v["cat"] = rng.integers(0, 20, N_DOCS)
    sh.upload_facets(v.view(np.uint8).reshape(N_DOCS, rec.itemsize))
    off = {n: rec.fields[n][1] for n in rec.names}
    facets = [
        {"field": "brand", "offset": off["brand"], "type": "string16", "values": ["b%d" % i for i in range(64)], "prefix": "", "length": 10},
        {"field": "date", "offset": off["date"], "type": "i32", "ranges": [("d%d" % i, i * 200_000_000) for i in range(10)], "range_type": "within"},
        {"field": "cat", "offset": off["cat"], "type": "u8", "ranges": [("c%d" % i, i) for i in range(20)], "range_type": "within"},
    ]
    sort = [(off["price"], "u32", False)]
    ba, bb = bench.band_terms(th, 0.01, 0.05), bench.band_terms(th, 0.05, 0.20)
    and_tl = [[int(rng.choice(ba)), int(rng.choice(bb))] for _ in range(64)]
    TC, CNT = S.ResultType.TopkCount, S.ResultType.Count

    def two_calls(q):
        hits = sh.search_lexical_sorted_batch(q, sort, 10)
        return hits, sh.search_lexical_facets(q, 0, facets, CNT, reference_shortcuts=False)[4]

    def one_call(q):
        return sh.search_lexical_sorted_facets(q, sort, 10, facets, TC)

    out = {}
    for name, lists, qt in (("or3", tl, S.QueryType.Union), ("and2", and_tl, S.QueryType.Intersection)):
        for nq in (1, 64):
            q = sh.make_queries(lists[:nq], qt)
            for _ in range(WARM):
                ra, rn = two_calls(q), one_call(q)
            same = all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                       for x, y in zip(ra[0], rn[:4])) and all(np.array_equal(x, y) for x, y in zip(ra[1], rn[4]))
            ta, tn = [], []
            gc.collect()
            gc.disable()  # (a collection inside one timed call would be that variant's max)
            for _ in range(ROUNDS):  # alternated: a drift of the machine reaches both alike
                t0 = time.perf_counter(); two_calls(q); t1 = time.perf_counter(); one_call(q); t2 = time.perf_counter()
                ta.append((t1 - t0) * 1e6); tn.append((t2 - t1) * 1e6)
            gc.enable()
            out["%s_nq%d" % (name, nq)] = {"two_calls_us": [float(np.median(ta)), min(ta), max(ta)], "one_call_us": [float(np.median(tn)), min(tn), max(tn)],
                                           "same_answers": bool(same), "mean_matches": float(np.mean(rn[3])),
                                           "two_calls_rounds_us": [round(x, 1) for x in ta], "one_call_rounds_us": [round(x, 1) for x in tn]}
            print(name, nq, {k: v for k, v in out["%s_nq%d" % (name, nq)].items() if not k.endswith("rounds_us")}, flush=True)
    sh.close()
    json.dump(out, open(os.environ["LEG_OUT"], "w"))


if os.environ.get("LEG_OUT"):
    leg()
    sys.exit(0)
out_dir = os.environ.get("OUT_DIR") or os.path.join(ROOT, "profiles")
res = {"docs": N_DOCS, "rounds": ROUNDS, "unit": "us per page: [median, min, max]", "shapes": {}}
legs = {}
for tag, fused in (("b", "0"), ("c", "1")):
    path = os.path.join(out_dir, "sorted_facets_time_leg_%s.json" % tag)
    rc = subprocess.call([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, LEG_OUT=path, SS_SORT_FUSED=fused), timeout=500)
    if rc != 0:
        print("leg", tag, "failed:", rc, flush=True)
        sys.exit(1)  # (nothing more is started on the device)
    legs[tag] = json.load(open(path))
    os.remove(path)
for shape in legs["b"]:
    b, c = legs["b"][shape], legs["c"][shape]
    res["shapes"][shape] = {"a_two_calls_in_leg_b": b["two_calls_us"], "a_two_calls_in_leg_c": c["two_calls_us"], "b_unfused": b["one_call_us"],
                            "c_fused": c["one_call_us"], "same_answers": b["same_answers"] and c["same_answers"], "mean_matches": c["mean_matches"],
                            "b_rounds_us": b["one_call_rounds_us"], "c_rounds_us": c["one_call_rounds_us"]}
json.dump(res, open(os.path.join(out_dir, "sorted_facets_time.json"), "w"), indent=1)
print(json.dumps(res, indent=1))
