"""Faceted callers at the C2 size: 10 M docs (ss_bm25_synth), 16-byte synthetic facet records (tools/probes/sorted_facets_time.py's),
C2's 3-term ORs, k = 10, ONE u32 sort field, three facets (string16 with 64 ids, i32 with 10 ranges, u8).
  (a) ONE call of 64 queries under 8 distinct filter sets, three ways, ALTERNATED round by round (host clock around each, warm-up first,
      ROUNDS rounds: median and min .. max): ss_bm25_search_each; 8 calls of ss_bm25_search_sorted_facets, one per filter group; 64
      single calls.  The two older forms run with the faceted coalescer off: they are what a host does on the parent commit.
  (b) T = 1, 8, 64 threads, each a loop of one-query calls under ITS OWN filter (ctypes straight into the library, arguments built
      once per thread), the sorted page (ss_bm25_search_sorted_facets) and the unsorted one (ss_bm25_search_facets): q/s, p50, p99 --
      with the faceted kind on, with it off, and on the PARENT commit's build of the library (PARENT_LIB: a libseekstorm_hip.so built
      from the parent commit; the legs alternate process by process, LEGS = 6 of each).
  (c) facet_filter_rows_kernel at R = 1, 8, 64 rows next to facet_filter_kernel on the same records: one rocprofv3 --kernel-trace
      process per R (the kernel's name does not carry R), durations read from its rocpd database.
Usage: python tools/probes/faceted_callers_time.py   -> profiles/faceted_callers_time.json (OUT_DIR in the environment: written there)"""
import ctypes as C
import gc
import glob
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
N_DOCS, ROUNDS, WARM = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("ROUNDS", 24)), 6
SECS = float(os.environ.get("SECS", 1.5))
LEGS = int(os.environ.get("LEGS", 6))  # alternated processes a side
NEW = ("ss_bm25_search_each", "ss_shard_set_coalescing_faceted", "ss_shard_coalescing_stats_faceted")
PARENT = bool(os.environ.get("LEG_PARENT"))


def world():
    from seekstorm_amd import _native as N
    if PARENT:  # the parent commit's library has none of the new entries
        N.SYMBOLS = [s for s in N.SYMBOLS if s[0] not in NEW]
    import seekstorm_amd as S
    from oracle import oracle as O
    import bench
    tl, th = bench.make_c2_queries(O, 64)
    sh = S.Shard(0)
    sh.synth_lexical(O.LEX_SEED, N_DOCS, th, O.len_table())
    rng = np.random.default_rng(3)
    rec = np.dtype([("price", "<u4"), ("date", "<i4"), ("brand", "<u2"), ("cat", "u1"), ("pad", "u1", 5)])
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
    q = sh.make_queries(tl, S.QueryType.Union)
    # 8 filter sets of a sidebar: a brand, or a quarter of the price range; 64 more for the threads: a price window each
    sets8 = [[(off["brand"], "string16", [j])] for j in range(4)] + [[(off["price"], "u32", j << 30, (j + 1) << 30)] for j in range(4)]
    sets64 = [[(off["price"], "u32", t << 25, (t << 25) + (1 << 31))] for t in range(64)]
    return S, N, sh, q, facets, sort, sets8, sets64


def stat(xs):
    return [float(np.median(xs)), float(min(xs)), float(max(xs))]


def eq(a, b):
    n = int(a[2])
    return (n == int(b[2]) and int(a[3]) == int(b[3]) and np.array_equal(a[0][:n], b[0][:n]) and np.array_equal(a[1][:n].view(np.uint32), b[1][:n].view(np.uint32)) and
            all(np.array_equal(x, y) for x, y in zip(a[4], b[4])))


def part_a(S, sh, q, facets, sort, sets8):
    TC = S.ResultType.TopkCount
    per_query = [sets8[i % 8] for i in range(64)]
    groups = [np.ascontiguousarray(q[g::8]) for g in range(8)]
    each = lambda: sh.search_lexical_each(q, 10, TC, per_query, sort, facets)
    grouped = lambda: [sh.search_lexical_sorted_facets(groups[g], sort, 10, facets, TC, sets8[g]) for g in range(8)]
    singles = lambda: [sh.search_lexical_sorted_facets(q[i:i + 1], sort, 10, facets, TC, per_query[i]) for i in range(64)]
    sh.set_coalescing_faceted(0)
    for _ in range(WARM):
        e, g, s1 = each(), grouped(), singles()
    row = lambda r, i: (r[0][i], r[1][i], r[2][i], r[3][i], [p[i] for p in r[4]])
    same = all(eq(row(e, i), row(s1[i], 0)) and eq(row(e, i), row(g[i % 8], i // 8)) for i in range(64))
    te, tg, ts = [], [], []
    gc.collect()
    gc.disable()
    for _ in range(ROUNDS):  # alternated: a drift of the machine reaches all three alike
        t0 = time.perf_counter(); each(); t1 = time.perf_counter(); grouped(); t2 = time.perf_counter(); singles(); t3 = time.perf_counter()
        te.append((t1 - t0) * 1e6); tg.append((t2 - t1) * 1e6); ts.append((t3 - t2) * 1e6)
    gc.enable()
    out = {"each_us": stat(te), "grouped_8_calls_us": stat(tg), "single_64_calls_us": stat(ts), "same_answers": bool(same),
           "mean_matches": float(np.mean(e[3])), "each_rounds_us": [round(x, 1) for x in te], "grouped_rounds_us": [round(x, 1) for x in tg]}
    gain, spreads = out["grouped_8_calls_us"][0] - out["each_us"][0], (max(te) - min(te)) + (max(tg) - min(tg))
    out["each_gain_over_grouped_us"], out["two_spreads_us"], out["keep_fast_path"] = gain, spreads, bool(gain > spreads)
    print("a", {k: v for k, v in out.items() if not k.endswith("rounds_us")}, flush=True)
    return out


def part_b(S, N, sh, q, facets, sort, sets64, Ts=(1, 8, 64)):
    """-> {shape: {T: {qps, p50_us, p99_us}}}; the kind as it stands (the caller set it)"""
    L = N.lib()
    off, ty, nb, allb, bases, stride = sh._query_facet_args(facets)
    n_s, sarr = sh._result_sorts(sort)
    out = {}
    for shape in ("sorted_facets", "facets"):
        out[shape] = {}
        for T in Ts:
            lat = [[] for _ in range(T)]
            stop_at = [0.0]
            bar = threading.Barrier(T + 1)

            def loop(t):
                farr, nf = sh.facet_filters(sets64[t % 64])
                qq = np.ascontiguousarray(q[t % 64:t % 64 + 1])
                doc, score, cnt, tot, cnts = np.zeros(10, np.uint32), np.zeros(10, np.float32), np.zeros(1, np.uint32), np.zeros(1, np.uint64), np.zeros(stride, np.uint64)
                tail = (nf, C.cast(farr, C.c_void_p), len(facets), N.ptr(off, N.u32p), N.ptr(ty, N.u32p), N.ptr(nb, N.u32p), N.ptr(allb, N.u64p), None,
                        N.ptr(doc, N.u32p), N.ptr(score, N.f32p), N.ptr(cnt, N.u32p), N.ptr(tot, N.u64p), N.ptr(cnts, N.u64p))
                if shape == "sorted_facets":
                    fn, args = L.ss_bm25_search_sorted_facets, (sh._h, 1, qq.ctypes.data_as(C.c_void_p), n_s, C.cast(sarr, C.c_void_p), 10, N.RT_TOPKCOUNT) + tail
                else:
                    fn, args = L.ss_bm25_search_facets, (sh._h, 1, qq.ctypes.data_as(C.c_void_p), 10, N.RT_TOPKCOUNT) + tail
                for _ in range(3):
                    assert fn(*args) == 0
                bar.wait(timeout=120)
                mine, pc = lat[t], time.perf_counter
                while True:
                    t0 = pc()
                    if t0 >= stop_at[0]:
                        break
                    rc = fn(*args)
                    mine.append(pc() - t0)
                    if rc != 0:
                        mine.append(-1.0)
                        break

            th = [threading.Thread(target=loop, args=(t,)) for t in range(T)]
            for x in th:
                x.start()
            stop_at[0] = time.perf_counter() + SECS + 1.0  # (set before the barrier opens; the warm-up calls are behind it)
            bar.wait(timeout=120)
            t_begin = time.perf_counter()
            stop_at[0] = t_begin + SECS
            for x in th:
                x.join()
            took = time.perf_counter() - t_begin
            allv = np.array([x for l in lat for x in l])
            assert (allv >= 0).all(), "a call failed"
            out[shape][str(T)] = {"qps": round(len(allv) / took, 1), "p50_us": round(float(np.percentile(allv, 50)) * 1e6, 1),
                                  "p99_us": round(float(np.percentile(allv, 99)) * 1e6, 1), "calls": int(len(allv))}
            print("b", "parent" if PARENT else "new", shape, T, out[shape][str(T)], flush=True)
    return out


def leg():
    S, N, sh, q, facets, sort, sets8, sets64 = world()
    out = {}
    if os.environ.get("LEG_KERNELS"):  # (c): a few calls that launch the two kernels, for rocprofv3 to time
        R = int(os.environ["LEG_KERNELS"])
        per_query = [sets64[i % R] for i in range(64)]
        for _ in range(12):
            sh.search_lexical_each(q, 10, S.ResultType.Count, per_query, [], facets)
            sh.search_lexical_batch(q[:1], 10, S.ResultType.Count, False, sets64[0])
    elif PARENT:
        out["b_parent"] = part_b(S, N, sh, q, facets, sort, sets64)
    else:
        if os.environ.get("LEG_A"):
            out["a"] = part_a(S, sh, q, facets, sort, sets8)
        sh.set_coalescing_faceted(64, 0)
        s0 = sh.coalescing_stats_faceted()
        out["b_on"] = part_b(S, N, sh, q, facets, sort, sets64)
        s1 = sh.coalescing_stats_faceted()
        out["b_on_mean_batch"] = round((s1[1] - s0[1]) / max(s1[0] - s0[0], 1), 2)
        sh.set_coalescing_faceted(0)
        out["b_off"] = part_b(S, N, sh, q, facets, sort, sets64)
    sh.close()
    json.dump(out, open(os.environ["LEG_OUT"], "w"))


def kernel_times(out_dir):
    """(c) -> {R: {kernel: [avg us, min us, max us, launches]}}"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    res = {}
    for R in (1, 8, 64):
        d = os.path.join(out_dir, "faceted_callers_prof_%d" % R)
        shutil.rmtree(d, ignore_errors=True)
        path = os.path.join(out_dir, "faceted_callers_leg_k.json")
        rc = subprocess.call([prof, "--kernel-trace", "-d", d, "-o", "x", "--", sys.executable, os.path.abspath(__file__)],
                             env=dict(os.environ, LEG_OUT=path, LEG_KERNELS=str(R)), timeout=300, stdout=subprocess.DEVNULL)
        if rc != 0:
            print("kernel leg", R, "failed:", rc, flush=True)
            return None  # (nothing more is started on the device)
        db = sqlite3.connect(glob.glob(os.path.join(d, "**", "*results.db"), recursive=True)[0])
        tables = [r[0] for r in db.execute("select name from sqlite_master where type in ('table', 'view')")]
        t = "kernels" if "kernels" in tables else [x for x in tables if x.startswith("kernels")][0]
        cols = [r[1] for r in db.execute("pragma table_info(%s)" % t)]
        name = "name" if "name" in cols else "kernel_name"
        res[str(R)] = {}
        for kern in ("facet_filter_rows_kernel", "facet_filter_kernel"):
            rows = db.execute("select end - start from %s where %s like ?" % (t, name), ("%" + kern + "%",)).fetchall()
            xs = [r[0] / 1e3 for r in rows][2:]  # (the first launches: cold)
            if xs:
                res[str(R)][kern] = [round(float(np.mean(xs)), 2), round(min(xs), 2), round(max(xs), 2), len(xs)]
        db.close()
        shutil.rmtree(d, ignore_errors=True)
        os.remove(path)
        print("c", R, res[str(R)], flush=True)
    return res


if os.environ.get("LEG_OUT"):
    leg()
    sys.exit(0)
out_dir = os.environ.get("OUT_DIR") or os.path.join(ROOT, "profiles")
parent_lib = os.environ.get("PARENT_LIB")
res = {"docs": N_DOCS, "rounds": ROUNDS, "seconds_per_thread_leg": SECS, "unit": "us: [median, min, max]; threads: q/s, p50 and p99 of a call in us"}
legs = {"new": [], "parent": []}
order = ["new", "parent"] * LEGS if parent_lib else ["new", "new"]
for n_leg, which in enumerate(order):
    path = os.path.join(out_dir, "faceted_callers_leg.json")
    env = dict(os.environ, LEG_OUT=path)
    if which == "parent":
        env.update(LEG_PARENT="1", SEEKSTORM_HIP_LIB=parent_lib)
    elif n_leg == 0:
        env.update(LEG_A="1")
    rc = subprocess.call([sys.executable, os.path.abspath(__file__)], env=env, timeout=500)
    if rc != 0:
        print("leg", which, "failed:", rc, flush=True)
        sys.exit(1)  # (nothing more is started on the device)
    legs[which].append(json.load(open(path)))
    os.remove(path)
res["a_one_call_of_64_queries_8_filter_sets"] = legs["new"][0]["a"]
res["b_threads"] = {"kind_on_rounds": [l["b_on"] for l in legs["new"]], "kind_off_rounds": [l["b_off"] for l in legs["new"]],
                    "parent_build_rounds": [l["b_parent"] for l in legs["parent"]], "kind_on_mean_batch": [l["b_on_mean_batch"] for l in legs["new"]]}
if legs["parent"]:
    cond = {}
    for shape in ("sorted_facets", "facets"):
        on64 = [r[shape]["64"]["qps"] for r in res["b_threads"]["kind_on_rounds"]]
        pa64 = [r[shape]["64"]["qps"] for r in res["b_threads"]["parent_build_rounds"]]
        on1 = [r[shape]["1"]["p50_us"] for r in res["b_threads"]["kind_on_rounds"]]
        pa1 = [r[shape]["1"]["p50_us"] for r in res["b_threads"]["parent_build_rounds"]]
        cond[shape] = {"T64_qps_on": on64, "T64_qps_parent": pa64, "T64_gains": bool(min(on64) - max(pa64) > (max(on64) - min(on64)) + (max(pa64) - min(pa64))),
                       "T1_p50_on": on1, "T1_p50_parent": pa1,
                       "T1_p50_on_median": float(np.median(on1)), "T1_p50_parent_min_max": [min(pa1), max(pa1)],
                       # the issue's rule: the kind-on p50 (median of its rounds) inside the parent's round-to-round spread -- not above
                       # the slowest parent round (below the fastest is no loss either)
                       "T1_does_not_lose": bool(np.median(on1) <= max(pa1))}
    res["default_on_condition"] = cond
    res["default_on"] = all(c["T64_gains"] and c["T1_does_not_lose"] for c in cond.values())
res["c_filter_kernels_us_avg_min_max_launches"] = kernel_times(out_dir)
json.dump(res, open(os.path.join(out_dir, "faceted_callers_time.json"), "w"), indent=1)
print(json.dumps({k: v for k, v in res.items() if k != "a_one_call_of_64_queries_8_filter_sets"}, indent=1))
