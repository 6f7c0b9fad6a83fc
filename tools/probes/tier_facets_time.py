"""Match sets of queries that name sparse-tier terms (csrc/bm25_match.hip): what a facet count, a sort pivot and a sorted search cost
when the query is tiered, against an all-dense query of the same list count on the same image.

Image: 1 M docs, 8 dense lists (df 0.5 % .. 20 %) and 64 sparse lists (50 .. 1940 postings) drawn from a pool of 50 000 docs.  Times: host
clock around whole calls (each ends in the library's own stream synchronisation), warm-up first, medians over REPS repeats of CALLS
calls, spread = min .. max of the repeats.  The match set's share of a facet-count call is not separable from outside: it is read
from the difference between query shapes, and stated as such."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import seekstorm_amd as S
from oracle import oracle as O

N_DOCS, REPS = 1_000_000, 7
rng = np.random.default_rng(5)
dl = O.lex_doclen(N_DOCS)
offs, docs, tfs = [0], [], []
for df in (0.005, 0.01, 0.02, 0.04, 0.08, 0.12, 0.16, 0.2):
    d = np.sort(rng.choice(N_DOCS, int(df * N_DOCS), replace=False)).astype(np.uint32)
    docs.append(d); tfs.append(np.minimum(rng.geometric(0.6, len(d)), 60).astype(np.uint16)); offs.append(offs[-1] + len(d))
ND = len(offs) - 1
hot = np.sort(rng.choice(N_DOCS, 50_000, replace=False))
s_offs, s_docs, s_tfs = [0], [], []
sizes = [50 + 30 * i for i in range(64)]
for n in sizes:
    d = np.sort(rng.choice(hot, n, replace=False)).astype(np.uint32)
    s_docs.append(d); s_tfs.append(np.minimum(rng.geometric(0.5, n), 30).astype(np.uint16)); s_offs.append(s_offs[-1] + n)
sh = S.Shard(0)
sh.upload_lexical(N_DOCS, dl, np.asarray(offs, np.uint64), np.concatenate(docs), np.concatenate(tfs))
assert sh.append_sparse(np.asarray(s_offs, np.uint64), np.concatenate(s_docs), np.concatenate(s_tfs)) == ND
rec = np.dtype([("date", "<u4"), ("cat", "u1"), ("price", "<f4")])
v = np.zeros(N_DOCS, rec)
v["date"] = rng.integers(0, 1 << 31, N_DOCS); v["cat"] = rng.integers(0, 20, N_DOCS); v["price"] = rng.random(N_DOCS) * 1000
sh.upload_facets(v.view(np.uint8).reshape(N_DOCS, rec.itemsize))
off = {n: rec.fields[n][1] for n in rec.names}
sh.set_deleted(list(range(7, N_DOCS, 211)))


def timed(call, calls):
    for _ in range(max(3, calls // 10)):
        call()
    reps = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        reps.append((time.perf_counter() - t0) / calls * 1e6)
    return float(np.median(reps)), min(reps), max(reps)


U, I = S.QueryType.Union, S.QueryType.Intersection
sp = lambda i: ND + i
shapes = [("or3 all dense", U, [1, 3, 5], []), ("or3 one sparse", U, [1, 3, sp(40)], []), ("or3 two sparse", U, [1, sp(63), sp(40)], []),
          ("or3 all sparse", U, [sp(10), sp(63), sp(40)], []), ("or2 dense - dense", U, [1, 3], [5]), ("or2 dense - sparse", U, [1, 3], [sp(63)]),
          ("and2 all dense", I, [4, 6], []), ("and2 dense & sparse", I, [6, sp(63)], []), ("and2 sparse & sparse", I, [sp(62), sp(63)], [])]
print(f"image: {N_DOCS} docs, {ND} dense lists, {len(sizes)} sparse lists of {sizes[0]}..{sizes[-1]} postings; "
      f"medians of {REPS} x 200 calls, us per call (min .. max of the repeats)")
base = {}
bounds = list(range(20))
for name, qt, terms, neg in shapes:
    q = sh.make_queries([terms], qt, [neg])
    tot = sh.facet_count(q, off["cat"], "u8", range_lower_bounds=bounds)[2]
    m, lo, hi = timed(lambda: sh.facet_count(q, off["cat"], "u8", range_lower_bounds=bounds), 200)
    km, klo, khi = timed(lambda: sh.facet_kth(q, off["date"], "u32", True, 10), 200)
    key = name.split()[0]
    if "sparse" not in name:
        base.setdefault(key, m)
    ratio = f", x{m / base[key]:.2f} of the all-dense {key}" if key in base and "sparse" in name else ""
    print(f"{name:22s} matches {tot:7d}: facet_count {m:7.1f} ({lo:.1f} .. {hi:.1f}){ratio}; facet_kth {km:7.1f} ({klo:.1f} .. {khi:.1f})", flush=True)

# sorted batches of 64 or3 queries, k = 10: all dense, and every query with one sparse term (a tiered chunk's searches run one by one)
spec = [(off["date"], "u32", True)]
dense_q = sh.make_queries([[int(x) for x in rng.choice(ND, 3, replace=False)] for _ in range(64)], U)
tier_q = sh.make_queries([[int(x) for x in rng.choice(ND, 2, replace=False)] + [sp(int(rng.integers(0, 64)))] for _ in range(64)], U)
for name, q in (("64 x or3 all dense", dense_q), ("64 x or3 one sparse", tier_q)):
    m, lo, hi = timed(lambda: sh.search_lexical_sorted_batch(q, spec, 10), 10)
    print(f"sorted by date desc, k = 10, {name}: {m / 1e3:.2f} ms per call ({lo / 1e3:.2f} .. {hi / 1e3:.2f}), {64 / m * 1e6:.0f} q/s", flush=True)
sh.close()
