#!/usr/bin/env python3
"""CPU model of the pruned kernel's sparse-stage decisions on the benchmark's own C2 queries (csrc/bm25_probe_body.h pb_wave; no GPU):

    python tools/probes/survivor_model.py [queries = 6] [docs = 10000000] [seedless lo as a share of hi = 0.25]

For the first queries of bench.py's batch 0 (make_c2_queries: 3-term unions, top-10) the posting lists are regenerated at full size by the
oracle's generator and weighed with the oracle's component cache (f32 weights: the device's 16-bit codes differ in the last digits only).
Terms are put in the body's processing order (U = idf x largest weight, descending: J the driver, A the first probed list, one further
list).  Only the FIRST driver stream is modelled -- the later ones are almost always non-essential by the time they would start.  A
driver posting SURVIVES the dense stage when

    idf[J] w0 + (hit A ? U[A] : 0) + U[rest] >= thr          (the further list's bound counts whether or not the doc is in it)

and every survivor that hit A costs a rank-table entry and a posting of A ("A fetches").  With the bound summed over the lists whose bit is
set -- idf[J] w0 + (hit A ? U[A] : 0) + (hit rest ? U[rest] : 0) >= thr -- fewer survive.  Three thresholds bracket what a wave sees:

    final    the query's final 10th-best score from the first posting on (the most any schedule can know)
    rising   16 partitions of the doc range in lock step, 256 driver postings a step; the shared threshold is the largest of the
             partitions' OWN 10th-best scores, and starts at the list seed (the best idf x 10th-largest weight of a list)
    ideal    the same walk, threshold = the 10th best over ALL partitions so far
    hist     the same walk, threshold = what the score histogram publishes (csrc/bm25_hist.h, pb_publish_hist): the scores every
             partition ACCEPTS (at or above the threshold it sees and above its own 10th best) are counted in 64 buckets, equal steps in
             float-bit space from lo = the seed to hi = the sum of the U; the threshold is the edge of the highest bucket at or above which
             10 scores were counted (or a partition's own 10th best, where that is larger)
    rising, no seed / hist, no seed   the two walks for a query that has no seed (tombstones, NOT terms, filters): the threshold starts at 0 and
             lo = SEEDLESS_LO x hi; scores below lo are not counted

Prints one table row per threshold: survivors as a share of the driver postings and A fetches per query, under both rules, and for the
walks the accepted offers per query -- each is one atomic add, and one read of the 64 counters, of the histogram's mechanism."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

K = 10
PARTS, STEP = 16, 256
HIST_B, SEEDLESS_LO = 64, 0.25  # (bm25_hist.h BM_HIST_B, BM_HIST_SEEDLESS_LO)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32).astype(np.int64)


def hist_rule(lo, hi):
    """(lo_bits, shift): the smallest shift with (bits(hi) - bits(lo)) >> shift < B"""
    lo_b, hi_b = int(bits(lo)), max(int(bits(lo)), int(bits(hi)))
    shift = 0
    while (hi_b - lo_b) >> shift >= HIST_B:
        shift += 1
    return lo_b, shift


def weights(O, tfs, dl_of_docs, comp):
    k1 = O.lib().so_bm25_term(1.0, 1, 0.0)  # K + 1
    t = tfs.astype(np.float32)
    return (t * np.float32(k1) / (t + comp[dl_of_docs])).astype(np.float32)


def kth(a, k):
    return float(np.partition(a, len(a) - k)[len(a) - k]) if len(a) >= k else 0.0


def model_query(O, terms, th, n_docs, doclen, comp):
    lists = []
    for t in terms:
        d, tf = O.lex_term(int(t), th[int(t)], n_docs)
        w = weights(O, tf, doclen[d], comp)
        idf = O.lib().so_idf(n_docs, len(d))
        lists.append(dict(d=d, w=w, idf=idf, U=idf * float(w.max()), seed=idf * kth(w, K)))
    lists.sort(key=lambda x: -x["U"])
    J, A, R = lists
    pa = np.searchsorted(A["d"], J["d"]); pa[pa == len(A["d"])] = 0
    hit_a = A["d"][pa] == J["d"]
    pr = np.searchsorted(R["d"], J["d"]); pr[pr == len(R["d"])] = 0
    hit_r = R["d"][pr] == J["d"]
    base = J["idf"] * J["w"]
    score = base + np.where(hit_a, A["idf"] * A["w"][pa], 0) + np.where(hit_r, R["idf"] * R["w"][pr], 0)
    ub_old = base + np.where(hit_a, A["U"], 0) + R["U"]
    ub_new = base + np.where(hit_a, A["U"], 0) + np.where(hit_r, R["U"], 0)
    n = len(base)
    out = {"postings": n}
    # docs outside J can be in the top-10 too (A and rest only): the final threshold comes from all three lists
    alld = np.concatenate([J["d"], A["d"], R["d"]])
    alls = np.concatenate([J["idf"] * J["w"], A["idf"] * A["w"], R["idf"] * R["w"]])
    o = np.argsort(alld, kind="stable")
    alld, alls = alld[o], alls[o]
    first = np.r_[True, alld[1:] != alld[:-1]]
    tot = np.add.reduceat(alls, np.nonzero(first)[0])
    final = kth(tot, K)

    def tally(thr):  # thr: per driver posting
        so, sn = ub_old >= thr * 0.99999, ub_new >= thr * 0.99999
        return np.array([so.sum(), sn.sum(), (so & hit_a).sum(), (sn & hit_a).sum()], np.float64)

    out["final"] = np.r_[tally(np.full(n, final, np.float32)), 0.0]
    # the lock-step walk: partition p = an equal share of the doc range, its driver postings in order
    part = np.minimum((J["d"].astype(np.uint64) * PARTS // n_docs).astype(np.int64), PARTS - 1)
    starts = np.searchsorted(part, np.arange(PARTS + 1))
    seed = max(x["seed"] for x in lists)
    hi = sum(x["U"] for x in lists)
    for name in ("rising", "ideal", "hist", "rising, no seed", "hist, no seed"):
        thr = np.empty(n, np.float32)
        own = [np.zeros(0, np.float32) for _ in range(PARTS)]
        seeded = not name.endswith("no seed")
        cur = seed if seeded else 0.0
        lo_b, shift = hist_rule(seed if seeded else SEEDLESS_LO * hi, hi)
        counts = np.zeros(HIST_B, np.int64)
        accepted = 0
        for s in range(0, int((starts[1:] - starts[:-1]).max()), STEP):
            for p in range(PARTS):
                a, b = starts[p] + s, min(starts[p] + s + STEP, starts[p + 1])
                if a < b:
                    thr[a:b] = cur
                    sc = score[a:b]
                    acc = sc[(sc >= cur) & (sc > (own[p][0] if len(own[p]) >= K else 0.0))]  # offers past the wave's own worst
                    accepted += len(acc)
                    if name.startswith("hist") and len(acc):
                        bb = bits(acc)
                        bb = bb[bb >= lo_b]
                        np.add.at(counts, np.minimum(HIST_B - 1, (bb - lo_b) >> shift), 1)
                    m = np.concatenate([own[p], sc])
                    own[p] = np.sort(m)[-K:]
            own_best = max((float(x[0]) for x in own if len(x) >= K), default=0.0)
            if name.startswith("rising"):
                cur = max(cur, own_best)
            elif name == "ideal":
                cur = max(cur, kth(np.concatenate(own), K))
            else:
                suffix = np.cumsum(counts[::-1])[::-1]
                reach = np.nonzero(suffix >= K)[0]
                edge = float(np.array([lo_b + (int(reach[-1]) << shift)], np.uint32).view(np.float32)[0]) if len(reach) else 0.0
                cur = max(cur, own_best, edge)
        out[name] = np.r_[tally(thr), accepted]
    return out


def main():
    global SEEDLESS_LO
    if len(sys.argv) > 3:
        SEEDLESS_LO = float(sys.argv[3])
    nq = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    n_docs = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    from oracle import oracle as O
    import bench
    term_lists, th = bench.make_c2_queries(O, 1000)
    doclen = O.lex_doclen(n_docs)
    L = O.lib()
    lens = np.array([L.so_byte4_to_int(i) for i in range(256)], np.uint64)
    comp = np.empty(256, np.float32)
    L.so_bm25_component_cache(L.so_avgdl(int(lens[doclen].sum()), n_docs), comp.ctypes.data_as(O.f32p))
    names = ("final", "rising", "ideal", "hist", "rising, no seed", "hist, no seed")
    acc = {k: np.zeros(5) for k in names}
    posts = 0
    for q in range(nq):
        r = model_query(O, term_lists[q], th, n_docs, doclen, comp)
        posts += r["postings"]
        for k in acc:
            acc[k] += r[k]
    print(f"{nq} queries of batch 0, {n_docs} docs, {posts / nq:.0f} driver postings a query; seedless lo = {SEEDLESS_LO} x hi")
    print("| threshold the wave sees | survivors, today | survivors, bound over set bits | A fetches, today | A fetches, bound over set bits | accepted offers |")
    print("|---|---|---|---|---|---|")
    for k in names:
        a = acc[k]
        print(f"| {k} | {100 * a[0] / posts:.2f} % | {100 * a[1] / posts:.2f} % | {a[2] / nq:.0f} per query | {a[3] / nq:.0f} per query | "
              + (f"{a[4] / nq:.0f} per query |" if k != "final" else "- |"))


if __name__ == "__main__":
    main()
