"""Incremental commits of an image with THREE indexed fields AND a sparse tier: the dense part is the shape of commit_fields_time.py (16
levels of 65 536 docs, 256 dense terms), beside it --rare rare terms whose entries of a level go through
ss_bm25_commit_sparse_level_fields.  Per level the wall time of the dense commit plus the sparse commit, without and with positions
(median and spread of --runs runs on fresh shards), and beside it what a host had to do before for the same prefix: ONE
ss_bm25_upload_fields[_positions] plus ONE ss_bm25_append_sparse_fields[_positions] of everything committed so far (at --prefixes).
    python tools/probes/commit_fields_tier_time.py [--out FILE] [--runs 3] [--levels 16] [--terms 256] [--rare 20000]"""
import argparse, json, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "commit_fields_tier_time.json"))
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--levels", type=int, default=16)
ap.add_argument("--terms", type=int, default=256)
ap.add_argument("--rare", type=int, default=20000)
ap.add_argument("--rare-entries", type=int, default=60000, help="entries of the rare terms per level")
ap.add_argument("--prefixes", default="1,2,4,8,12,16")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import seekstorm_amd as S

LVL, NF, BOOST = 65536, 3, [2.0, 1.0, 0.5]
NT, NL, NR = args.terms, args.levels, args.rare
dens = 0.3 * (0.001 / 0.3) ** (np.arange(NT) / max(NT - 1, 1))  # (commit_fields_time.py)
fprob = np.array([0.7, 0.35, 0.35])


def with_positions(tf):
    st = np.zeros(len(tf) + 1, np.int64); st[1:] = np.cumsum(tf.astype(np.int64))
    return (np.arange(st[-1], dtype=np.int64) - np.repeat(st[:-1], tf.astype(np.int64))).astype(np.uint16)  # 0 .. tf - 1


def make_level(lv):
    rng = np.random.default_rng(1000 + lv)
    dl = rng.integers(8, 90, (NF, LVL)).astype(np.uint8)
    offs, docs, fields, tfs = [0], [], [], []
    for t in range(NT):
        has = rng.random(LVL) < dens[t]
        inf = (rng.random((LVL, NF)) < fprob) & has[:, None]
        inf[has & ~inf.any(axis=1), 0] = True
        d, f = np.nonzero(inf)
        docs.append(d + lv * LVL); fields.append(f); tfs.append(np.minimum(rng.geometric(0.5, len(d)), 12))
        offs.append(offs[-1] + len(d))
    tf = np.concatenate(tfs).astype(np.uint16)
    dense = (np.array(offs, np.uint64), np.concatenate(docs).astype(np.uint32), np.concatenate(fields).astype(np.uint8), tf, with_positions(tf))
    # the rare terms: skewed list sizes (a term's share falls like 1 / rank), one field per entry, now and then a second one
    w = 1.0 / np.arange(1, NR + 1)
    term = rng.choice(NR, args.rare_entries, p=w / w.sum())
    key = np.unique(term.astype(np.int64) * LVL + rng.integers(0, LVL, len(term)))  # distinct (term, doc), sorted
    f0 = rng.integers(0, NF, len(key))
    two = rng.random(len(key)) < 0.2
    k2 = np.concatenate([key * NF + f0, key[two] * NF + (f0[two] + 1) % NF])
    k2.sort()
    rterm, rdoc, rfield = k2 // (NF * LVL), (k2 // NF) % LVL + lv * LVL, k2 % NF
    roffs = np.zeros(NR + 1, np.uint64); roffs[1:] = np.cumsum(np.bincount(rterm, minlength=NR))
    rtf = np.minimum(rng.geometric(0.6, len(k2)), 6).astype(np.uint16)
    rare = (roffs, rdoc.astype(np.uint32), rfield.astype(np.uint8), rtf, with_positions(rtf))
    return dl, dense, rare


def prefix_of(parts, n_terms):
    """the levels' CSRs (offs, docs, fields, tfs, positions) as ONE CSR: a term's entries level after level"""
    term = np.concatenate([np.repeat(np.arange(n_terms), np.diff(p[0].astype(np.int64))) for p in parts])
    order = np.argsort(term, kind="stable")
    docs, fields, tfs = (np.concatenate([p[i] for p in parts])[order] for i in (1, 2, 3))
    offs = np.zeros(n_terms + 1, np.uint64); offs[1:] = np.cumsum(np.bincount(term, minlength=n_terms))
    return offs, docs, fields, tfs, with_positions(tfs)


t0 = time.time()
levels = [make_level(lv) for lv in range(NL)]
print("host generation %.1f s: %d levels, %d dense terms with %.2f M entries and %d rare terms with %.3f M entries per level" %
      (time.time() - t0, NL, NT, np.mean([len(l[1][1]) for l in levels]) / 1e6, NR, np.mean([len(l[2][1]) for l in levels]) / 1e6), flush=True)


def tiered_run(positions):
    sh = S.Shard(0)
    ms = []
    try:
        for lv, (dl, dense, rare) in enumerate(levels):
            t = time.perf_counter()
            sh.commit_level_fields(lv, dl, BOOST, *dense[:4], positions=dense[4] if positions else None)
            sh.commit_sparse_level_fields(lv, *rare[:4], positions=rare[4] if positions else None)
            ms.append((time.perf_counter() - t) * 1e3)
        tot = sh.search_lexical_batch(sh.make_queries([[0, 1], [NT, NT + 1, 3]], S.QueryType.Union), 10)[3]
        return ms, [int(x) for x in tot], sh.sparse_info()
    finally:
        sh.close()


def upload_run(positions, n_levels, dense, rare):
    dl = np.concatenate([l[0] for l in levels[:n_levels]], axis=1)
    sh = S.Shard(0)
    try:
        t = time.perf_counter()
        sh.upload_lexical_fields(n_levels * LVL, dl, BOOST, *dense[:4], dense[4] if positions else None)
        sh.append_sparse_fields(*rare[:4], positions=rare[4] if positions else None)
        ms = (time.perf_counter() - t) * 1e3
        tot = sh.search_lexical_batch(sh.make_queries([[0, 1], [NT, NT + 1, 3]], S.QueryType.Union), 10)[3]
        return ms, [int(x) for x in tot]
    finally:
        sh.close()


out = {"config": {"levels": NL, "level_docs": LVL, "fields": NF, "dense_terms": NT, "rare_terms": NR,
                  "dense_entries_per_level": [int(len(l[1][1])) for l in levels], "rare_entries_per_level": [int(len(l[2][1])) for l in levels],
                  "runs": args.runs, "unit": "ms of wall time per level: the dense commit plus the sparse commit; the re-upload at the listed prefixes"},
       "series": {}}
totals = {}
for positions in (False, True):
    runs = []
    for r in range(args.runs):
        ms, tot, info = tiered_run(positions)
        runs.append(ms)
        totals[NL] = tot
    a = np.array(runs)
    name = "commit_level_fields + commit_sparse_level_fields" + (", positions" if positions else "")
    out["series"][name] = {"median_ms": [round(float(x), 2) for x in np.median(a, axis=0)], "spread_ms": [round(float(x), 2) for x in a.max(axis=0) - a.min(axis=0)],
                           "runs_ms": [[round(float(x), 2) for x in row] for row in a], "sparse_info_after_last_commit": list(info)}
    med, spr = out["series"][name]["median_ms"], out["series"][name]["spread_ms"]
    print("%-62s level 1 %.1f ms, 4 %.1f, 8 %.1f, %d %.1f (spread %.1f)" % (name, med[0], med[min(3, NL - 1)], med[min(7, NL - 1)], NL, med[-1], spr[-1]), flush=True)
prefixes = [int(x) for x in args.prefixes.split(",") if int(x) <= NL]
up = {False: {}, True: {}}
for n in prefixes:
    dense = prefix_of([l[1] for l in levels[:n]], NT)
    rare = prefix_of([l[2] for l in levels[:n]], NR)
    for positions in (False, True):
        res = [upload_run(positions, n, dense, rare) for _ in range(args.runs)]
        if n == NL:
            assert res[0][1] == totals[NL], (res[0][1], totals[NL])  # both ways end with the same image
        up[positions][n] = [r[0] for r in res]
    del dense, rare
for positions in (False, True):
    name = "upload_fields + append_sparse_fields of the prefix" + (", positions" if positions else "")
    out["series"][name] = {"levels": prefixes, "median_ms": [round(float(np.median(up[positions][n])), 2) for n in prefixes],
                           "spread_ms": [round(float(max(up[positions][n]) - min(up[positions][n])), 2) for n in prefixes],
                           "runs_ms": [[round(float(x), 2) for x in up[positions][n]] for n in prefixes]}
    print("%-62s %s" % (name, ", ".join("%d levels %.1f ms" % (n, m) for n, m in zip(prefixes, out["series"][name]["median_ms"]))), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(out, open(args.out, "w"), indent=1)
print("wrote", os.path.abspath(args.out))
