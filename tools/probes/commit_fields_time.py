"""Incremental commits of an image with THREE indexed fields: a corpus grown by 16 levels of 65 536 docs, per level the wall time of the
commit call -- ss_bm25_commit_level_fields (levels in HBM, device rebuild) without and with positions, and ss_bm25_append_level_fields
(levels on the host, host rebuild of the whole shard) as the baseline.  Three runs each on fresh shards; per level the median and
the spread (max - min) go to a JSON file, merged with what it holds (so that a run on another checkout adds its series).
    python tools/probes/commit_fields_time.py [--entries commit,commit_pos,append] [--tag TEXT] [--root CHECKOUT] [--out FILE] [--runs 3]
--root: the checkout whose package is measured (default: this one); --tag: appended to the series' names."""
import argparse, json, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--entries", default="commit,commit_pos,append")
ap.add_argument("--tag", default="")
ap.add_argument("--root", default=os.path.join(HERE, "..", ".."))
ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "commit_fields_time.json"))
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--levels", type=int, default=16)
ap.add_argument("--terms", type=int, default=256)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import seekstorm_amd as S

LVL, NF, BOOST = 65536, 3, [2.0, 1.0, 0.5]
NT, NL = args.terms, args.levels
# a term's density falls from 0.3 to 0.001 over the vocabulary; a doc that holds a term holds it in field 0 with p 0.7, in 1 and 2 with 0.35
dens = 0.3 * (0.001 / 0.3) ** (np.arange(NT) / max(NT - 1, 1))
fprob = np.array([0.7, 0.35, 0.35])


def make_level(lv):
    rng = np.random.default_rng(1000 + lv)
    dl = rng.integers(8, 90, (NF, LVL)).astype(np.uint8)
    offs, docs, fields, tfs = [0], [], [], []
    for t in range(NT):
        has = rng.random(LVL) < dens[t]
        inf = (rng.random((LVL, NF)) < fprob) & has[:, None]
        inf[has & ~inf.any(axis=1), 0] = True  # every doc of the term somewhere
        d, f = np.nonzero(inf)                 # sorted by (doc, field)
        docs.append(d + lv * LVL); fields.append(f); tfs.append(np.minimum(rng.geometric(0.5, len(d)), 12))
        offs.append(offs[-1] + len(d))
    tf = np.concatenate(tfs).astype(np.uint16)
    st = np.zeros(len(tf) + 1, np.int64); st[1:] = np.cumsum(tf.astype(np.int64))
    pos = (np.arange(st[-1], dtype=np.int64) - np.repeat(st[:-1], tf.astype(np.int64))).astype(np.uint16)  # 0 .. tf - 1: the content is irrelevant to the cost
    return dl, np.array(offs, np.uint64), np.concatenate(docs).astype(np.uint32), np.concatenate(fields).astype(np.uint8), tf, pos


t0 = time.time()
levels = [make_level(lv) for lv in range(NL)]
n_ent = [int(l[1][-1]) for l in levels]
print("host generation %.1f s: %d levels, %d terms, %.2f M entries and %.2f M positions per level" %
      (time.time() - t0, NL, NT, np.mean(n_ent) / 1e6, np.mean([len(l[5]) for l in levels]) / 1e6), flush=True)


def one_run(entry):
    sh = S.Shard(0)
    ms = []
    try:
        for lv, (dl, offs, docs, fields, tfs, pos) in enumerate(levels):
            t = time.perf_counter()
            if entry == "append":
                sh.append_level_fields(lv, dl, BOOST, offs, docs, fields, tfs)
            else:
                sh.commit_level_fields(lv, dl, BOOST, offs, docs, fields, tfs, positions=pos if entry == "commit_pos" else None)
            ms.append((time.perf_counter() - t) * 1e3)
        q = sh.make_queries([[0, 1], [NT // 2, NT - 1]], S.QueryType.Union)
        tot = sh.search_lexical_batch(q, 10)[3]
        return ms, [int(x) for x in tot], sh.incremental_info()[1]
    finally:
        sh.close()


NAMES = {"commit": "commit_level_fields", "commit_pos": "commit_level_fields, positions", "append": "append_level_fields"}
out = {}
if os.path.exists(args.out):
    out = json.load(open(args.out))
out.setdefault("config", {"levels": NL, "level_docs": LVL, "fields": NF, "terms": NT, "entries_per_level": n_ent, "runs": args.runs,
                          "unit": "ms of wall time of the commit call, per level"})
out.setdefault("series", {})
totals = None
for entry in [e for e in args.entries.split(",") if e]:
    runs = []
    for r in range(args.runs):
        ms, tot, raw_b = one_run(entry)
        assert totals is None or totals == tot, (totals, tot)  # every entry ends with the same image
        totals = tot
        runs.append(ms)
    a = np.array(runs)
    name = NAMES[entry] + (" (" + args.tag + ")" if args.tag else "")
    out["series"][name] = {"median_ms": [round(float(x), 2) for x in np.median(a, axis=0)],
                           "spread_ms": [round(float(x), 2) for x in a.max(axis=0) - a.min(axis=0)],
                           "runs_ms": [[round(float(x), 2) for x in row] for row in a], "levels_bytes_after_last_commit": int(raw_b)}
    med, spr = out["series"][name]["median_ms"], out["series"][name]["spread_ms"]
    print("%-42s level 1 %.1f ms, 4 %.1f, 8 %.1f, 16 %.1f (spread %.1f); growth 4 -> 16: x %.2f" %
          (name, med[0], med[3], med[min(7, NL - 1)], med[-1], spr[-1], med[-1] / med[3]), flush=True)
json.dump(out, open(args.out, "w"), indent=1)
print("wrote", os.path.abspath(args.out))
