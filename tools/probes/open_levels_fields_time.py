"""What it costs to open an index.bin of SEVERAL indexed fields level by level (ss_bm25_open_index_bin_levels_fields), beside the routes a
host had before, on the three-field text-shaped index of tools/real_format.py (oracle/ss_textindex.c writer; --docs docs, boosts 2 / 1 /
0.5), in one process.  The vocabulary is UNTIERED and cut with ss_index_bin_filter to the keys of at least --min-postings postings (the
entry refuses a tiered ix; the cut is stated in the JSON):
  (a) ss_bm25_upload_index_bin_fields              -- the host decodes every block; no commit can follow
  (b) host decode, then every level through ss_bm25_commit_level_fields -- the route to an image one can commit to before this entry:
      the decode is timed as ss_index_bin_decode_stats (the same host decoder on the same worker threads), the commits per level; the
      cut of the entries per level is not timed (the levels are taken from a read-back of an opened shard)
  (c) ss_bm25_open_index_bin_levels_fields, SS_OPEN_NO_POSITIONS   -- field vectors decoded on the device
  (d) ss_bm25_open_index_bin_levels_fields, SS_OPEN_POSITIONS_HOST -- entries and positions from the host decoder, cut per level
One untimed warm-up round, then --rounds rounds alternating (a), (c), (d) and (b)'s decode; (b)'s commits once; the host clock around
calls that end in a synchronise.  With SS_LOAD_TRACE=1 in the environment the library's own splits go to stderr.  --only c: leg (c) once
and nothing else (for a kernel trace of the decode kernels in a run of its own); --kernel-stats CSV adds that trace's rows
(rocprofv3 --kernel-trace --stats) to the JSON at --out and does nothing else.
    python tools/probes/open_levels_fields_time.py [--out FILE] [--docs 1000000] [--min-postings 200] [--rounds 5] [--only c] [--kernel-stats CSV]"""
import argparse, json, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "open_levels_fields_time.json"))
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--vocab", type=int, default=1_000_000)
ap.add_argument("--min-postings", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--only", default="")
ap.add_argument("--kernel-stats", default="")
args = ap.parse_args()
KERNELS = ("rbd_flat_kernel", "rbd_wg_kernel", "rbd_scan_sums_kernel", "rbd_scan_tiles_kernel", "rbd_scan_write_kernel", "rbd_foff_kernel", "rbd_fsplit_kernel")
if args.kernel_stats:
    import csv
    out = json.load(open(args.out))
    rows = {}
    for r in csv.DictReader(open(args.kernel_stats)):  # (a templated kernel: one row per instantiation)
        for k in KERNELS:
            if k + "(" in r["Name"] or k + "<" in r["Name"]:
                e = rows.setdefault(k, {"Calls": 0, "TotalDurationNs": 0})
                e["Calls"] += int(r["Calls"]); e["TotalDurationNs"] += int(r["TotalDurationNs"])
    ns = sum(int(r["TotalDurationNs"]) for r in rows.values())
    out["decode_kernels"] = {"source": "rocprofv3 --kernel-trace --stats, leg (c) once, a run of its own",
                             "kernels": {k: {"calls": int(r["Calls"]), "total_ms": int(r["TotalDurationNs"]) / 1e6} for k, r in rows.items()},
                             "total_ms": ns / 1e6, "postings_decoded": out.get("postings_decoded"),
                             "postings_per_s": (out["postings_decoded"] / (ns / 1e9)) if out.get("postings_decoded") and ns else None}
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out["decode_kernels"], indent=1))
    sys.exit(0)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import ctypes as C
import seekstorm_amd as S
from seekstorm_amd import _native as N
from oracle import textindex as TI

F, BOOST = 3, [2.0, 1.0, 0.5]
t0 = time.perf_counter()
T = TI.TextCorpus(11, args.docs, args.vocab, n_frequent=64, mean_len=100.0, topic_share=0.35, n_fields=F, longest_field=1)
data = T.write_index_bin(key_head_size=23)
whole = S.IndexBin(data, F, key_head_size=23)
terms_whole = int(whole.term_count)
whole.close()
ix = S.IndexBin(data, F, key_head_size=23, min_posting_count=args.min_postings)
out = {"docs": args.docs, "indexed_fields": F, "boost": BOOST, "index_bin_bytes": len(data), "postings_in_the_file": int(T.n_postings),
       "terms_in_the_file": terms_whole, "terms": int(ix.term_count), "levels": int(ix.level_count),
       "vocabulary_cut": "untiered; ss_index_bin_filter keeps the keys of at least %d postings" % args.min_postings,
       "write_and_walk_s": time.perf_counter() - t0, "cpus_visible": len(os.sched_getaffinity(0)),
       "loader_threads": int(os.environ.get("SS_LOADER_THREADS", 0)) or None}
print(out, flush=True)


def leg_a():
    sh = S.Shard(0)
    t = time.perf_counter()
    sh.upload_index_bin(ix, BOOST)
    dt = time.perf_counter() - t
    sh.close()
    return dt


def leg_open(mode, keep=False):
    sh = S.Shard(0)
    t = time.perf_counter()
    sh.open_index_bin_levels_fields(ix, BOOST, positions=mode)
    dt = time.perf_counter() - t
    info = sh.open_info()
    assert sh.incremental_info()[0] == ix.level_count and info[0] == (2 if mode else 0)
    if keep:
        return dt, sh, info
    sh.close()
    return dt, None, info


def leg_decode():
    a_, b_ = C.c_uint64(), C.c_uint64()
    t = time.perf_counter()
    N.check(N.lib().ss_index_bin_decode_stats(ix._h, 0, C.byref(a_), C.byref(b_)), "ss_index_bin_decode_stats")
    return time.perf_counter() - t, int(a_.value)


if args.only == "c":
    print("leg c:", leg_open(False)[0])
    sys.exit(0)

leg_a(); leg_open(False); leg_open("host"); leg_decode()  # warm-up, untimed
a, c, d, dec = [], [], [], []
for r in range(args.rounds):
    a.append(leg_a()); c.append(leg_open(False)[0]); d.append(leg_open("host")[0]); dec.append(leg_decode()[0])
    print(f"round {r}: (a) upload {a[-1]:.3f} s, (c) open mode 0 {c[-1]:.3f} s, (d) open mode 2 {d[-1]:.3f} s, host decode {dec[-1]:.3f} s", flush=True)
stat = lambda v: {"median_s": float(np.median(v)), "min_s": float(min(v)), "max_s": float(max(v)), "runs_s": [float(x) for x in v]}
out["a_upload_index_bin_fields"], out["c_open_levels_fields_mode_0"], out["d_open_levels_fields_mode_2"] = stat(a), stat(c), stat(d)
out["entries_decoded"] = leg_decode()[1]

# (b) the commits: the levels of an opened shard read back and turned into entries (untimed), committed one by one
_, src, info = leg_open(False, keep=True)
out["postings_decoded"] = info[1]  # merged entries (term, doc) the device decoded in leg (c)
nt = ix.term_count
levels = []
for l in range(ix.level_count):
    L = src.read_level_fields(l, 0, nt)
    rows, fields = np.nonzero(L["mtf"])  # row-major: (merged entry, field) = the order of a term's entries
    before = np.concatenate(([0], np.cumsum((L["mtf"] != 0).sum(axis=1))))
    levels.append((L["doclen"], before[L["moff"].astype(np.int64)].astype(np.uint64), L["mdoc"][rows], fields.astype(np.uint8), L["mtf"][rows, fields]))
src.close()
sh = S.Shard(0)
per = []
for l, (dl, o, dd, ff, tt) in enumerate(levels):
    t1 = time.perf_counter()
    sh.commit_level_fields(l, dl, BOOST, o, dd, ff, tt)
    per.append(time.perf_counter() - t1)
assert sh.incremental_info()[0] == ix.level_count
sh.close()
out["b_host_decode_then_commit_level_fields"] = {"decode": stat(dec), "commits_total_s": float(sum(per)), "commits_per_level_s": [float(x) for x in per],
                                                 "commit_runs": 1, "total_s": float(np.median(dec) + sum(per)),
                                                 "note": "decode = ss_index_bin_decode_stats without positions; the cut of the entries per level is not timed"}
spread = max(a) - min(a)
out["expectation"] = {"c_le_a_plus_spread": {"a_median_plus_spread_s": float(np.median(a) + spread), "c_median_s": float(np.median(c)),
                                             "holds": bool(np.median(c) <= np.median(a) + spread)},
                      "b_over_c": float((np.median(dec) + sum(per)) / np.median(c))}
print(json.dumps(out, indent=1))
json.dump(out, open(args.out, "w"), indent=1)
