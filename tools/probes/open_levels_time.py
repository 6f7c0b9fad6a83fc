"""What it costs to open index.bin level by level, decoded on the device (ss_bm25_open_index_bin_levels), beside the whole-image open that
decodes on the host (ss_bm25_upload_index_bin), on the text-shaped index of tools/real_format.py (oracle/ss_textindex.c writer; --docs docs,
tiered at --dense-min), without positions, in one process:
  (a) ss_bm25_upload_index_bin            -- unchanged code: the parent commit's time
  (b) ss_bm25_open_index_bin_levels       -- the new entry
  (c) every level through commit_level    -- the route a host had before to an image it can commit to (one run)
One untimed warm-up round, then --rounds rounds alternating (a) and (b); the host clock around calls that end in a synchronise.  With
SS_LOAD_TRACE=1 in the environment the library's own splits go to stderr.  SS_LOADER_THREADS sets the host decoder's worker threads
(leg (a) decodes on them; the library otherwise takes what the machine shows): the JSON records it.  --only b: leg (b) once and nothing
else (for a kernel trace of the decode kernels in a run of its own); --kernel-stats CSV: adds that trace's rows of the decode kernels
(rocprofv3 --kernel-trace --stats) to the JSON at --out and does nothing else.
    python tools/probes/open_levels_time.py [--out FILE] [--docs 1000000] [--rounds 5] [--only b] [--kernel-stats CSV]"""
import argparse, json, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "open_levels_time.json"))
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--vocab", type=int, default=1_000_000)
ap.add_argument("--dense-min", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--only", default="")
ap.add_argument("--kernel-stats", default="")
args = ap.parse_args()
if args.kernel_stats:
    import csv
    out = json.load(open(args.out))
    rows = {k: r for r in csv.DictReader(open(args.kernel_stats)) for k in ("rbd_flat_kernel", "rbd_wg_kernel") if k + "(" in r["Name"]}
    ns = sum(int(r["TotalDurationNs"]) for r in rows.values())
    out["decode_kernels"] = {"source": "rocprofv3 --kernel-trace --stats, leg (b) once, a run of its own",
                             "kernels": {k: {"calls": int(r["Calls"]), "total_ms": int(r["TotalDurationNs"]) / 1e6} for k, r in rows.items()},
                             "total_ms": ns / 1e6, "postings_decoded": out.get("postings_decoded"),
                             "postings_per_s": (out["postings_decoded"] / (ns / 1e9)) if out.get("postings_decoded") else None,
                             "file_bytes_read": out["index_bin_bytes"]}
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out["decode_kernels"], indent=1))
    sys.exit(0)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
import ctypes as C
import seekstorm_amd as S
from seekstorm_amd import _native as N
from oracle import textindex as TI

t0 = time.perf_counter()
T = TI.TextCorpus(11, args.docs, args.vocab, n_frequent=64, mean_len=100.0, topic_share=0.35, n_fields=1, longest_field=0)
data = T.write_index_bin(key_head_size=23)
ix = S.IndexBin(data, 1, key_head_size=23)
n_dense = ix.tier(args.dense_min)
out = {"docs": args.docs, "index_bin_bytes": len(data), "postings": int(T.n_postings), "terms": int(ix.term_count), "dense_terms": int(n_dense),
       "levels": int(ix.level_count), "dense_min": args.dense_min, "positions": False, "write_and_walk_s": time.perf_counter() - t0,
       "cpus_visible": len(os.sched_getaffinity(0)), "loader_threads": int(os.environ.get("SS_LOADER_THREADS", 0)) or None}
a_, b_ = C.c_uint64(), C.c_uint64()
N.check(N.lib().ss_index_bin_decode_stats(ix._h, 0, C.byref(a_), C.byref(b_)), "ss_index_bin_decode_stats")
out["postings_decoded"] = int(a_.value)  # (an n-gram key's postings once per component term)
print(out, flush=True)


def leg_a():
    sh = S.Shard(0)
    t = time.perf_counter()
    sh.upload_index_bin(ix)
    dt = time.perf_counter() - t
    sh.close()
    return dt


def leg_b():
    sh = S.Shard(0)
    t = time.perf_counter()
    sh.open_index_bin_levels(ix)
    dt = time.perf_counter() - t
    assert sh.incremental_info()[0] == ix.level_count
    sh.close()
    return dt


if args.only == "b":
    print("leg b:", leg_b())
    sys.exit(0)

leg_a(); leg_b()  # warm-up, untimed
a, b = [], []
for r in range(args.rounds):
    a.append(leg_a()); b.append(leg_b())
    print(f"round {r}: upload_index_bin {a[-1]:.3f} s, open_index_bin_levels {b[-1]:.3f} s", flush=True)
stat = lambda v: {"median_s": float(np.median(v)), "min_s": float(min(v)), "max_s": float(max(v)), "runs_s": [float(x) for x in v]}
out["upload_index_bin"], out["open_index_bin_levels"] = stat(a), stat(b)
spread = max(a) - min(a)
out["expectation_b_le_a_plus_spread"] = {"a_median_plus_spread_s": float(np.median(a) + spread), "b_median_s": float(np.median(b)),
                                         "holds": bool(np.median(b) <= np.median(a) + spread)}

# (c) the levels of the same index through commit_level: the postings decoded on the host (untimed), cut per level (untimed), committed
offs, docs, tfs = ix.decode_all()
nt = ix.term_count
term = np.repeat(np.arange(nt, dtype=np.uint32), np.diff(offs).astype(np.int64))
lvl = (docs >> 16).astype(np.uint16)
levels = []
for l in range(ix.level_count):
    m = lvl == l
    o = np.zeros(nt + 1, np.uint64)
    o[1:] = np.cumsum(np.bincount(term[m], minlength=nt))
    levels.append((o, docs[m], tfs[m]))
del term, lvl
# the levels' length bytes as the file holds them (level header: 65 536 bytes in front of the two u64 counters)
buf = np.frombuffer(data, np.uint8)
dl_levels, pos = [], 4 + 2
for l in range(ix.level_count):
    n = min(65536, args.docs - l * 65536)
    dl_levels.append(buf[pos:pos + n].copy())
    pos += 65536 + 16
    tbl = np.frombuffer(data, "<u4", 2 * 2048, pos).reshape(2048, 2)
    pos += 2048 * 8 + int(tbl[:, 0].astype(np.int64).sum())
sh = S.Shard(0)
per = []
t_all = time.perf_counter()
for l, (o, d, t) in enumerate(levels):
    t1 = time.perf_counter()
    sh.commit_level(l, dl_levels[l], o, d, t, n_dense)
    per.append(time.perf_counter() - t1)
c = time.perf_counter() - t_all
assert sh.incremental_info()[0] == ix.level_count
sh.close()
out["all_levels_through_commit_level"] = {"total_s": float(c), "per_level_s": [float(x) for x in per], "runs": 1,
                                          "note": "host decode and the cut per level are not in this time"}
out["ratio_c_over_b"] = float(c / np.median(b))
print(json.dumps(out, indent=1))
json.dump(out, open(args.out, "w"), indent=1)
