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
--positions: the POSITIONS leg instead, on the same index (every index.bin carries positions), into profiles/open_levels_positions_time.json:
  (2) ss_bm25_open_index_bin_levels, SS_OPEN_POSITIONS_HOST    -- unchanged code: the parent commit's open with positions
  (3) ss_bm25_open_index_bin_levels, SS_OPEN_POSITIONS_DEVICE  -- positions decoded on the device
one untimed warm-up round, then --rounds rounds alternating (2) and (3); median (min .. max); "mode_1_takes_device" is the rule the
library's SS_OPEN_POSITIONS follows: the device path unless its median is above (2)'s by more than (2)'s own spread (max - min).  In
the same run one shard opened in mode 3 answers a phrase set (pairs and triples of the most frequent dense terms, pairs with the most
frequent rare terms) exactly as one opened in mode 2.  --positions --only 3: mode 3 once (for a kernel trace in a run of its own);
--positions --kernel-stats CSV adds that trace's rows of the decode, scan and position kernels.
    python tools/probes/open_levels_time.py [--out FILE] [--docs 1000000] [--rounds 5] [--only b] [--kernel-stats CSV] [--positions]"""
import argparse, json, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--vocab", type=int, default=1_000_000)
ap.add_argument("--dense-min", type=int, default=1000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--only", default="")
ap.add_argument("--kernel-stats", default="")
ap.add_argument("--positions", action="store_true")
args = ap.parse_args()
args.out = args.out or os.path.join(HERE, "..", "..", "profiles", "open_levels_positions_time.json" if args.positions else "open_levels_time.json")
KERNELS = ("rbd_flat_kernel", "rbd_wg_kernel")
if args.positions:
    KERNELS += ("rbd_scan_sums_kernel", "rbd_scan_tiles_kernel", "rbd_scan_write_kernel", "rbd_tpos_kernel", "rbd_guard_kernel", "rbd_pos_kernel",
                "rbd_pos_long_kernel", "rbd_tier_gather_kernel")
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
    out["decode_kernels"] = {"source": "rocprofv3 --kernel-trace --stats, %s once, a run of its own" % ("mode 3" if args.positions else "leg (b)"),
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
       "levels": int(ix.level_count), "dense_min": args.dense_min, "positions": bool(args.positions), "write_and_walk_s": time.perf_counter() - t0,
       "cpus_visible": len(os.sched_getaffinity(0)), "loader_threads": int(os.environ.get("SS_LOADER_THREADS", 0)) or None}
a_, b_ = C.c_uint64(), C.c_uint64()
N.check(N.lib().ss_index_bin_decode_stats(ix._h, 0, C.byref(a_), C.byref(b_)), "ss_index_bin_decode_stats")
out["postings_decoded"] = int(a_.value)  # (an n-gram key's postings once per component term)
print(out, flush=True)


def leg_positions(mode, keep=False):
    sh = S.Shard(0)
    t = time.perf_counter()
    sh.open_index_bin_levels(ix, positions=mode)
    dt = time.perf_counter() - t
    info = sh.open_info()
    assert sh.incremental_info()[0] == ix.level_count and info[0] == {"host": 2, "device": 3}[mode]
    if keep:
        return dt, sh, info
    sh.close()
    return dt, None, info


if args.positions:
    if args.only == "3":
        print("mode 3:", leg_positions("device")[0])
        sys.exit(0)
    leg_positions("host"); leg_positions("device")  # warm-up, untimed
    h, d = [], []
    for r in range(args.rounds):
        h.append(leg_positions("host")[0]); d.append(leg_positions("device")[0])
        print(f"round {r}: mode 2 (host) {h[-1]:.3f} s, mode 3 (device) {d[-1]:.3f} s", flush=True)
    stat = lambda v: {"median_s": float(np.median(v)), "min_s": float(min(v)), "max_s": float(max(v)), "runs_s": [float(x) for x in v]}
    out["mode_2_host"], out["mode_3_device"] = stat(h), stat(d)
    spread = max(h) - min(h)
    out["mode_1_takes_device"] = {"rule": "mode 3's median <= mode 2's median + mode 2's spread (max - min)",
                                  "mode_2_median_plus_spread_s": float(np.median(h) + spread), "mode_3_median_s": float(np.median(d)),
                                  "holds": bool(np.median(d) <= np.median(h) + spread)}
    # one shard of each mode: the same counts, the same answers to a phrase set
    _, sh2, info2 = leg_positions("host", keep=True)
    _, sh3, info3 = leg_positions("device", keep=True)
    out["position_counts"] = {"decoded_on_the_device": info3[2], "brought_by_the_host_decoder": info2[3], "postings_decoded_on_the_device": info3[1]}
    assert info3[2] == info2[3] and info3[3] == 0
    df = np.asarray(sh2.posting_count(np.arange(ix.term_count, dtype=np.uint32)), np.int64)
    top = [int(t) for t in np.argsort(-df[:n_dense])[:12]]
    rare = [int(n_dense + t) for t in np.argsort(-df[n_dense:])[:4]]
    phrases = [[a, b] for a, b in zip(top, top[1:])] + [[b, a] for a, b in zip(top, top[1:])] + [list(top[i:i + 3]) for i in range(0, 9, 3)] + \
        [[top[i], r] for i, r in enumerate(rare)] + [[r, top[i]] for i, r in enumerate(rare)]
    ans = [s.search_lexical_batch(s.make_queries(phrases, S.QueryType.Phrase), 10, S.ResultType.TopkCount) for s in (sh2, sh3)]
    same = all(np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else x, np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else y)
               for x, y in zip(*ans))
    out["phrase_set"] = {"phrases": len(phrases), "matching_docs": int(np.asarray(ans[0][3]).sum()), "mode_3_equals_mode_2": bool(same)}
    sh2.close(); sh3.close()
    print(json.dumps(out, indent=1))
    json.dump(out, open(args.out, "w"), indent=1)
    assert same, "a shard opened in mode 3 answers the phrase set differently from one opened in mode 2"
    sys.exit(0)


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
