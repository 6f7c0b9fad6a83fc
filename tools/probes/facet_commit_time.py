"""What a host pays at a commit for the side images, O(change) against O(shard): facet records, string ranks, tombstones -- and the
numeric result sort, whose field table gained a base per field.  At 16 and at 153 levels of 65 536 docs of a 24-byte record:
  new   -- one ss_facet_append_level into reserved room; one that has to grow the image; ss_facet_set_string_ranks with 65 536 ids;
           ss_add_deleted of 1 and of 1 000 docs onto a set of 10^5
  base  -- what the same steps cost without those entries: ss_facet_upload of everything committed; string_facet_rank_column +
           ss_facet_upload; ss_set_deleted of the union; and a batch of sorted searches by a numeric field (measured on both sides)
Median of --runs runs (after one warm-up run of every step) and the spread (max - min), merged into the JSON file, so that a run on the parent checkout adds its series:
    python tools/probes/facet_commit_time.py --what new,base [--tag TEXT] [--root CHECKOUT] [--out FILE] [--runs 3] [--levels 16,153]"""
import argparse, json, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--what", default="new,base")
ap.add_argument("--tag", default="")
ap.add_argument("--root", default=os.path.join(HERE, "..", ".."))
ap.add_argument("--out", default=os.path.join(HERE, "..", "..", "profiles", "facet_commit_time.json"))
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--levels", default="16,153")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import seekstorm_amd as S
from seekstorm_amd import _native as N

LVL, RS, S16_OFF, N_IDS = 65536, 24, 8, 65536
WHAT = [w for w in args.what.split(",") if w]
SIZES = [int(x) for x in args.levels.split(",")]
L = N.lib()


def records(n_levels):
    """[n_levels + 1 levels][24 bytes]: i32, f32, string16 (ids below 65 536), string32, u16, Point -- the content is irrelevant to the cost"""
    return np.random.default_rng(n_levels).integers(0, 256, ((n_levels + 1) * LVL, RS), dtype=np.uint8)


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


series = {}
RUNS = args.runs + 1  # one warm-up run of every step


def record(name, runs, warm=1):
    a = np.asarray(runs[warm:], np.float64)  # the first run of a step loads code objects and touches fresh pages: not counted
    series[name + (" (" + args.tag + ")" if args.tag else "")] = {"median_ms": round(float(np.median(a)), 3), "spread_ms": round(float(a.max() - a.min()), 3),
                                                                  "runs_ms": [round(float(x), 3) for x in a]}
    print("%-72s %9.3f ms (spread %.3f)" % (name, np.median(a), a.max() - a.min()), flush=True)


strings = ["v%05d" % ((i * 40503) % N_IDS) for i in range(N_IDS)]
for nl in SIZES:
    rec = records(nl)
    head, level = rec[:nl * LVL], rec[nl * LVL:]
    if "new" in WHAT:
        rank = S.Shard.string_ranks(strings)
        runs_res, runs_grow, runs_rank = [], [], []
        for r in range(RUNS):
            sh = S.Shard(0)
            sh.reserve_facets((nl + 1) * LVL)
            for lv in range(nl):
                sh.append_facet_level(lv, head[lv * LVL:(lv + 1) * LVL])
            assert sh.facet_info() == (nl * LVL, RS, (nl + 1) * LVL, 0)
            runs_rank.append(timed(lambda: N.check(L.ss_facet_set_string_ranks(sh._h, S16_OFF, N.FACET_TYPES["string16"], N_IDS, N.ptr(rank, N.u32p)), "ranks")))
            L.ss_facet_set_string_ranks(sh._h, S16_OFF, N.FACET_TYPES["string16"], 0, None)
            runs_res.append(timed(lambda: sh.append_facet_level(nl, level)))
            assert sh.facet_info()[:3] == ((nl + 1) * LVL, RS, (nl + 1) * LVL)
            sh.close()
            sh = S.Shard(0)
            sh.upload_facets(head)
            runs_grow.append(timed(lambda: sh.append_facet_level(nl, level)))
            assert sh.facet_info()[2] == nl * LVL + nl * LVL // 2
            sh.close()
        record("ss_facet_append_level into reserved room, level %d" % nl, runs_res)
        record("ss_facet_append_level growing the image, level %d" % nl, runs_grow)
        record("ss_facet_set_string_ranks, 65 536 ids, %d levels" % nl, runs_rank)
    if "base" in WHAT:
        runs_up, runs_col = [], []
        for r in range(RUNS):
            sh = S.Shard(0)
            sh.upload_facets(head)
            runs_up.append(timed(lambda: sh.upload_facets(rec)))

            def rank_column_and_upload():
                raw, _ = S.Shard.string_facet_rank_column(head, S16_OFF, "string16", strings)
                sh.upload_facets(raw)
            runs_col.append(timed(rank_column_and_upload))
            sh.close()
        record("ss_facet_upload of everything committed, %d + 1 levels" % nl, runs_up)
        record("string_facet_rank_column + ss_facet_upload, %d levels" % nl, runs_col)

# tombstones: a set of 10^5 of 10 M docs, then 1 / 1 000 more
rng = np.random.default_rng(3)
base_set = rng.choice(10_000_000, 100_000, replace=False).astype(np.uint64)
more = {1: np.array([9_999_999], np.uint64), 1000: rng.choice(10_000_000, 1000, replace=False).astype(np.uint64)}
for n_more, ids in more.items():
    if "new" in WHAT:
        runs = []
        for r in range(RUNS):
            sh = S.Shard(0)
            sh.set_deleted(base_set)
            runs.append(timed(lambda: sh.add_deleted(ids)))
            sh.close()
        record("ss_add_deleted of %d onto a set of 10^5" % n_more, runs)
    if "base" in WHAT:
        union = np.concatenate([base_set, ids])
        runs = []
        for r in range(RUNS):
            sh = S.Shard(0)
            sh.set_deleted(base_set)
            runs.append(timed(lambda: sh.set_deleted(union)))
            sh.close()
        record("ss_set_deleted of the union, 10^5 + %d" % n_more, runs)

# the numeric sort: a batch of queries sorted by (an i32 field descending, a u16 field ascending) over 1 M docs, the same shard and queries on either side
if "base" in WHAT or "new" in WHAT:
    n_docs = 1_000_000
    rng = np.random.default_rng(4)
    offs, docs, tfs = [0], [], []
    for df in (0.3, 0.2, 0.1, 0.05, 0.02, 0.01):
        d = np.sort(rng.choice(n_docs, int(df * n_docs), replace=False)).astype(np.uint32)
        docs.append(d); tfs.append(np.minimum(rng.geometric(0.6, len(d)), 60).astype(np.uint16)); offs.append(offs[-1] + len(d))
    sh = S.Shard(0)
    sh.upload_lexical(n_docs, rng.integers(8, 90, n_docs).astype(np.uint8), np.asarray(offs, np.uint64), np.concatenate(docs), np.concatenate(tfs))
    sh.upload_facets(records(15)[:n_docs])
    qs = sh.make_queries([[int(a), int(b)] for a, b in rng.integers(0, 6, (64, 2)) if a != b] or [[0, 1]], S.QueryType.Union)
    spec = [(0, "i32", True), (4, "u16", False)]
    sh.search_lexical_sorted_batch(qs, spec, 10)
    for rep in range(3):  # three series of --runs x 20 calls: the run-to-run spread of the same code
        runs = [timed(lambda: [sh.search_lexical_sorted_batch(qs, spec, 10) for _ in range(20)]) / 20 for r in range(max(args.runs, 3))]
        record("ss_bm25_search_sorted, %d queries by two numeric fields, 1 M docs, series %d" % (len(qs), rep), runs, warm=0)
    sh.close()

out = {}
if os.path.exists(args.out):
    out = json.load(open(args.out))
out.setdefault("config", {"level_docs": LVL, "record_size": RS, "levels": SIZES, "string_ids": N_IDS, "runs": args.runs,
                          "unit": "ms of wall time of the call(s) named, host pointers in, median of the runs and max - min"})
out.setdefault("series", {}).update(series)
json.dump(out, open(args.out, "w"), indent=1)
print("wrote", os.path.abspath(args.out))
