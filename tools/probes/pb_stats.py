#!/usr/bin/env python3
"""Counters of the pruned kernel's sparse stage on the C2 batches (GPU; an experiment build with -DPB_STATS=1, csrc/bm25_probe_body.h):

    SS_OUT_DIR=$PWD/seekstorm_amd/lib_stats SS_HIPCC_FLAGS="-DPB_STATS=1" python -m seekstorm_amd.build                      # the two-phase body
    SS_OUT_DIR=$PWD/seekstorm_amd/lib_stats1 SS_HIPCC_FLAGS="-DPB_STATS=1 -DPB_TWO_PHASE=0" python -m seekstorm_amd.build   # the one-phase rule
    SEEKSTORM_HIP_LIB=$PWD/seekstorm_amd/lib_stats/libseekstorm_hip.so python tools/probes/pb_stats.py [batches] [docs]

Prints, per 1000-query batch (bench.py's rotation: batch 0 = make_c2_queries' default seed) and per query of it: entries pushed to the first
queue, entries that pass the sparse stage's bound, postings of the first probed list fetched, times a wave read its query's score histogram
(pb_publish_hist; a library from before the histogram leaves that counter at 0); then one JSON line with the means.  Each batch is searched
three times and the last launch is read: the counts depend on how the partitions' thresholds interleave."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    docs = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    import torch  # noqa: F401  (first: the HIP runtime torch loads is shared with the library)
    import seekstorm_amd as S
    from seekstorm_amd import _native as N
    from oracle import oracle as O
    import bench
    L = S.lib()
    if not hasattr(L, "ssi_dbg_pb_stats"):
        raise SystemExit("this library was built without -DPB_STATS=1")
    L.ssi_dbg_pb_stats.argtypes = [C.c_void_p]
    L.ssi_dbg_pb_stats.restype = C.c_int
    sh = S.Shard(0)
    lists0, th = bench.make_c2_queries(O, 1000)
    sh.synth_lexical(O.LEX_SEED, docs, th, O.len_table())
    rot = [lists0] + [bench.make_c2_queries(O, 1000, seed=5000 + i)[0] for i in range(1, nb)]
    rows = []
    for b, tl in enumerate(rot):
        q = sh.make_queries(tl, S.QueryType.Union)
        for _ in range(3):
            sh.search_lexical_batch(q, 10, S.ResultType.Topk, reference_shortcuts=False)
        out = np.zeros(4, np.uint64)
        N.check(L.ssi_dbg_pb_stats(out.ctypes.data_as(C.c_void_p)), "ssi_dbg_pb_stats")
        rows.append([int(x) for x in out])
        print(f"batch {b}: pushed {out[0]} ({out[0] / 1000:.0f} / query)  passed {out[1]} ({out[1] / 1000:.0f})  A postings {out[2]} ({out[2] / 1000:.0f})  histogram reads {out[3]} ({out[3] / 1000:.0f})", flush=True)
    m = np.mean(np.asarray(rows, np.float64), axis=0) / 1000.0
    print(json.dumps({"batches": nb, "docs": docs, "per_query_mean": {"pushed": m[0], "passed": m[1], "a_postings": m[2], "hist_reads": m[3]}, "per_batch": rows}))
    sh.close()


if __name__ == "__main__":
    main()
