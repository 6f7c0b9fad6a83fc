"""Point (geo) facets at coordinate, distance and Morton-range edges (-m gpu): every Point entry of the library over
tests/point_edge_world.py -- all four quadrants, five bases (north-east, south-west, the origin, near the pole, near the antimeridian),
km, miles and the sort key, docs exactly on the bases, families whose distances are the same bits on any machine, saturated and NaN
inputs, and filters whose Z-order range is empty, proper, or narrower than their circle.  Every answer is compared with
oracle/naive.py's geo_* restatement over the CPU oracle's match sets and scores (test_point_edge_world_cpu.py proves the world and the
checks); two device answers are compared with each other only where a test says so."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import point_edge_world as PW
from point_edge_world import BASES, HI, LO, N_DOCS, N_EXTRA, OFF

pytestmark = pytest.mark.gpu

UNITS = ("km", "miles", "sortkey")
KS = (1, 10, 64, 1030)


@pytest.fixture(scope="module")
def S():
    import seekstorm_amd
    return seekstorm_amd


def _upload(S, W, sh, records_in_levels=False):
    if records_in_levels:  # the first level, then the rest as a commit appends it; facets first, the lexical image second
        sh.upload_facets(W.raw[:65536])
        sh.append_facet_level(1, W.raw[65536:])
    else:
        sh.upload_facets(W.raw)
    sh.upload_lexical(N_DOCS, W.dl, W.offs, W.docs, W.tfs)
    sh.set_deleted(W.gone)


def _world(S):
    from oracle import oracle as O
    W = PW.build(O)
    W.sh = S.Shard(0)
    _upload(S, W, W.sh)
    return W


@pytest.fixture(scope="module")
def W(S):
    W = _world(S)
    yield W
    W.sh.close()


def _q(S, sh, W, qis):
    qt = lambda u: S.QueryType.Union if u else S.QueryType.Intersection
    return np.concatenate([sh.make_queries([W.queries[i][0]], qt(W.queries[i][1]), [W.queries[i][2]]) for i in qis])


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


# ------------------------------------------------------------------ values
def test_stored_codes_and_distances(S, W):
    """ss_facet_values: the stored codes bit for bit (both columns, the records beyond the image too); ss_facet_point_distances of every
    doc x B0..B4 x km / miles / sortkey: at most 16 ulp from the reference, more than 90 % bit-equal, and 0 ulp on the determined docs
    (the coincident ones among them)"""
    every = np.arange(N_DOCS + N_EXTRA, dtype=np.uint32)
    for col in ("loc", "loc2"):
        assert np.array_equal(W.sh.facet_values(every, OFF[col], "point"), W.rec[col]), col
        for bi, base in enumerate(BASES):
            det = PW.determined(W.rec[col][:N_DOCS], base)
            for unit in UNITS:
                got = W.sh.facet_point_distances(every[:N_DOCS], OFF[col], base, unit)
                u = _ulps(got, W.dist(col, bi, unit))
                print("distances", col, base, unit, "max ulp", int(u.max()), "bit-equal", float((u == 0).mean()), "determined max", int(u[det].max()) if det.any() else 0)
                assert u.max() <= 16 and (u == 0).mean() > 0.9, (col, base, unit, int(u.max()), float((u == 0).mean()))
                bad = np.nonzero(det & (u != 0))[0]
                assert len(bad) == 0, (col, base, unit, "determined docs differ", bad[:5], got[bad[:5]], W.dist(col, bi, unit)[bad[:5]])
                if col == "loc":
                    zero = W.dist(col, bi, unit) == 0.0
                    assert zero.sum() >= PW.N_COINCIDENT and np.all(got[zero].view(np.uint64) == 0)  # +0.0, not -0.0


# ------------------------------------------------------------------ filter
def _filter_cases(W):
    sd = PW.step_distance
    cases = [[PW.point_filter(W, "loc", *f)] for f in PW.Z_FILTERS + PW.EXACT_FILTERS]
    for fl in (0, HI, LO, LO | HI):  # the pivot form, ends on determined keys inside tie groups
        cases.append([PW.point_filter(W, "loc", 0, sd(5, "sortkey"), sd(20, "sortkey"), "sortkey", fl)])
        cases.append([PW.point_filter(W, "loc", 1, sd(7, "sortkey"), sd(7, "sortkey"), "sortkey", fl)])  # lo == hi
    cases.append([PW.point_filter(W, "loc", 2, 0.0, 0.0, "sortkey", HI)])             # distance 0 alone
    cases.append([PW.point_filter(W, "loc", 3, 0.0, np.inf, "sortkey", LO | HI)])      # everything but distance 0
    cases.append([PW.point_filter(W, "loc", 0, sd(20, "sortkey"), sd(5, "sortkey"), "sortkey", LO | HI)])  # lo > hi
    for fl in (HI, LO, LO | HI):
        cases.append([PW.point_filter(W, "loc", 0, PW.EXACT_FILTERS[0][1], PW.EXACT_FILTERS[0][2], "km", fl)])
    cases.append([PW.point_filter(W, "loc", 0, 0.0, 500.0, "km"), PW.h_filter(W, 1000, 30000)])
    cases.append([PW.point_filter(W, "loc", 1, 0.0, 1000.0, "km"), PW.point_filter(W, "loc2", *PW.LOC2_FILTERS[0])])
    cases.append([PW.point_filter(W, "loc2", *PW.LOC2_FILTERS[1]), PW.h_filter(W, 0, 40000), PW.point_filter(W, "loc", 4, 0.0, 100.0, "km")])
    return cases


H_BOUNDS = [0, 10000, 30000]


def run_filters(S, W, sh):
    """ss_bm25_search_filtered (all queries in one call, TopkCount and Count) and a filtered facet_count under every filter case: exact
    totals, the top-k rule on the hits, every hit passes.  -> the raw answers"""
    qis = list(range(len(W.queries)))
    qb = _q(S, sh, W, qis)
    raw = []
    for fs in _filter_cases(W):
        filt = [f for f, _ in fs]
        keep = np.logical_and.reduce([k for _, k in fs])
        for rt in (S.ResultType.TopkCount, S.ResultType.Count):
            doc, score, cnt, tot = sh.search_lexical_batch(qb, 10, rt, reference_shortcuts=False, facet_filter=filt)
            raw += [doc, score, cnt, tot]
            for qi in qis:
                md = W.matches[qi][0]
                assert int(tot[qi]) == int(keep[md].sum()), (filt, qi, rt, int(tot[qi]), int(keep[md].sum()))
                if rt != S.ResultType.Count:
                    PW.check_filtered(W, doc[qi], score[qi], cnt[qi], tot[qi], qi, keep, 10, (filt, qi))
        for qi in (3, 4):
            md = W.matches[qi][0]
            got = sh.facet_count(qb[qi:qi + 1], OFF["h"], "u16", range_lower_bounds=H_BOUNDS, facet_filter=filt)
            m = md[keep[md]]
            PW.check_counts(got, PW.want_counts_h(W, H_BOUNDS, m) + (len(m),), ("filtered count", filt, qi))
            raw += [got[0], np.array(got[1:])]
    return raw


def test_filters(S, W):
    run_filters(S, W, W.sh)


# ------------------------------------------------------------------ counts
def _point_qf(name, col, bi, unit, bounds, range_type="within"):
    return {"field": name, "type": "point", "offset": OFF[col], "ranges": [("%s%d" % (name, i), b) for i, b in enumerate(bounds)],
            "base": BASES[bi], "unit": unit, "range_type": range_type}


def _h_qf(range_type="within"):
    return {"field": "h", "type": "u16", "offset": OFF["h"], "ranges": [("h%d" % i, b) for i, b in enumerate(H_BOUNDS)], "range_type": range_type}


def finish_facets(*a):
    from seekstorm_amd.search import finish_facets as f
    return f(*a)


def merge_facets(*a):
    from seekstorm_amd.search import merge_facets as f
    return f(*a)


def _facet_sets():
    c = PW.COUNT_CASES
    # two Point facets of different bases, units and columns with a numeric facet in between; the same column under two bases
    return [[_point_qf("near", *c[0]), _h_qf(), _point_qf("far", *c[5])],
            [_point_qf("sw", *c[1], "above"), _h_qf("below"), _point_qf("sw2", *c[6], "below")],
            [_point_qf("origin", *c[2]), _point_qf("anti", *c[4]), _point_qf("pole", *c[3], "above")]]


def _want_facet(W, qf, docs):
    if qf["type"] == "point":
        bi = BASES.index(qf["base"])
        col = "loc" if qf["offset"] == OFF["loc"] else "loc2"
        c, o = PW.want_counts(W, col, bi, qf["unit"], [b for _, b in qf["ranges"]], docs)
    else:
        c, o = PW.want_counts_h(W, H_BOUNDS, docs)
    return c, o


def _check_per(W, qfs, per, row, docs, total, what):
    for f, qf in enumerate(qfs):
        c, o = _want_facet(W, qf, docs)
        PW.check_counts((per[f][row][:-1], per[f][row][-1], total), (c, o, len(docs)), what + (qf["field"],))


def run_counts(S, W, sh):
    """ss_bm25_facet_count_point, ss_bm25_search_facets, ss_bm25_search_sorted_facets and ss_docs_search with facets: every bucket,
    "other" and the total exact.  -> the raw answers"""
    raw = []
    hf = PW.h_filter(W, 1000, 30000)
    qis = list(range(len(W.queries)))
    qb = _q(S, sh, W, qis)
    for qi in (1, 3, 4, 5):
        md = W.matches[qi][0]
        for flt, keep in ((None, None), ([hf[0]], hf[1])):
            m = md if keep is None else md[keep[md]]
            for col, bi, unit, bounds in PW.COUNT_CASES:
                got = sh.facet_count(qb[qi:qi + 1], OFF[col], "point", range_lower_bounds=bounds, facet_filter=flt, base=BASES[bi], unit=unit)
                PW.check_counts(got, PW.want_counts(W, col, bi, unit, bounds, m) + (len(m),), ("facet_count", col, bi, unit, qi, flt is None))
                raw += [got[0], np.array(got[1:])]
    live = np.setdiff1d(np.arange(N_DOCS), W.gone)
    for qfs in _facet_sets():
        for flt, keep in ((None, None), ([hf[0]], hf[1])):
            doc, score, cnt, tot, per = sh.search_lexical_facets(qb, 10, qfs, S.ResultType.TopkCount, flt, reference_shortcuts=False)
            raw += [doc, score, cnt, tot] + per
            sd, ss, sc, st, sper = sh.search_lexical_sorted_facets(qb, [(OFF["h"], "u16", True)], 10, qfs, S.ResultType.TopkCount, flt)
            raw += [sd, ss, sc, st] + sper
            for qi in qis:
                md = W.matches[qi][0]
                m = md if keep is None else md[keep[md]]
                _check_per(W, qfs, per, qi, m, int(tot[qi]), ("search_facets", qi, flt is None))
                _check_per(W, qfs, sper, qi, m, int(st[qi]), ("search_sorted_facets", qi, flt is None))
            bd, bc, bt, bper = sh.search_docs_raw(10, S.ResultType.TopkCount, flt, None, qfs)
            m = live if keep is None else live[keep[live]]
            _check_per(W, qfs, [p[None, :] for p in bper], 0, m, bt, ("docs_search", flt is None))
            raw += [bd] + bper
            # the range types the wrapper knows, as the shard finishes them
            _, _, _, fac = sh.search_docs(10, S.ResultType.TopkCount, flt, None, qfs)
            want = finish_facets(qfs, [np.append(*_want_facet(W, qf, m)) for qf in qfs], 1)
            assert fac == want, ("docs_search facets", [qf["field"] for qf in qfs], fac, want)
    return raw


def test_counts(S, W):
    run_counts(S, W, W.sh)


# ------------------------------------------------------------------ pivot
def test_pivots(S, W):
    """ss_bm25_facet_kth_point, both directions, k = 1, inside and at both edges of the coincident group, the first docs beyond it (a
    +- pair's group), matches, matches + 1: n_better and n_equal exact, the value's bits exact where a determined doc holds the key"""
    for qi in (3, 4, 1, 0):
        q = _q(S, W.sh, W, [qi])
        md = W.matches[qi][0]
        for bi, base in enumerate(BASES):
            key = W.dist("loc", bi, "sortkey")[md] + 0.0
            det = W.det[bi][md]
            for desc in (False, True):
                order = np.sort(key)[::-1] if desc else np.sort(key)
                n, n0 = len(md), int((key == 0.0).sum())
                ks = {1, n, n + 1, n // 2}
                ks |= ({n0 // 2, n0, n0 + 1, n0 + 2, n0 + 13} if not desc else {n - n0 // 2, n - n0 + 1, n - n0, n - n0 - 1, n - n0 - 12}) if n0 else set()
                for k in sorted(x for x in ks if x >= 1):
                    p = order[min(k, n) - 1]
                    nb, ne = int((key > p).sum() if desc else (key < p).sum()), int((key == p).sum())
                    bits, gb, ge, tot = W.sh.facet_kth(q, OFF["loc"], "point", desc, k, base=base)
                    what = (qi, base, desc, k)
                    assert tot == n and (gb, ge) == (nb, ne), (what, (gb, ge), (nb, ne))
                    got = np.array([bits], np.uint64).view(np.float64)[0]
                    if det[key == p].any():
                        assert bits == int(np.array([p], np.float64).view(np.uint64)[0]), (what, got, p)
                    else:
                        assert _ulps(got, p) <= 16, (what, got, p)
    assert int((W.dist("loc", 0, "sortkey")[W.matches[3][0]] == 0.0).sum()) == PW.N_COINCIDENT


# ------------------------------------------------------------------ sort
SORTS = [[("loc", d, bi)] for bi in range(len(BASES)) for d in (False, True)]
SORTS2 = [[("loc", False, 0), ("h", True, None)], [("h", False, None), ("loc", True, 1)], [("loc", True, 2), ("h", False, None)]]


def run_sorts(S, W, sh, ks=KS):
    """ss_bm25_search_sorted: ascending and descending by distance to B0..B4, a Point field before and after a u16 field, under a u16 and
    under a Point filter, k = 1, 10, 64 and 1030 (a deep page whose pass boundary lies inside a determined tie group).  -> raw answers"""
    raw = []
    hf = PW.h_filter(W, 1000, 30000)
    pf = PW.point_filter(W, "loc", 1, 0.0, 1000.0, "km")
    plan = [(qi, srt, None) for qi in (3, 4) for srt in SORTS + SORTS2] + [(qi, srt, None) for qi in (0, 1, 2, 5, 6, 7) for srt in (SORTS[0], SORTS[3])]
    plan += [(3, SORTS[0], hf), (4, SORTS[2], pf), (4, SORTS2[0], hf)]
    for qi, srt, f in plan:
        q = _q(S, sh, W, [qi])
        ref = PW.reference_order(W, qi, srt, None if f is None else f[1])
        for k in ks:
            doc, score, tot = sh.search_lexical_sorted(q, PW.sort_spec(srt), k, facet_filter=None if f is None else [f[0]])
            PW.check_sorted(W, doc, score, tot, ref, srt, k, ("sorted", qi, srt, k, f is not None))
            raw += [doc, score]
    # all queries in one call
    qis = list(range(len(W.queries)))
    qb = _q(S, sh, W, qis)
    for srt in (SORTS[1], SORTS[8], SORTS2[1]):
        bd, bs, bc, bt = sh.search_lexical_sorted_batch(qb, PW.sort_spec(srt), 64)
        raw += [bd, bs, bc, bt]
        for qi in qis:
            PW.check_sorted(W, bd[qi][:bc[qi]], bs[qi][:bc[qi]], int(bt[qi]), PW.reference_order(W, qi, srt), srt, 64, ("sorted batch", qi, srt))
            assert np.all(bd[qi][bc[qi]:] == 0xFFFFFFFF)
    return raw


def test_sorts(S, W):
    run_sorts(S, W, W.sh)


def test_browse_sorted_by_distance(S, W):
    """ss_docs_search sorted by distance: every live doc, the key position by position, inside a tie group the larger doc id first (the
    smaller with doc_ascending); the records beyond the image never appear"""
    live = np.setdiff1d(np.arange(N_DOCS), W.gone)
    pf = PW.point_filter(W, "loc", 0, 0.0, 500.0, "km")
    for bi in range(len(BASES)):
        key = W.dist("loc", bi, "sortkey") + 0.0
        for desc, asc, f in ((False, False, None), (True, True, None), (False, True, pf)):
            m = live if f is None else live[f[1][live]]
            order = m[np.lexsort((m if asc else -m, -key[m] if desc else key[m]))]
            for k in (64, 1030):
                doc, cnt, tot, _ = W.sh.search_docs_raw(k, S.ResultType.TopkCount, None if f is None else [f[0]], [(OFF["loc"], "point", desc, BASES[bi])],
                                                        None, asc)
                what = ("browse", bi, desc, asc, k, f is not None)
                assert tot == len(m) and cnt == min(k, len(m)) and np.all(doc < N_DOCS), what
                assert np.array_equal(key[doc].view(np.uint64), key[order[:cnt]].view(np.uint64)), what
                same = key[doc][1:] == key[doc][:-1]
                d = doc.astype(np.int64)
                assert np.all((d[1:] > d[:-1])[same] if asc else (d[1:] < d[:-1])[same]), what


# ------------------------------------------------------------------ sorted with facets (fused and not)
def run_sorted_facets(S, W, sh):
    """ss_bm25_search_sorted_facets under a Point sort with Point facets: hits by check_sorted, counters exact.  -> raw answers"""
    raw = []
    qis = list(range(len(W.queries)))
    qb = _q(S, sh, W, qis)
    for srt, qfs, k in ((SORTS[0], _facet_sets()[0], 64), (SORTS[3], _facet_sets()[1], 10), (SORTS2[0], _facet_sets()[2], 10), (SORTS[5], _facet_sets()[0], 1030)):
        doc, score, cnt, tot, per = sh.search_lexical_sorted_facets(qb, PW.sort_spec(srt), k, qfs)
        raw += [doc, score, cnt, tot] + per
        for qi in qis:
            PW.check_sorted(W, doc[qi][:cnt[qi]], score[qi][:cnt[qi]], int(tot[qi]), PW.reference_order(W, qi, srt), srt, k, ("sorted facets", qi, srt, k))
            _check_per(W, qfs, per, qi, W.matches[qi][0], int(tot[qi]), ("sorted facets", qi))
    return raw


def test_sorted_with_facets(S, W):
    run_sorted_facets(S, W, W.sh)


def test_sorted_with_facets_with_the_fused_pass_switched_off():
    """the same checks in a child process under SS_SORT_FUSED=0 (the switch is read once per process)"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_point_edges as t; t.run_unfused()" % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SS_SORT_FUSED="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "unfused ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def run_unfused():
    import seekstorm_amd
    assert os.environ.get("SS_SORT_FUSED") == "0"
    W = _world(seekstorm_amd)
    try:
        run_sorted_facets(seekstorm_amd, W, W.sh)
    finally:
        W.sh.close()
    print("unfused ok")


# ------------------------------------------------------------------ per-query filters
def test_each_query_under_its_own_point_filter(S, W):
    """one ss_bm25_search_each call: neighbouring queries carry Point filters of different bases and units, one has no filter, one a
    filter that passes nothing -- unsorted with Point facets, and sorted by distance.  Every row is its own."""
    sets = PW.each_sets(W)
    qis = [3, 4] * 9  # the two queries that see every family, each under every set
    rows = [(qi, sets[(r // 2 + r % 2 * 4) % len(sets)]) for r, qi in enumerate(qis)]
    qb = _q(S, W.sh, W, qis)
    per_q = [[f for f, _ in fs] for _, fs in rows]
    keeps = [np.logical_and.reduce([k for _, k in fs]) if fs else np.ones(N_DOCS, bool) for _, fs in rows]
    qfs = _facet_sets()[0]
    doc, score, cnt, tot, per = W.sh.search_lexical_each(qb, 10, S.ResultType.TopkCount, per_q, None, qfs)
    for r, (qi, _) in enumerate(rows):
        md = W.matches[qi][0]
        PW.check_filtered(W, doc[r], score[r], cnt[r], tot[r], qi, keeps[r], 10, ("each", r))
        _check_per(W, qfs, per, r, md[keeps[r][md]], int(tot[r]), ("each", r))
    assert sum(int(t) == 0 for t in tot) == 2 and len({int(t) for t in tot}) > 10  # (the sets are what the CPU test shows them to be)
    srt = SORTS[8]
    doc, score, cnt, tot, _ = W.sh.search_lexical_each(qb, 64, S.ResultType.TopkCount, per_q, PW.sort_spec(srt), None)
    for r, (qi, _) in enumerate(rows):
        PW.check_sorted(W, doc[r][:cnt[r]], score[r][:cnt[r]], int(tot[r]), PW.reference_order(W, qi, srt, keeps[r]), srt, 64, ("each sorted", r))


# ------------------------------------------------------------------ the coalescer
def test_coalesced_callers_that_differ_in_base_or_unit(S, W):
    """8 threads in 6 barriered rounds of one-query faceted calls.  Rounds 0-2: the specs differ only in the Point facet's base; rounds
    3-4: only in its unit -- such callers must not share a batch's facet spec: each answer is the caller's answer alone (and the
    reference's).  Round 5: one base and unit, eight different filters: these callers still share batches."""
    sh = W.sh
    bounds = PW.COUNT_CASES[0][3]
    n_t, n_r = 8, 6

    def spec(t, r):
        if r < 3:
            return [_point_qf("d", "loc", (t + r) % len(BASES), "km", bounds)], None
        if r < 5:
            return [_point_qf("d", "loc", r - 3, ("km", "miles")[t % 2], bounds)], None
        return [_point_qf("d", "loc", 0, "km", bounds)], PW.h_filter(W, 1000 * t, 30000 + 1000 * t)

    qs = {t: _q(S, sh, W, [(3, 4, 2, 1)[t % 4]]) for t in range(n_t)}

    def call(t, r):
        qfs, f = spec(t, r)
        return sh.search_lexical_facets(qs[t], 10, qfs, S.ResultType.TopkCount, None if f is None else [f[0]], reference_shortcuts=False)

    sh.set_coalescing_faceted(0)
    alone = {(t, r): call(t, r) for t in range(n_t) for r in range(n_r)}
    for (t, r), a in alone.items():  # the answers alone are the reference's
        qfs, f = spec(t, r)
        md = W.matches[(3, 4, 2, 1)[t % 4]][0]
        _check_per(W, qfs, a[4], 0, md if f is None else md[f[1][md]], int(a[3][0]), ("alone", t, r))
    b0, q0 = sh.coalescing_stats_faceted()
    sh.set_coalescing_faceted(64, 50000)
    bar, got, errors, after = threading.Barrier(n_t), {}, [], {}

    def loop(t):
        try:
            for r in range(n_r):
                bar.wait()
                got[(t, r)] = call(t, r)
                bar.wait()
                if t == 0:
                    after[r] = sh.coalescing_stats_faceted()
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
            bar.abort()

    th = [threading.Thread(target=loop, args=(t,)) for t in range(n_t)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    sh.set_coalescing_faceted(0)
    assert not errors, errors[:3]
    for key, a in alone.items():
        g = got[key]
        n = int(a[2][0])
        assert n == int(g[2][0]) and int(a[3][0]) == int(g[3][0]) and np.array_equal(a[0][0][:n], g[0][0][:n]), key
        assert np.array_equal(a[1][0][:n].view(np.uint32), g[1][0][:n].view(np.uint32)), key
        assert all(np.array_equal(x, y) for x, y in zip(a[4], g[4])), (key, [x.tolist() for x in g[4]], [x.tolist() for x in a[4]])
    assert after[n_r - 1][1] - q0 == n_t * n_r
    # equal base and unit, different filters: the eight callers of the last round went out in fewer than eight batches
    assert after[5][1] - after[4][1] == n_t and 1 <= after[5][0] - after[4][0] < n_t, (after[4], after[5])


# ------------------------------------------------------------------ commits
def test_records_committed_level_by_level_answer_the_same(S, W):
    """the same records as ss_facet_upload of the first level plus ss_facet_append_level of the rest: the filter, count and sort checks
    once more, and every answer bit for bit the one upload's (two device answers compared: the one place it is the point)"""
    sh = S.Shard(0)
    try:
        _upload(S, W, sh, records_in_levels=True)
        assert sh.facet_info()[0] == N_DOCS + N_EXTRA
        for run in (run_filters, run_counts, lambda S_, W_, s: run_sorts(S_, W_, s, ks=(10, 1030))):
            a, b = run(S, W, W.sh), run(S, W, sh)
            assert len(a) == len(b) and all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))
    finally:
        sh.close()


# ------------------------------------------------------------------ two shards, both mirrors
def test_two_shards_sorted_by_distance_with_point_facets(S, W):
    """Index.search with a Point result_sort and Point query facets over the world split doc % 2, through the Python mirror and through
    the C++ mirror: the merged order and the summed counters are the whole world's reference, each doc scored with its own shard's
    statistics"""
    from oracle import oracle as O
    from test_gpu_sorted_facets import _cpp
    n_sh = 2
    parts = O.split_corpus(N_DOCS, W.dl, W.offs, W.docs, W.tfs, n_sh)
    shards, oshards = [], []
    saved = W.matches
    try:
        for sid, (nd, dl, o, d, t) in enumerate(parts):
            sh = S.Shard(0, shard_id=sid)
            sh.upload_lexical(nd, dl, o, d, t)
            sh.upload_facets(np.ascontiguousarray(W.raw[:N_DOCS][sid::n_sh]))
            shards.append(sh)
            oshards.append(O.Shard(nd, dl, o, d, t))
        idx = S.Index(shards)
        W.matches = []
        for terms, union, neg in W.queries:  # no tombstones here; scores from each shard's own statistics
            md, ms = [], []
            for sid, osh in enumerate(oshards):
                d, s_, _ = osh.search_exhaustive(terms, O.OP_OR if union else O.OP_AND, N_DOCS, neg)
                md.append(d.astype(np.int64) * n_sh + sid)
                ms.append(s_)
            md, ms = np.concatenate(md), np.concatenate(ms)
            o = np.lexsort((md, -ms.astype(np.float64)))
            W.matches.append((md[o], ms[o]))
        for qi in (3, 4, 1):
            terms, union, neg = W.queries[qi]
            qt = S.QueryType.Union if union else S.QueryType.Intersection
            md = W.matches[qi][0]
            for srt, qfs in ((SORTS[0], _facet_sets()[0]), (SORTS[3], _facet_sets()[2]), (SORTS2[0], _facet_sets()[0])):
                ref = PW.reference_order(W, qi, srt)
                want = merge_facets(qfs, [finish_facets(qfs, [np.append(*_want_facet(W, qf, md[md % n_sh == sid])) for qf in qfs], n_sh)
                                                   for sid in range(n_sh)])
                whole = finish_facets(qfs, [np.append(*_want_facet(W, qf, md)) for qf in qfs], n_sh)
                assert {k_: sorted(v) for k_, v in want.items() if v} == {k_: sorted(v) for k_, v in whole.items()}  # summed = the whole world's
                for off_, length in ((0, 10), (0, 64), (5, 1025)):
                    sub = (ref[0][off_:], ref[1][off_:], ref[2])
                    n = min(length, max(len(md) - off_, 0))
                    ro = idx.search(terms, None, qt, S.SearchMode.Lexical, off_, length, strict=True, not_terms=neg, result_sort=PW.sort_spec(srt),
                                    query_facets=qfs)
                    what = ("index", qi, srt, off_, length)
                    PW.check_sorted(W, [r.doc_id for r in ro.results], [r.score for r in ro.results], ro.result_count_total, sub, srt, n, what)
                    assert {k_: sorted(v) for k_, v in ro.facets.items() if v} == {k_: sorted(v) for k_, v in want.items() if v}, what
                    if not neg:
                        cd, cs, ctot, cfac = _cpp(shards, "both", terms, qt, off_, length, S.ResultType.TopkCount, PW.sort_spec(srt), qfs, None, 0)
                        PW.check_sorted(W, cd, cs, ctot, sub, srt, n, ("c++",) + what)
                        assert {k_: sorted(v) for k_, v in cfac.items() if v} == {k_: sorted(v) for k_, v in want.items() if v}, ("c++",) + what
    finally:
        W.matches = saved
        for sh in shards:
            sh.close()
