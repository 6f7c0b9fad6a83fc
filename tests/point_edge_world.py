"""The Point (geo) edge world: one seeded corpus whose Point facets sit where distance, sign and Z-order code go wrong, and the checks
that compare any answer over it with oracle/naive.py's geo_* restatement.  Pure numpy: importable, and proven, without a GPU
(test_point_edge_world_cpu.py); test_gpu_point_edges.py drives every Point entry of the library through it.

70 003 docs (one 65 536-doc level and a partial last 64-doc group), five terms from ~20 matches to most of the corpus, a few tombstones,
and a packed 19-byte facet record: Point `loc` at offset 1, u16 `h` at 9, a second Point `loc2` at 11.  40 records beyond the lexical
image sit exactly on the bases.  `loc` holds, at doc ids drawn from the matches of terms 3 AND 4 (so every large query sees all of it):
  coincident   32 docs exactly on each base: distance 0, key +0.0
  meridian     B0, B1: the base's longitude, latitude +-i/128 deg (i = 1..50, 12 docs a side): x is exactly 0
  mirror       B0, B1, B2: latitude -base.lat, longitude +-i/128 deg (i = 1..20, 4 docs a side): cos(0) = 1
  axes         lat or lon exactly 0, +-1e-7 (codes 1, 2 and their negative counterparts), one doc per quadrant next to the origin
  extremes     (+-90, +-180), inputs beyond the i32 range (they saturate), NaN inputs (code 0)
  zrange       per filter of Z_FILTERS: docs inside the distance range but outside [m0, m1), docs inside [m0, m1) but outside the
               distance range, a doc on m0 and a doc on m1
Everything else is the cloud, uniform over the globe.  i/128 deg times 1e7 is an integer and base +- i/128 a binary fraction, so the
+- pairs of a family decode to exactly mirrored coordinates and tie bit for bit.

DETERMINED docs of a base (determined()): the decoded longitude equals the base's (x = 0 * cos = 0) or the decoded latitude is minus the
base's (cos(0) = 1).  Their distances and keys are chains of single correctly rounded IEEE operations -- the same bits on any machine.
All other distances pass through cos and may differ in the last places between libraries; the builder re-draws cloud docs until
  * every non-determined doc's sort key is bit-equal to or more than CLEAR (1e-9, relative) away from every other doc's, per base
    (ORIGIN_CLEAR, 1e-10, between two docs of the origin's cluster: see there);
  * every non-determined doc's km / miles distance is more than CLEAR away from every filter end and count bound in use (IN_USE)
-- so a 16-ulp difference (3.6e-15) can move no doc across a bound and swap no two docs of a sort."""
import numpy as np

from oracle import naive

N_DOCS, N_EXTRA = 70_003, 40
DFS = [0.0003, 0.004, 0.04, 0.3, 0.85]  # df / N of terms 0..4
REC = np.dtype([("pad", "u1"), ("loc", "<u8"), ("h", "<u2"), ("loc2", "<u8")])
OFF = {n: REC.fields[n][1] for n in REC.names}
BASES = [(12.5, 40.0), (-33.25, -70.5), (0.0, 0.0), (89.5, 10.0), (10.0, 179.5)]  # B0 north-east, B1 south-west, B2, B3 pole, B4 antimeridian
CLEAR = 1e-9
# The five docs on and one coordinate step (1e-7 deg) beside the origin cannot be CLEAR apart seen from a base 70 deg away: their keys differ
# by 2 * 1e-7 / 70 = 3e-9 relative at the very best, and by less where the step runs across the line of sight.  Among themselves they are
# held to this figure instead (the smallest gap is 1.25e-10, B3's view of the two longitude steps): 2.8e4 times the 16-ulp band.
ORIGIN_CLEAR = 1e-10
HI, LO = naive.FACET_HI_INCLUSIVE, naive.FACET_LO_EXCLUSIVE
N_COINCIDENT, MERIDIAN_I, MERIDIAN_REP, MIRROR_I, MIRROR_REP = 32, 50, 12, 20, 4
FAMILIES = ["cloud", "coincident", "meridian", "mirror", "axes", "extremes", "zrange"]
RADIUS = {"km": naive.GEO_EARTH_KM, "miles": naive.GEO_EARTH_MI}


def step_distance(i, unit):
    """the determined distance of a meridian doc i/128 deg from its base: R * sqrt(y * y), y = DEG2RAD * (i / 128); "sortkey": the key
    (i / 128)^2"""
    if unit == "sortkey":
        return float(np.float64(i / 128.0) * np.float64(i / 128.0))
    y = np.float64(naive.GEO_DEG2RAD) * np.float64(i / 128.0)
    return float(np.float64(RADIUS[unit]) * np.sqrt(y * y))


# (base index, lo, hi, unit): the filters whose Z-order range is part of the case
Z_FILTERS = [(0, 0.0, 500.0, "km"), (0, 100.0, 300.0, "miles"), (1, 0.0, 1000.0, "km"), (1, 50.0, 400.0, "miles"),
             (2, 0.0, 500.0, "km"),      # the box crosses both zero axes: m0 > m1, nothing passes
             (3, 0.0, 3.32, "km"),       # towards the pole the circle is wider than the box, and lon + delta ends just below 2^27 * 1e-7
                                         # deg: docs inside the circle beyond that side have a code above m1
             (4, 0.0, 4000.0, "miles"),  # lon + delta saturates, lat - delta is negative: m0 > m1
             (4, 0.0, 100.0, "km")]      # a proper range that ends beyond lon 180
# ends exactly on determined distances of B0's / B1's meridian family
EXACT_FILTERS = [(0, step_distance(5, "km"), step_distance(20, "km"), "km"), (0, step_distance(7, "miles"), step_distance(7, "miles"), "miles"),
                 (0, step_distance(20, "km"), step_distance(5, "km"), "km"), (1, 0.0, step_distance(33, "miles"), "miles"),
                 (1, step_distance(50, "km"), 600.0, "km")]
# (column, base index, unit, lower bounds of the distance ranges)
COUNT_CASES = [("loc", 0, "km", [0.0, step_distance(10, "km"), 500.0, 2000.0, 10000.0, 1.0e5]),  # from 0; a determined bound; one above all
               ("loc", 1, "miles", [50.0, 1000.0, 5000.0]),                                     # from above 0: distance 0 is "other"
               ("loc", 2, "km", [0.0, 1.0, 1000.0, 1.0e5]),
               ("loc", 3, "miles", [0.0, 2000.0, 6000.0]),
               ("loc", 4, "miles", [0.0, 100.0, 3000.0]),
               ("loc2", 3, "miles", [10.0, 2000.0, 6000.0]),
               ("loc2", 1, "km", [0.0, 3000.0, 9000.0])]
LOC2_FILTERS = [(1, 100.0, 3000.0, "km"), (3, 0.0, 3000.0, "miles")]  # over the second column: a proper Z range, an empty one


def in_use():
    """{(column, base index, unit): every filter end and count bound the GPU tests hand to the library}"""
    u = {}
    for bi, lo, hi, unit in Z_FILTERS + EXACT_FILTERS:
        u.setdefault(("loc", bi, unit), set()).update((lo, hi))
    for bi, lo, hi, unit in LOC2_FILTERS:
        u.setdefault(("loc2", bi, unit), set()).update((lo, hi))
    for col, bi, unit, bounds in COUNT_CASES:
        u.setdefault((col, bi, unit), set()).update(bounds)
    return {key: sorted(v) for key, v in u.items()}


IN_USE = in_use()


class World:
    def dist(self, col, bi, unit):
        """the reference distance of every doc's `col` to base bi (cached)"""
        key = (col, bi, unit)
        if key not in self._dist:
            self._dist[key] = naive.geo_distance(self.rec[col][:N_DOCS], BASES[bi], unit)
        return self._dist[key]


def determined(codes, base):
    lat, lon = naive.geo_decode(codes)
    return (lon == base[1]) | (lat == -base[0])


def origin_cluster(codes):
    """the docs one coordinate step (1e-7 deg) or less from the origin"""
    lat, lon = naive.geo_decode(codes)
    return (np.abs(lat) <= 1e-7) & (np.abs(lon) <= 1e-7)


def z_cases(base, lo, hi, unit):
    """candidate codes of one filter from a grid over 1.3 x its box: (inside the distance range, outside [m0, m1)), (inside [m0, m1),
    outside the distance range) -- each well away from the filter's ends -- and (m0, m1)"""
    m0, m1 = naive.geo_morton_range(base, hi, unit)
    dlat = hi / (naive.GEO_DEG2RAD * RADIUS[unit])
    dlon = hi / (naive.GEO_DEG2RAD * RADIUS[unit] * np.cos(naive.GEO_DEG2RAD * base[0]))
    g = np.linspace(-1.3, 1.3, 301)
    la = np.repeat(base[0] + dlat * g, len(g))
    lo_ = np.tile(base[1] + dlon * g, len(g))
    for eps in (1e-5, 1e-4, 2e-4, 4e-4, 1e-3, 3e-3):  # just beyond the box's sides, where a circle wider than the box sticks out
        for side in (-1.0, 1.0):
            la = np.concatenate([la, base[0] + dlat * g])
            lo_ = np.concatenate([lo_, np.full(len(g), base[1] + side * dlon * (1.0 + eps))])
    ok = (np.abs(la) <= 90.0) & (np.abs(lo_) <= 180.0)
    codes = naive.geo_encode(la[ok], lo_[ok])
    d = naive.geo_distance(codes, base, unit)
    far = np.ones(len(d), bool)
    for end in (lo, hi):
        far &= np.abs(d - end) > 1e-6 * max(end, 1.0)
    inr = (d >= lo) & (d < hi)
    inz = (codes >= np.uint64(m0)) & (codes < np.uint64(m1))
    pick = lambda m: codes[m][np.linspace(0, m.sum() - 1, min(3, m.sum())).astype(np.int64)] if m.any() else codes[:0]
    return pick(inr & ~inz & far), pick(inz & ~inr & far), (m0, m1)


def offenders(codes, cols_in_use, sort_bases):
    """docs that break a clearance guarantee: non-determined sort keys closer than CLEAR (relative) to another doc's without being
    bit-equal (per base of sort_bases), non-determined distances within CLEAR of a value in use ({(base index, unit): values})"""
    bad = np.zeros(len(codes), bool)
    oc = origin_cluster(codes)
    for bi in sort_bases:
        nd = ~determined(codes, BASES[bi])
        key = naive.geo_distance(codes, BASES[bi], "sortkey")
        order = np.argsort(key, kind="stable")
        ks = key[order]
        close = (ks[1:] != ks[:-1]) & (ks[1:] - ks[:-1] <= np.where(oc[order][1:] & oc[order][:-1], ORIGIN_CLEAR, CLEAR) * ks[1:])
        for side in (order[:-1][close], order[1:][close]):
            bad[side[nd[side]]] = True
    for (bi, unit), values in cols_in_use.items():
        nd = ~determined(codes, BASES[bi])
        d = naive.geo_distance(codes, BASES[bi], unit)
        for v in values:
            bad |= nd & (np.abs(d - v) <= CLEAR * np.maximum(d, abs(v)))
    return bad


def _cloud(rng, n):
    """n points uniform over the globe, none within 1 deg of latitude and 1.5 deg of longitude of a base"""
    lat, lon = rng.uniform(-90.0, 90.0, n), rng.uniform(-180.0, 180.0, n)
    while True:
        near = np.zeros(n, bool)
        for b in BASES:
            near |= (np.abs(lat - b[0]) < 1.0) & (np.abs(lon - b[1]) < 1.5)
        if not near.any():
            return naive.geo_encode(lat, lon)
        lat[near], lon[near] = rng.uniform(-90.0, 90.0, near.sum()), rng.uniform(-180.0, 180.0, near.sum())


def special_codes():
    """(codes, family index) of every non-cloud doc, and the Z-range cases per filter"""
    codes, fam = [], []

    def add(name, lat, lon, rep=1):
        c = naive.geo_encode(np.asarray(lat, np.float64), np.asarray(lon, np.float64))
        codes.append(np.repeat(c, rep))
        fam.append(np.full(len(c) * rep, FAMILIES.index(name)))

    for b in BASES:
        add("coincident", [b[0]], [b[1]], N_COINCIDENT)
    for b in BASES[:2]:
        d = np.arange(1, MERIDIAN_I + 1) / 128.0
        add("meridian", np.concatenate([b[0] + d, b[0] - d]), np.full(2 * len(d), b[1]), MERIDIAN_REP)
    for b in BASES[:3]:
        e = np.arange(1, MIRROR_I + 1) / 128.0
        add("mirror", np.full(2 * len(e), -b[0]), np.concatenate([b[1] + e, b[1] - e]), MIRROR_REP)
    t = 1e-7
    add("axes", [0.0, 0.0, 0.0, 0.0, 37.5, -61.25, 5.0, -5.0], [25.0, -25.0, 140.5, -99.0, 0.0, 0.0, 0.0, 0.0], 3)
    add("axes", [t, 0.0, -t, 0.0], [0.0, t, 0.0, -t], 3)
    add("axes", [0.5, 0.5, -0.5, -0.5], [0.5, -0.5, 0.5, -0.5], 3)  # one per quadrant next to the origin
    nan = float("nan")
    add("extremes", [90.0, 90.0, -90.0, -90.0, 300.0, -300.0, 10.0, -20.0, nan, 45.0, nan],
        [180.0, -180.0, 180.0, -180.0, 10.0, -300.0, 400.0, -1000.0, 20.0, nan, nan], 3)
    zc = []
    for bi, lo, hi, unit in Z_FILTERS:
        a, b_, (m0, m1) = z_cases(BASES[bi], lo, hi, unit)
        zc.append((a, b_, m0, m1))
        c = np.concatenate([a, b_, np.array([m0, m1], np.uint64)])
        codes.append(np.repeat(c, 3))
        fam.append(np.full(3 * len(c), FAMILIES.index("zrange")))
    return np.concatenate(codes), np.concatenate(fam), zc


def build(O):
    """the world over the CPU oracle O (oracle/oracle.py): corpus, oracle shard, records, families, queries and every query's matches"""
    W = World()
    W._dist = {}
    th = O.term_thresholds().copy()
    for t, f in enumerate(DFS):
        th[t] = int(f * 2.0 ** 32)
    W.offs, W.docs, W.tfs = O.lex_corpus(N_DOCS, list(range(len(DFS))), thresholds=th)
    W.dl = O.lex_doclen(N_DOCS)
    W.osh = O.Shard(N_DOCS, W.dl, W.offs, W.docs, W.tfs)
    W.gone = list(range(13, N_DOCS, 997))
    W.osh.set_deleted(W.gone)
    rng = np.random.default_rng(4207)
    # the special docs: at ids that hold terms 3 AND 4, spread over both levels
    sc, sf, W.z_cases = special_codes()
    pool, _, _ = W.osh.search_exhaustive([3, 4], O.OP_AND, N_DOCS)
    pool = np.sort(pool.astype(np.int64))
    assert len(pool) > 2 * len(sc)
    at = rng.choice(pool, len(sc), replace=False)
    loc = _cloud(rng, N_DOCS)
    W.family = np.zeros(N_DOCS, np.int64)
    loc[at], W.family[at] = sc, sf
    loc2 = _cloud(rng, N_DOCS)
    use = {col: {(bi, unit): v for (c, bi, unit), v in IN_USE.items() if c == col} for col in ("loc", "loc2")}
    for col, codes, sort_bases in (("loc", loc, range(len(BASES))), ("loc2", loc2, ())):
        for _ in range(50):
            bad = offenders(codes, use[col], sort_bases) & (W.family == 0 if col == "loc" else True)
            if not bad.any():
                break
            codes[bad] = _cloud(rng, int(bad.sum()))
        else:
            raise AssertionError("the cloud does not settle")
    rec = np.zeros(N_DOCS + N_EXTRA, REC)
    rec["loc"][:N_DOCS], rec["loc2"][:N_DOCS] = loc, loc2
    rec["h"][:N_DOCS] = rng.integers(0, 50000, N_DOCS)
    on_base = naive.geo_encode([b[0] for b in BASES], [b[1] for b in BASES])
    rec["loc"][N_DOCS:] = rec["loc2"][N_DOCS:] = on_base[np.arange(N_EXTRA) % len(BASES)]  # the best answers, if a kernel read them
    W.rec = rec
    W.raw = rec.view(np.uint8).reshape(N_DOCS + N_EXTRA, REC.itemsize)
    W.det = [determined(rec["loc"][:N_DOCS], b) for b in BASES]
    # (terms, union?, NOT terms): ~20 matches, hundreds, thousands, the special docs' intersection, most of the corpus, a NOT term that
    # removes every special doc, none, one
    W.queries = [([0], True, []), ([1], True, []), ([2, 1], True, []), ([3, 4], False, []), ([4, 3, 2], True, []), ([4], True, [3]),
                 ([0, 1], False, []), ([0, 3], False, [4])]
    W.sees_all = (3, 4)  # the queries that match every special doc
    W.matches = []
    for terms, union, neg in W.queries:  # every match with its score, by (score desc, doc asc)
        md, ms, tot = W.osh.search_exhaustive(terms, O.OP_OR if union else O.OP_AND, N_DOCS, neg)
        assert len(md) == tot
        W.matches.append((md.astype(np.int64), ms))
    return W


# ------------------------------------------------------------------ references
def point_filter(W, col, bi, lo, hi, unit, flags=0):
    """(the filter tuple Shard.facet_filters takes, the reference's keep mask over the docs)"""
    keep = naive.geo_pass(W.rec[col][:N_DOCS], BASES[bi], lo, hi, unit, flags)
    t = (OFF[col], "point", BASES[bi], lo, hi, unit) + ((flags,) if flags else ())
    return t, keep


def h_filter(W, lo, hi):
    return (OFF["h"], "u16", lo, hi), (W.rec["h"][:N_DOCS] >= lo) & (W.rec["h"][:N_DOCS] < hi)


def each_sets(W):
    """the filter sets of a batch whose queries each carry their own: neighbouring bases and units differ, one set is empty, one passes
    nothing (its Z range is empty), one is over the second column, one in the pivot form, one holds two filters"""
    return [[point_filter(W, "loc", 0, 0.0, 500.0, "km")], [point_filter(W, "loc", 1, 50.0, 400.0, "miles")], [],
            [point_filter(W, "loc", 2, 0.0, 500.0, "km")],
            [point_filter(W, "loc2", *LOC2_FILTERS[0])], [point_filter(W, "loc", 0, 100.0, 300.0, "miles")],
            [point_filter(W, "loc", 0, step_distance(5, "sortkey"), step_distance(20, "sortkey"), "sortkey", LO | HI)],
            [point_filter(W, "loc", 4, 0.0, 100.0, "km"), h_filter(W, 0, 40000)], [point_filter(W, "loc", 1, 0.0, 1000.0, "km")]]


def want_counts(W, col, bi, unit, bounds, docs):
    """(counts per range, "other") of docs: the last lower bound <= distance (facet_bucket, vectorised); below the first: other"""
    b = np.searchsorted(np.asarray(bounds, np.float64), W.dist(col, bi, unit)[docs], side="right") - 1
    return np.bincount(b[b >= 0], minlength=len(bounds)).astype(np.int64), int((b < 0).sum())


def want_counts_h(W, bounds, docs):
    b = np.searchsorted(np.asarray(bounds, np.int64), W.rec["h"][docs].astype(np.int64), side="right") - 1
    return np.bincount(b[b >= 0], minlength=len(bounds)).astype(np.int64), int((b < 0).sum())


def sort_columns(W, srt):
    """srt = [(column, descending, base index or None for a numeric column)] -> each doc's value per field (f64)"""
    return [W.dist(c, bi, "sortkey") if bi is not None else W.rec[c][:N_DOCS].astype(np.float64) for c, _, bi in srt]


def sort_spec(srt):
    return [(OFF[c], "point", d, BASES[bi]) if bi is not None else (OFF[c], "u16", d) for c, d, bi in srt]


def reference_order(W, qi, srt, keep=None):
    """query qi's matches in result-sort order: the fields, then score descending, then doc ascending -> (docs, scores, all matches)"""
    md, ms = W.matches[qi]
    if keep is not None:
        ms, md = ms[keep[md]], md[keep[md]]
    cols = [(-c[md] if d else c[md]) for c, (_, d, _) in zip(sort_columns(W, srt), srt)]
    order = np.lexsort((md, -ms.astype(np.float64)) + tuple(reversed(cols)))
    return md[order], ms[order], md


# ------------------------------------------------------------------ checks (every one raises AssertionError on a wrong answer)
REL = 1e-4  # the suite's tolerance for BM25 scores


def check_sorted(W, doc, score, total, ref, srt, k, what):
    """a sorted answer against reference_order's: count min(k, matches), no doc twice, none beyond the lexical image, every sort field
    bit-equal to the reference's position by position, scores within REL of the reference's at the position and of the doc's own, and
    where fields and returned scores tie the docs ascend"""
    od, os_, md = ref
    n = min(k, len(od))
    doc = np.asarray(doc, np.int64)
    score = np.asarray(score, np.float32)
    assert total == len(md), (what, "total", total, len(md))
    assert len(doc) == n, (what, "count", len(doc), n)
    assert len(set(doc.tolist())) == n, (what, "a doc twice")
    assert np.all(doc < N_DOCS), (what, "a record beyond the lexical image")
    cols = sort_columns(W, srt)
    tie = np.ones(max(n - 1, 0), bool)
    for c, f in zip(cols, srt):
        got, want = c[doc] + 0.0, c[od[:n]] + 0.0
        bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        assert len(bad) == 0, (what, "field", f, "position", int(bad[0]), "doc", int(doc[bad[0]]), "reference doc", int(od[bad[0]]))
        tie &= got[1:] == got[:-1]
    assert np.allclose(score, os_[:n], rtol=REL), (what, "scores", np.nonzero(~np.isclose(score, os_[:n], rtol=REL))[0][:5])
    assert np.all(np.isin(doc, md)), (what, "a doc that does not match")
    own = dict(zip(od.tolist(), os_.tolist()))
    assert np.allclose(score, [own[d] for d in doc.tolist()], rtol=REL), (what, "own scores")
    tie &= score[1:].view(np.uint32) == score[:-1].view(np.uint32)
    bad = np.nonzero(tie & (doc[1:] < doc[:-1]))[0]
    assert len(bad) == 0, (what, "tied docs out of doc order", int(doc[bad[0]]), int(doc[bad[0] + 1]))


def check_counts(got, want, what):
    """(counts, other, total) against the reference's, every bucket"""
    gc, go, gt = got
    wc, wo, wt = want
    assert int(gt) == int(wt), (what, "total", int(gt), int(wt))
    assert np.array_equal(np.asarray(gc, np.int64), np.asarray(wc, np.int64)), (what, "counts", list(map(int, gc)), list(map(int, wc)))
    assert int(go) == int(wo), (what, "other", int(go), int(wo))


def check_filtered(W, doc, score, cnt, total, qi, keep, k, what):
    """a filtered top-k: the exact total, the suite's top-k rule on the hits, and every returned doc passes the reference's filter"""
    from test_gpu_parity import _check_topk
    md, ms = W.matches[qi]
    kept = keep[md]
    assert int(total) == int(kept.sum()), (what, "total", int(total), int(kept.sum()))
    _check_topk(np.asarray(doc), np.asarray(score), cnt, md[kept][:k], ms[kept][:k])
    out = [int(d) for d in np.asarray(doc)[:int(cnt)] if not keep[int(d)]]
    assert not out, (what, "docs the filter excludes", out[:5])
