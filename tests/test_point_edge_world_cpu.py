"""The Point edge world (tests/point_edge_world.py) is what it claims, proven on the CPU: oracle/naive.py's geo_* and the C oracle's
agree over every doc of it, every family is among the matches of the queries meant to see it, determined tie groups straddle every k
the GPU tests page at, the clearances hold for every doc (none is skipped for being "too close"), the Z-range cases are there, and
the shared checks refuse altered answers."""
import numpy as np
import pytest

import point_edge_world as PW
from oracle import naive
from oracle import oracle as O

UNITS = ("km", "miles", "sortkey")


@pytest.fixture(scope="module")
def W():
    return PW.build(O)


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


def test_naive_and_oracle_geo_agree_over_the_world(W):
    """codes and Morton ranges bit-equal, distances within 2 ulp (numpy's cos may differ from libm's), bit-equal on the determined docs"""
    lat = np.array([12.5, -33.25, 0.0, 1e-7, -1e-7, 90.0, -90.0, 300.0, -300.0, float("nan"), 214.7483647, -214.7483648, 89.9999999])
    lon = np.array([40.0, -70.5, -0.0, -1e-7, 1e-7, 180.0, -180.0, 10.0, -1000.0, float("nan"), 179.9999999, 1e300, float("inf")])
    assert np.array_equal(naive.geo_encode(lat, lon), O.morton_encode(lat, lon))
    assert [int(x) for x in naive.geo_encode([1e-7, 0.0, float("nan")], [0.0, 1e-7, float("nan")])] == [1, 2, 0]
    for col in ("loc", "loc2"):
        codes = W.rec[col]
        dla, dlo = naive.geo_decode(codes)
        assert np.array_equal(np.stack([dla, dlo], 1), O.morton_decode(codes))
        for bi, base in enumerate(PW.BASES):
            det = PW.determined(codes, base)
            for unit in UNITS:
                u = _ulps(naive.geo_distance(codes, base, unit), O.geo_distances(codes, base, unit))
                assert u.max() <= 2, (col, base, unit, int(u.max()))
                assert u[det].max() == 0, (col, base, unit)
    ends = sorted({(bi, hi, unit) for (c, bi, unit), v in PW.IN_USE.items() for hi in v if unit != "sortkey"})
    assert len(ends) > 30
    for bi, hi, unit in ends:
        assert naive.geo_morton_range(PW.BASES[bi], hi, unit) == O.geo_morton_range(PW.BASES[bi], hi, unit), (bi, hi, unit)


def test_the_shape_of_the_world(W):
    assert PW.N_DOCS > 65536 and PW.N_DOCS % 64 != 0 and PW.OFF["loc"] % 2 == 1 and PW.OFF["loc2"] % 2 == 1 and PW.REC.itemsize % 2 == 1
    assert len(W.rec) == PW.N_DOCS + PW.N_EXTRA and 10 < len(W.gone) < 100
    n = [len(m[0]) for m in W.matches]
    assert n[0] < 30 and 100 < n[1] < 1000 and 1030 < n[2] < 5000 and n[3] > 10000 and n[4] > 60000 and n[5] > 1030 and n[6:] == [0, 1]
    # the 40 records beyond the image sit exactly on the bases: distance 0 to one of them each
    for bi in range(len(PW.BASES)):
        d = naive.geo_distance(W.rec["loc"][PW.N_DOCS:], PW.BASES[bi], "km")
        assert (d == 0.0).sum() == PW.N_EXTRA // len(PW.BASES)
    assert not np.isin(W.gone, np.nonzero(W.family)[0]).any()  # no special doc is tombstoned
    special = np.nonzero(W.family)[0]
    assert special.min() < 2000 and (special > 65536).sum() > 50  # spread over both levels
    assert W.family[W.matches[5][0]].max() == 0  # the NOT query sees the cloud alone


def test_every_family_is_among_the_matches(W):
    lat, lon = naive.geo_decode(W.rec["loc"][:PW.N_DOCS])
    codes = W.rec["loc"][:PW.N_DOCS]
    for qi in W.sees_all:
        m = np.zeros(PW.N_DOCS, bool)
        m[W.matches[qi][0]] = True
        assert np.all(m[W.family != 0])
        for f in range(len(PW.FAMILIES)):
            assert (m & (W.family == f)).any(), PW.FAMILIES[f]
        for q in ((lat > 0) & (lon > 0), (lat > 0) & (lon < 0), (lat < 0) & (lon > 0), (lat < 0) & (lon < 0)):
            assert (m & q & (W.family == 0)).sum() > 1000  # the cloud in all four quadrants
        for bi, b in enumerate(PW.BASES):
            assert (m & (W.dist("loc", bi, "km") == 0.0)).sum() >= 30  # coincident: distance 0 ...
            key = W.dist("loc", bi, "sortkey")
            assert np.all(key[W.dist("loc", bi, "km") == 0.0].view(np.uint64) == 0)  # ... and key +0.0
        for want in (1, 2, 0, int(naive.geo_encode(-1e-7, 0.0)[0]), int(naive.geo_encode(0.0, -1e-7)[0])):
            assert (m & (codes == np.uint64(want))).any(), want
        for la, lo in ((90.0, 180.0), (-90.0, -180.0), (214.7483647, 10.0), (-214.7483648, -214.7483648), (10.0, 214.7483647)):
            assert (m & (lat == la) & (lon == lo)).any(), (la, lo)  # the poles' corners; inputs beyond i32 saturate as the writer's cast
        assert (m & (lat == 0.0) & (lon != 0.0)).any() and (m & (lon == 0.0) & (lat != 0.0)).any()
    # the +- pairs of the meridian and mirror families tie bit for bit, and each family is determined for its base
    for bi in (0, 1):
        b = PW.BASES[bi]
        for unit in UNITS:
            d = W.dist("loc", bi, unit)
            for i in (1, 7, PW.MERIDIAN_I):
                up, dn = (lon == b[1]) & (lat == b[0] + i / 128.0), (lon == b[1]) & (lat == b[0] - i / 128.0)
                assert up.sum() == dn.sum() == PW.MERIDIAN_REP and len(set(d[up | dn].view(np.uint64).tolist())) == 1
                assert d[up][0] == PW.step_distance(i, unit)
    for bi in (0, 1, 2):
        b = PW.BASES[bi]
        for unit in UNITS:
            d = W.dist("loc", bi, unit)
            for i in (1, PW.MIRROR_I):
                e, w_ = (lat == -b[0]) & (lon == b[1] + i / 128.0), (lat == -b[0]) & (lon == b[1] - i / 128.0)
                assert e.sum() >= PW.MIRROR_REP and w_.sum() >= PW.MIRROR_REP and len(set(d[e | w_].view(np.uint64).tolist())) == 1
                assert np.all(W.det[bi][e | w_])


def test_the_clearances_hold_for_every_doc(W):
    """no doc is left out: offenders() over the whole columns finds none, and the figures themselves are asserted once more here"""
    use = {col: {(bi, unit): v for (c, bi, unit), v in PW.IN_USE.items() if c == col} for col in ("loc", "loc2")}
    assert not PW.offenders(W.rec["loc"][:PW.N_DOCS].copy(), use["loc"], range(len(PW.BASES))).any()
    assert not PW.offenders(W.rec["loc2"][:PW.N_DOCS].copy(), use["loc2"], ()).any()
    for (col, bi, unit), values in PW.IN_USE.items():
        d = W.dist(col, bi, unit)
        nd = ~PW.determined(W.rec[col][:PW.N_DOCS], PW.BASES[bi])
        for v in values:
            assert np.all(np.abs(d[nd] - v) > PW.CLEAR * np.maximum(d[nd], abs(v))), (col, bi, unit, v)
    for bi in range(len(PW.BASES)):
        key = W.dist("loc", bi, "sortkey")
        order = np.argsort(key, kind="stable")
        ks, nd = key[order], ~W.det[bi][order]
        gap = ks[1:] - ks[:-1]
        oc = PW.origin_cluster(W.rec["loc"][:PW.N_DOCS])[order]
        assert oc.sum() == 12 + PW.N_COINCIDENT + 3  # (0, 0) 32 times and its four neighbours 3 times each; the NaN inputs' code 0
        near = (gap != 0) & (gap <= np.where(oc[1:] & oc[:-1], PW.ORIGIN_CLEAR, PW.CLEAR) * ks[1:])
        assert not (near & (nd[1:] | nd[:-1])).any(), bi
    assert max(max(v) for v in PW.IN_USE.values()) > max(W.dist("loc", 0, "km").max(), W.dist("loc", 2, "km").max())  # a bound above all


def test_determined_tie_groups_straddle_every_k(W):
    """k = 1, 10, 64, 1030: some (query, base, direction) whose ranks k and k + 1 are determined docs with bit-equal keys; the
    coincident group lies at the head of every ascending sort and at the tail of every descending one"""
    found = {1: [], 10: [], 64: [], 1030: []}
    for qi in W.sees_all:
        for bi in range(len(PW.BASES)):
            for desc in (False, True):
                od, _, _ = PW.reference_order(W, qi, [("loc", desc, bi)])
                key, det = W.dist("loc", bi, "sortkey")[od], W.det[bi][od]
                zero = np.nonzero(key == 0.0)[0]
                assert len(zero) >= 30 and (zero[0] == 0 if not desc else zero[-1] == len(od) - 1)
                for k in found:
                    if key[k - 1] == key[k] and det[k - 1] and det[k]:
                        found[k].append((qi, bi, desc))
    assert all(found.values()), found
    assert any(not d for _, _, d in found[1030]) and any(bi == 1 for _, bi, _ in found[1030])


def test_the_z_range_cases(W):
    codes = W.rec["loc"][:PW.N_DOCS]
    kinds = set()
    for (bi, lo, hi, unit), (a, b, m0, m1) in zip(PW.Z_FILTERS, W.z_cases):
        d = W.dist("loc", bi, unit)
        inr = (d >= lo) & (d < hi)
        inz = (codes >= np.uint64(m0)) & (codes < np.uint64(m1))
        _, keep = PW.point_filter(W, "loc", bi, lo, hi, unit)
        assert np.array_equal(keep, inr & inz)
        assert (codes == np.uint64(m0)).sum() >= 3 and (codes == np.uint64(m1)).sum() >= 3  # docs exactly on m0 and on m1
        if m0 < m1:
            assert np.all(inz[codes == np.uint64(m0)]) and not inz[codes == np.uint64(m1)].any()  # m0 is inside the range, m1 is not
            kinds.add("on the ends")
            assert (inz & ~inr).any()
            if (inr & ~inz).any():
                kinds.add("non-empty, in-circle docs outside")
                assert keep.any()
        else:
            assert not inz.any() and inr.sum() >= 30 and not keep.any()
            kinds.add("empty")
    assert kinds == {"on the ends", "non-empty, in-circle docs outside", "empty"}
    # the bases the issue names: B2's and B4's wide boxes are empty ranges, B0's and B1's are proper ones
    empty = {(bi, hi) for (bi, _, hi, _), (_, _, m0, m1) in zip(PW.Z_FILTERS, W.z_cases) if m0 > m1}
    assert {bi for bi, _ in empty} == {2, 4}
    # the exact filters: ends on determined distances that docs hold
    for bi, lo, hi, unit in PW.EXACT_FILTERS:
        d = W.dist("loc", bi, unit)
        assert all((d == x).sum() >= 2 * PW.MERIDIAN_REP for x in (lo, hi) if x in [PW.step_distance(i, unit) for i in range(1, 51)])
    _, keep = PW.point_filter(W, "loc", *PW.EXACT_FILTERS[0])
    assert keep.sum() == 15 * 2 * PW.MERIDIAN_REP  # [d5, d20): steps 5..19, both sides
    assert not PW.point_filter(W, "loc", *PW.EXACT_FILTERS[1])[1].any() and not PW.point_filter(W, "loc", *PW.EXACT_FILTERS[2])[1].any()
    b0, lo, hi, unit = PW.EXACT_FILTERS[1]
    assert PW.point_filter(W, "loc", b0, lo, hi, unit, PW.HI)[1].sum() == 2 * PW.MERIDIAN_REP  # lo == hi, hi inclusive: that step alone


def test_the_checks_reject_altered_answers(W):
    """check_sorted, check_counts and check_filtered on hand-altered reference answers: a doc from the wrong quadrant swapped in, two
    tied docs in the wrong doc order, a count moved to the neighbouring bucket, a doc that only the Z range excludes -- each must be
    refused; the unaltered answers pass"""
    qi, bi, k = 4, 0, 64
    srt = [("loc", False, bi)]
    ref = PW.reference_order(W, qi, srt)
    od, os_, md = ref
    good_d, good_s = od[:k].copy(), os_[:k].astype(np.float32)
    PW.check_sorted(W, good_d, good_s, len(md), ref, srt, k, "good")
    lat, lon = naive.geo_decode(W.rec["loc"][:PW.N_DOCS])
    sw = next(int(d) for d in od[k:] if lat[d] < 0 and lon[d] < 0)  # B0 lies north-east
    d = good_d.copy()
    d[40] = sw
    with pytest.raises(AssertionError, match="field"):
        PW.check_sorted(W, d, good_s, len(md), ref, srt, k, "quadrant")
    key = W.dist("loc", bi, "sortkey")[good_d]
    tied = [i for i in range(k - 1) if key[i] == key[i + 1] and good_s[i] == good_s[i + 1]]
    assert tied  # two docs of a determined group with the same score
    d = good_d.copy()
    d[tied[0]], d[tied[0] + 1] = d[tied[0] + 1], d[tied[0]]
    with pytest.raises(AssertionError, match="out of doc order"):
        PW.check_sorted(W, d, good_s, len(md), ref, srt, k, "tie order")
    with pytest.raises(AssertionError, match="beyond the lexical image"):
        PW.check_sorted(W, np.append(good_d[:-1], PW.N_DOCS), good_s, len(md), ref, srt, k, "extra record")
    col, cbi, unit, bounds = PW.COUNT_CASES[0]
    wc, wo = PW.want_counts(W, col, cbi, unit, bounds, md)
    PW.check_counts((wc, wo, len(md)), (wc, wo, len(md)), "good")
    assert wc[0] >= 30 and wc[1] > 0  # distance 0 lands in bucket 0; the determined bound holds its own docs
    moved = wc.copy()
    moved[0] -= 1
    moved[1] += 1
    with pytest.raises(AssertionError, match="counts"):
        PW.check_counts((moved, wo, len(md)), (wc, wo, len(md)), "moved")
    # a doc only the Z range excludes, put at the head of the filtered answer it does not belong to
    fi = next(i for i, (a, _, m0, m1) in enumerate(W.z_cases) if len(a) and m0 < m1)
    fbi, lo, hi, unit = PW.Z_FILTERS[fi]
    _, keep = PW.point_filter(W, "loc", fbi, lo, hi, unit)
    dd = W.dist("loc", fbi, unit)
    ms_all = W.matches[qi][1]
    kept = keep[md_all := W.matches[qi][0]]
    gd, gs = md_all[kept][:10].astype(np.uint32), ms_all[kept][:10].astype(np.float32)
    PW.check_filtered(W, gd, gs, len(gd), int(kept.sum()), qi, keep, 10, "good")
    only_z = [int(x) for x in md_all if (lo <= dd[x] < hi) and not keep[x]]
    assert only_z
    bd = gd.copy()
    bd[-1] = only_z[0]
    with pytest.raises(AssertionError):
        PW.check_filtered(W, bd, gs, len(bd), int(kept.sum()), qi, keep, 10, "z only")


def test_the_per_query_filter_sets(W):
    """of the nine sets exactly one passes nothing for the two queries that see every family, the others pass some docs, and no two
    sets pass the same number: a row answered under its neighbour's set would show"""
    totals = []
    for fs in PW.each_sets(W):
        keep = np.logical_and.reduce([k for _, k in fs]) if fs else np.ones(PW.N_DOCS, bool)
        totals.append(tuple(int(keep[W.matches[qi][0]].sum()) for qi in W.sees_all))
    assert [t for t in totals if 0 in t] == [(0, 0)] and totals[3] == (0, 0)
    assert len(set(totals)) == len(totals) and len({x for t in totals for x in t}) > 10
    assert totals[2] == tuple(len(W.matches[qi][0]) for qi in W.sees_all)
